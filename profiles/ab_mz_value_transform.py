#!/usr/bin/env python3
"""What the value transform costs (MuZeroNet(value_transform=True): k_mz_search's VT instantiations, k_mzr_sample<true>) and what
the greedy evaluation shows, in one process, HIP events on the launch stream, medians after warm-up -- the method of
profiles/ab_mz_whole_env.py, whose helpers are reused.

  moves     moves/s of whole-move self-play at 50 simulations, ``collect(16)`` between two events, for CartPole and Acrobot at 256 and
            at 8192 environments: the flag off | the flag on, and with --parent DIR (a checkout of the parent commit with its library
            built) the parent's run TWICE, as two players; the players of one size and environment alternate and the round starts one
            player further on every time.  The flag-off route counts as unchanged if it lies within the spread of the two parent
            players; otherwise the file says by how much it does not.
  sample    ``MuZeroDeviceReplay.sample(256)`` with the flag on against off: 512 stored episodes of 100 steps, K = 5, td_steps = 10.
  build     seconds hipcc takes for csrc/rz_muzero.hip with the flags of rlzero_amd/_build.py, this tree and --parent (the
            instantiations of k_mz_search double); needs no GPU.
  learning  ONE observation each, no claim: tools/train_muzero.py's pipeline at 256 environments, 60 iterations, --device-replay
            --fused-learner --eval-every 10, for CartPole and for Acrobot, with and without --value-transform; the eval lines.

    python profiles/ab_mz_value_transform.py [--out profiles/mz_value_transform/ab.txt] [--reps 30] [--parent DIR] [--parts moves,sample,build,learning]

No figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import contextlib
import io
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ab_mz_env import MOVES, timed  # noqa: E402
from ab_mz_reanalyse import load_trainer, spread  # noqa: E402


def part_moves(args, torch, say):
    import rlzero_amd.muzero as here
    say('moves: whole moves, %d simulations, collect(%d) between two events, %d repetitions after 3, the players of one size and environment '
        'alternating (each round starts one player further on); moves/s = environments x %d / the median' % (args.sims, MOVES, args.reps, MOVES))
    parent = None
    if args.parent:
        load_trainer(os.path.abspath(args.parent), 'rlzero_amd_parent')
        parent = sys.modules['rlzero_amd_parent.muzero']
    for n_envs in (256, args.envs):
        for kind in ('cartpole', 'acrobot'):
            routes = [('flag off', here, {}), ('flag on', here, dict(value_transform=True))]
            if parent is not None:
                routes = [('parent (1)', parent, {})] + routes + [('parent (2)', parent, {})]
            players = []
            for name, mod, net_kw in routes:
                torch.manual_seed(args.seed)
                env = (mod.CartPoleBatch if kind == 'cartpole' else mod.AcrobotBatch)(n_envs, 'cuda:0', seed=args.seed)
                net = mod.MuZeroNet(env.obs_dim, env.n_actions, **net_kw).to('cuda:0').eval()
                sp = mod.MuZeroSelfPlay(net, env, n_sims=args.sims, seed=args.seed, moves_per_launch=MOVES, fused_moves=True)
                assert sp.fused_moves and getattr(sp.tree, 'value_transform', False) == bool(net_kw)
                players.append(sp)
            say('  %5d environments  %-9s plan: %s' % (n_envs, kind, players[0].tree.search_plan(whole_moves=True)))
            ms = [[] for _ in players]
            for rep in range(args.reps + 3):
                for j in range(len(players)):
                    i = (rep + j) % len(players)
                    x = timed(torch, lambda: players[i].collect(MOVES))
                    if rep >= 3:
                        ms[i].append(x)
            med = {}
            for (name, _, _), xs, sp in zip(routes, ms, players):
                med[name] = statistics.median(xs)
                say('  %5d environments  %-9s %-11s ms per %d moves: %s   -> %.0f moves/s' % (n_envs, kind, name, MOVES, spread(xs),
                                                                                            1e3 * n_envs * MOVES / med[name]))
                sp.tree.check()
                sp.close()
            say('  %5d environments  %-9s flag on / flag off = %.3f' % (n_envs, kind, med['flag on'] / med['flag off']))
            if parent is not None:
                a, b, c = med['parent (1)'], med['parent (2)'], med['flag off']
                lo, hi = min(a, b), max(a, b)
                verdict = 'within the spread of the two parent players' if lo <= c <= hi else \
                    'OUTSIDE the spread of the two parent players by %.3f ms (%.2f %% of the nearer one)' % (
                        (lo - c) if c < lo else (c - hi), 100.0 * ((lo - c) / lo if c < lo else (c - hi) / hi))
                say('  %5d environments  %-9s the two parent players: medians %.3f and %.3f ms; flag off: %.3f ms, %s'
                    % (n_envs, kind, a, b, c, verdict))
            else:
                say('  parent commit: not measured (no --parent)')


def part_sample(args, torch, say):
    import numpy as np
    from rlzero_amd.muzero import MuZeroDeviceReplay
    D, A, E, T, n = 6, 3, 512, 100, 256
    rng = np.random.RandomState(args.seed)
    block = np.zeros((E * T, D + 4 + A))
    block[:, :D] = rng.standard_normal((E * T, D))
    block[:, D] = rng.randint(A, size=E * T)
    block[:, D + 1] = -1.0
    block[:, D + 2:D + 2 + A] = rng.randint(1, 20, size=(E * T, A))
    block[:, D + 2 + A] = -rng.uniform(1.0, 90.0, size=E * T)
    bufs = []
    for on in (False, True):
        buf = MuZeroDeviceReplay(D, A, E, T, device='cuda:0', seed=args.seed, value_transform=on)
        buf.add_packed(block, [T] * E)
        bufs.append(buf)
    ms = [[], []]
    for rep in range(args.reps + 3):
        for j in range(2):
            i = (rep + j) % 2
            x = timed(torch, lambda: bufs[i].sample(n, step=rep))
            if rep >= 3:
                ms[i].append(x)
    say('sample: MuZeroDeviceReplay.sample(%d), %d episodes of %d steps held, K = 5, td_steps = 10; ms per call (launch + the six output '
        'tensors), %d repetitions after 3, the two buffers alternating' % (n, E, T, args.reps))
    for name, xs, buf in zip(('flag off', 'flag on'), ms, bufs):
        say('  %-9s %s' % (name, spread(xs)))
        assert buf.poll_errors() == 0
        buf.close()
    say('  flag on / flag off = %.3f' % (statistics.median(ms[1]) / statistics.median(ms[0])))


def part_build(args, torch, say):
    sys.path.insert(0, REPO)
    from rlzero_amd import _build
    say('build: seconds for `hipcc %s -c csrc/rz_muzero.hip` (the flags of rlzero_amd/_build.py), best of 2, on the host that ran this part'
        % ' '.join(_build.FLAGS))
    for name, repo in (('this tree', REPO), ('parent', os.path.abspath(args.parent) if args.parent else None)):
        if repo is None:
            say('  parent commit: not measured (no --parent)')
            continue
        best = None
        with tempfile.TemporaryDirectory() as tmp:
            for _ in range(2):
                t0 = time.perf_counter()
                subprocess.run([os.environ.get('HIPCC', 'hipcc')] + _build.FLAGS + ['-I' + os.path.join(repo, 'include'), '-DRZ_SOURCE_HASH="x"', '-c',
                                os.path.join(repo, 'rlzero_amd', 'csrc', 'rz_muzero.hip'), '-o', os.path.join(tmp, 'x.o')], check=True)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
        say('  %-10s %.1f s' % (name, best))


def part_learning(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    say('learning (ONE observation each, same seed; no claim): MuZeroPipeline(256 environments, device replay, fused learner).run(60, eval_every=10); '
        'the evaluation: 256 environments of its own, temperature 0, no root noise, the same initial states every time')
    for env in ('cartpole', 'acrobot'):
        for on in (False, True):
            torch.manual_seed(args.seed)
            with as_here():
                pipe = here.MuZeroPipeline(env=env, device_replay=True, fused_learner=True, seed=args.seed, value_transform=on)
            t0 = time.perf_counter()
            log = io.StringIO()
            with contextlib.redirect_stdout(log):
                pipe.run(60, eval_every=10)
            torch.cuda.synchronize()
            lines = log.getvalue().splitlines()
            batch = [ln for ln in lines if ln.startswith('batch i:')]
            say('  %s%s   (%.1f s for the 60 iterations and 6 evaluations; self-play episode_len of the last iteration %.1f)'
                % (env, ' --value-transform' if on else '', time.perf_counter() - t0, pipe.episode_len))
            for ln in lines:
                if ln.startswith('eval i:'):
                    say('    ' + ln)
            if batch:
                say('    last progress line: ' + batch[-1])
            pipe.selfplay.tree.check()
            pipe.selfplay.close()
            if pipe._evaluator is not None:
                pipe._evaluator[0].close()
            pipe.buffer.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mz_value_transform', 'ab.txt'))
    ap.add_argument('--envs', type=int, default=8192)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--parent', default='', help='a checkout of the parent commit with its library built')
    ap.add_argument('--parts', default='moves,sample,build,learning')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    parts = {'moves': part_moves, 'sample': part_sample, 'build': part_build, 'learning': part_learning}
    wanted = args.parts.split(',')
    torch, device = None, 'no GPU'
    if wanted != ['build']:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('profiles/ab_mz_value_transform.py measures on the GPU: none here (--parts build needs none)')
        device = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_mz_value_transform.py --parts %s: %s; HIP events on the launch stream' % (args.parts, device))
    for part in wanted:
        parts[part](args, torch, say)
    out.close()


if __name__ == '__main__':
    main()
