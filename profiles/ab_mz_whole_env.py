#!/usr/bin/env python3
"""What whole moves buy Acrobot next to device moves and the host loop (MuZeroSelfPlay(fused_moves=True) on an AcrobotBatch:
rz_mz_play_env, k_mz_search<TREE_LDS, MOVES = true, EnvAcrobot>), in one process, HIP events on the launch stream, medians after
warm-up -- the method of profiles/ab_mz_env.py, whose helpers are reused.

  moves       moves/s of Acrobot self-play at 50 simulations, ``collect(16)`` between two events: whole moves with the automatic shape
              (16 games per workgroup: the three-action trees stay in HBM) | whole moves with 8 games per workgroup (trees in LDS) |
              device moves | the host loop, at 256 and at 8192 environments; the routes of one size alternate and the round starts one
              route further on every time.  CartPole's whole moves on this tree run in the same rounds, and with --parent DIR (a
              checkout of the parent commit with its library built) the parent's run TWICE, as two players: CartPole counts as
              unchanged if this tree lies within the spread of the two.
  iteration   the iteration of tools/train_muzero.py at 8192 environments with --device-replay --fused-learner for Acrobot with and
              without --whole-moves.
  learning    ONE observation, no claim: MuZeroPipeline(env='acrobot', whole_moves=True, 256 environments, device replay, fused
              learner).run(60), same seed as profiles/ab_mz_env.py.

    python profiles/ab_mz_whole_env.py [--out profiles/mz_whole_env/ab.txt] [--reps 30] [--parent DIR] [--parts moves,iteration,learning]

No figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ab_mz_env import MOVES, timed  # noqa: E402
from ab_mz_reanalyse import load_trainer, spread  # noqa: E402


def part_moves(args, torch, say):
    import rlzero_amd.muzero as here
    say('moves: %d simulations, collect(%d) between two events, %d repetitions after 3, the routes of one size alternating (each round '
        'starts one route further on); moves/s = environments x %d / the median' % (args.sims, MOVES, args.reps, MOVES))
    routes = [('acrobot', 'whole moves, auto shape', here, dict(fused_moves=True), 0),
              ('acrobot', 'whole moves, 8 per wg', here, dict(fused_moves=True), 8),
              ('acrobot', 'device moves', here, dict(), 0),
              ('acrobot', 'host loop', here, dict(device_moves=False), 0),
              ('cartpole', 'whole moves', here, dict(), 0)]
    if args.parent:
        load_trainer(os.path.abspath(args.parent), 'rlzero_amd_parent')
        parent = sys.modules['rlzero_amd_parent.muzero']
        routes = routes[:4] + [('cartpole', 'whole moves, parent (1)', parent, dict(), 0), routes[4],
                               ('cartpole', 'whole moves, parent (2)', parent, dict(), 0)]
    for n_envs in (256, args.envs):
        players = []
        for kind, name, mod, kw, gpw in routes:
            torch.manual_seed(args.seed)
            env = (mod.CartPoleBatch if kind == 'cartpole' else mod.AcrobotBatch)(n_envs, 'cuda:0', seed=args.seed)
            net = mod.MuZeroNet(env.obs_dim, env.n_actions).to('cuda:0').eval()
            sp = mod.MuZeroSelfPlay(net, env, n_sims=args.sims, seed=args.seed, moves_per_launch=MOVES, **kw)
            assert (sp.fused_moves, sp.device_moves) == (name.startswith('whole moves'), name == 'device moves')
            sp.tree.set_search_shape(gpw)
            players.append(sp)
        for (kind, name, _, _, _), sp in zip(routes, players):
            if sp.fused_moves:
                say('  %5d environments  %-9s %-24s plan: %s' % (n_envs, kind, name, sp.tree.search_plan(whole_moves=True)))
        ms = [[] for _ in players]
        for rep in range(args.reps + 3):
            for j in range(len(players)):
                i = (rep + j) % len(players)
                x = timed(torch, lambda: players[i].collect(MOVES))
                if rep >= 3:
                    ms[i].append(x)
        med = {}
        for (kind, name, _, _, _), xs, sp in zip(routes, ms, players):
            med[name] = statistics.median(xs)
            say('  %5d environments  %-9s %-24s ms per %d moves: %s   -> %.0f moves/s' % (n_envs, kind, name, MOVES, spread(xs),
                                                                                         1e3 * n_envs * MOVES / med[name]))
            sp.tree.check()
            sp.close()
        w, d = med['whole moves, auto shape'], med['device moves']
        say('  %5d environments  acrobot: device moves / whole moves (auto) = %.2f, device moves / whole moves (8 per wg) = %.2f'
            % (n_envs, d / w, d / med['whole moves, 8 per wg']))
        if args.parent:
            a, b, c = med['whole moves, parent (1)'], med['whole moves, parent (2)'], med['whole moves']
            say('  %5d environments  cartpole: two players of the parent commit differ by %.3f ms (medians %.3f and %.3f); this tree - parent (1) = '
                '%+.3f ms, this tree - parent (2) = %+.3f ms: %s the spread between the two parent players'
                % (n_envs, abs(a - b), a, b, c - a, c - b, 'OUTSIDE' if (c < min(a, b) or c > max(a, b)) else 'within'))
        else:
            say('  parent commit: not measured (no --parent)')


def part_iteration(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    on = dict(device_replay=True, fused_learner=True, env='acrobot')
    variants = [('acrobot (device moves)', dict(on)), ('acrobot --whole-moves', dict(on, whole_moves=True))]
    pipes = []
    for name, kw in variants:
        torch.manual_seed(args.seed)
        with as_here():
            pipes.append(here.MuZeroPipeline(n_envs=args.envs, n_sims=args.sims, batch_size=256, updates_per_iteration=40, seed=args.seed, **kw))
    assert pipes[0].selfplay.device_moves and pipes[1].selfplay.fused_moves

    def iteration(pipe):
        def body():
            pipe.collect_selfplay_data()
            pipe.reanalyse_targets()
            pipe.policy_update()
        return timed(torch, body)

    for pipe in pipes:   # as MuZeroPipeline.run: no update before 8 episodes are held
        while len(pipe.buffer) < 8:
            pipe.collect_selfplay_data()
    for _ in range(3):
        for pipe in pipes:
            iteration(pipe)
    ms = [[] for _ in pipes]
    for r in range(args.reps):
        for j in range(len(pipes)):
            i = (r + j) % len(pipes)
            ms[i].append(iteration(pipes[i]))
    say('iteration: %d environments, --device-replay --fused-learner, collect %d moves, 40 updates of batch 256; ms per iteration, %d repetitions '
        'after 3 (and after the collects that bring 8 episodes into each buffer), the two pipelines alternating' % (args.envs, pipes[0].moves_per_iteration, args.reps))
    for (name, _), xs in zip(variants, ms):
        say('  %-30s %s' % (name, spread(xs)))
    for pipe in pipes:
        pipe.selfplay.tree.check()
        pipe.selfplay.close()
        pipe.buffer.close()


def part_learning(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    say('learning (ONE observation, same seed; no claim): MuZeroPipeline(env=acrobot, whole_moves=True, 256 environments, device replay, fused '
        'learner).run(60)')
    torch.manual_seed(args.seed)
    with as_here():
        pipe = here.MuZeroPipeline(env='acrobot', whole_moves=True, device_replay=True, fused_learner=True, seed=args.seed)
    t0 = time.perf_counter()
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        pipe.run(60)
    torch.cuda.synchronize()
    rets = [line.split('episode_return:')[1].split(',')[0] for line in log.getvalue().splitlines() if 'episode_return:' in line]
    say('  acrobot --whole-moves  final episode_return %.1f, episode_len %.1f   (%.1f s for the 60 iterations, %d of them printed a line; '
        'episode_return every 10th line: %s)' % (pipe.episode_return, pipe.episode_len, time.perf_counter() - t0, len(rets), ' '.join(rets[9::10])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mz_whole_env', 'ab.txt'))
    ap.add_argument('--envs', type=int, default=8192)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--parent', default='', help='a checkout of the parent commit with its library built')
    ap.add_argument('--parts', default='moves,iteration,learning')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_mz_whole_env.py measures on the GPU: none here')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_mz_whole_env.py --parts %s: %s; HIP events on the launch stream' % (args.parts, torch.cuda.get_device_name(0)))
    parts = {'moves': part_moves, 'iteration': part_iteration, 'learning': part_learning}
    for part in args.parts.split(','):
        parts[part](args, torch, say)
    out.close()


if __name__ == '__main__':
    main()
