#!/usr/bin/env python3
"""What MuZero's device moves cost next to whole moves and the host loop (MuZeroSelfPlay(device_moves=...), csrc/rz_muzero.hip:
k_mz_env_move, k_mz_root_noise, k_mz_env_step), in one process, HIP events on the launch stream, medians after warm-up.

  moves       moves/s of self-play at 50 simulations, ``collect(16)`` between two events (what the stream spends, the host's waits
              included, as the trainer pays them): CartPole on whole moves | device moves | the host loop, Acrobot on device moves
              | the host loop, at 256 and at 8192 environments; the routes of one size alternate.
  iteration   the iteration of tools/train_muzero.py (MuZeroPipeline: collect 20 moves, 40 updates of batch 256) at 8192
              environments with --device-replay --fused-learner for both environments, and for the CartPole default the parent
              commit (--parent DIR: a checkout of it with its library built) run TWICE, as two pipelines, for the spread between
              two runs of the same code (profiles/ab_mz_reanalyse.py: the same method, its loader reused).
  learning    ONE observation, no claim: MuZeroPipeline(env='acrobot', 256 environments, device replay, fused learner).run(60),
              the final episode_return (and the one of every 10th iteration).

    python profiles/ab_mz_env.py [--out profiles/mz_env/ab.txt] [--reps 30] [--parent DIR] [--parts moves,iteration,learning]

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
from ab_mz_reanalyse import load_trainer, spread  # noqa: E402

MOVES = 16


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def part_moves(args, torch, say):
    from rlzero_amd.muzero import AcrobotBatch, CartPoleBatch, MuZeroNet, MuZeroSelfPlay
    say('moves: %d simulations, collect(%d) between two events, %d repetitions after 3, the routes of one size alternating; moves/s = '
        'environments x %d / the median' % (args.sims, MOVES, args.reps, MOVES))
    routes = (('cartpole', 'whole moves', dict()), ('cartpole', 'device moves', dict(fused_moves=False, device_moves=True)),
              ('cartpole', 'host loop', dict(fused_moves=False)), ('acrobot', 'device moves', dict()), ('acrobot', 'host loop', dict(device_moves=False)))
    for n_envs in (256, args.envs):
        players = []
        for kind, name, kw in routes:
            torch.manual_seed(args.seed)
            env = CartPoleBatch(n_envs, 'cuda:0', seed=args.seed) if kind == 'cartpole' else AcrobotBatch(n_envs, 'cuda:0', seed=args.seed)
            net = MuZeroNet(env.obs_dim, env.n_actions).to('cuda:0').eval()
            sp = MuZeroSelfPlay(net, env, n_sims=args.sims, seed=args.seed, moves_per_launch=MOVES, **kw)
            assert (sp.fused_moves, sp.device_moves) == (name == 'whole moves', name == 'device moves')
            players.append(sp)
        ms = [[] for _ in players]
        for rep in range(args.reps + 3):
            for j in range(len(players)):
                i = (rep + j) % len(players)
                x = timed(torch, lambda: players[i].collect(MOVES))
                if rep >= 3:
                    ms[i].append(x)
        for (kind, name, _), xs, sp in zip(routes, ms, players):
            say('  %5d environments  %-9s %-13s ms per %d moves: %s   -> %.0f moves/s' % (n_envs, kind, name, MOVES, spread(xs),
                                                                                        1e3 * n_envs * MOVES / statistics.median(xs)))
            sp.close()


def part_iteration(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    on = dict(device_replay=True, fused_learner=True)
    variants = [('cartpole (whole moves)', here, as_here, dict(on)), ('acrobot (device moves)', here, as_here, dict(on, env='acrobot'))]
    if args.parent:   # (this tree's CartPole pipeline runs between the two of the parent: none of the three follows Acrobot's)
        parent, as_parent = load_trainer(os.path.abspath(args.parent), 'rlzero_amd_parent')
        variants = ([('cartpole, parent commit (1)', parent, as_parent, dict(on)), variants[0],
                     ('cartpole, parent commit (2)', parent, as_parent, dict(on)), variants[1]])
    pipes = []
    for name, mod, ctx, kw in variants:
        torch.manual_seed(args.seed)
        with ctx():
            pipes.append(mod.MuZeroPipeline(n_envs=args.envs, n_sims=args.sims, batch_size=256, updates_per_iteration=40, seed=args.seed, **kw))

    def iteration(pipe):
        def body():
            pipe.collect_selfplay_data()
            pipe.reanalyse_targets()
            pipe.policy_update()
        return timed(torch, body)

    for pipe in pipes:   # as MuZeroPipeline.run: no update before 8 episodes are held (an Acrobot episode lasts up to 500 moves: 25 collects)
        while len(pipe.buffer) < 8:
            pipe.collect_selfplay_data()
    for _ in range(3):
        for pipe in pipes:
            iteration(pipe)
    ms = [[] for _ in pipes]
    for r in range(args.reps):
        for j in range(len(pipes)):   # the round starts one pipeline further on every time: no variant always follows the same one
            i = (r + j) % len(pipes)
            ms[i].append(iteration(pipes[i]))
    say('iteration: %d environments, --device-replay --fused-learner, collect %d moves, 40 updates of batch 256; ms per iteration, %d repetitions '
        'after 3 (and after the collects that bring 8 episodes into each buffer), the pipelines alternating (each round starts one further on)'
        % (args.envs, pipes[0].moves_per_iteration, args.reps))
    med = {}
    for (name, _, _, _), xs in zip(variants, ms):
        med[name] = statistics.median(xs)
        say('  %-30s %s' % (name, spread(xs)))
    if args.parent:
        a, b, c = med['cartpole, parent commit (1)'], med['cartpole, parent commit (2)'], med['cartpole (whole moves)']
        say('  two runs of the parent commit differ by %.3f ms (medians %.3f and %.3f); this tree - parent (1) = %+.3f ms, this tree - parent (2) = '
            '%+.3f ms: %s the spread between the two parent runs' % (abs(a - b), a, b, c - a, c - b,
                                                                    'MORE than' if min(abs(c - a), abs(c - b)) > abs(a - b) else 'NOT more than'))
    else:
        say('  parent commit: not measured (no --parent)')


def part_learning(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    say('learning (ONE observation, same seed; no claim): MuZeroPipeline(env=acrobot, 256 environments, device replay, fused learner).run(60)')
    torch.manual_seed(args.seed)
    with as_here():
        pipe = here.MuZeroPipeline(env='acrobot', device_replay=True, fused_learner=True, seed=args.seed)
    t0 = time.perf_counter()
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        pipe.run(60)
    torch.cuda.synchronize()
    rets = [line.split('episode_return:')[1].split(',')[0] for line in log.getvalue().splitlines() if 'episode_return:' in line]
    say('  acrobot            final episode_return %.1f, episode_len %.1f   (%.1f s for the 60 iterations, %d of them printed a line; episode_return '
        'every 10th line: %s)' % (pipe.episode_return, pipe.episode_len, time.perf_counter() - t0, len(rets), ' '.join(rets[9::10])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mz_env', 'ab.txt'))
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
        raise SystemExit('profiles/ab_mz_env.py measures on the GPU: none here')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_mz_env.py --parts %s: %s; HIP events on the launch stream' % (args.parts, torch.cuda.get_device_name(0)))
    parts = {'moves': part_moves, 'iteration': part_iteration, 'learning': part_learning}
    for part in args.parts.split(','):
        parts[part](args, torch, say)
    out.close()


if __name__ == '__main__':
    main()
