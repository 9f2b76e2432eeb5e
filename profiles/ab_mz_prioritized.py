#!/usr/bin/env python3
"""What MuZero prioritized replay costs (rlzero_amd/muzero/replay.py: sample_prioritized), in one process, HIP events on the launch
stream, medians after warm-up.

  sample      8192 CartPole environments fill a MuZeroDeviceReplay of 2000 episodes with priorities on; with the prefixes clean,
              ``sample(256)`` (one launch) next to ``sample_prioritized(256)`` (draw launch, gather launch, the importance
              weights in torch), alternating; and ``refresh_priorities()`` with nothing to do (every workgroup of k_mzr_prio
              returns at its mark, then k_mzr_scan).
  refresh     the refresh alone, an event pair around ``refresh_priorities()``: after one iteration's hand-over (collect 20 moves
              into the buffer: the slots written are marked), and after a Reanalyse of 2048 positions (the slots of the steps
              written back are marked).
  iteration   the learner iteration of tools/train_muzero.py (MuZeroPipeline: collect 20 moves, [refresh], 40 updates of batch 256)
              at 8192 environments: off | --prioritized-replay | --prioritized-replay --reanalyse 2048 | the parent commit
              (--parent DIR: a checkout of it with its library built; run TWICE, as two pipelines, so that the spread between
              two runs of the same code stands next to the difference off - parent).  Same seed, alternating iteration by
              iteration, each round starting one pipeline further on (profiles/ab_mz_reanalyse.py: the same method, its loader
              reused).
  learning    ONE observation per variant, no claim: MuZeroPipeline(256 environments, device replay).run(60) with and without
              prioritized replay, same seed; the final episode_len of each.

    python profiles/ab_mz_prioritized.py [--out profiles/mz_prioritized/ab.txt] [--reps 30] [--parent DIR] [--parts sample,refresh,iteration,learning]

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


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def filled(args, torch):
    from rlzero_amd.muzero import CartPoleBatch, MuZeroAgent, MuZeroDeviceReplay, MuZeroSelfPlay
    torch.manual_seed(args.seed)
    agent = MuZeroAgent(device='cuda:0')
    env = CartPoleBatch(args.envs, 'cuda:0', seed=args.seed)
    sp = MuZeroSelfPlay(agent.net, env, n_sims=args.sims, seed=args.seed)
    dev = MuZeroDeviceReplay(4, 2, 2000, int(env.max_episode_steps), unroll_steps=5, td_steps=10, device='cuda:0', seed=args.seed,
                             prioritized=True)
    sp.collect(48, replay=dev)
    return agent, sp, dev


def part_sample(args, torch, say):
    agent, sp, dev = filled(args, torch)
    sp.close()
    dev.refresh_priorities()
    torch.cuda.synchronize()
    calls = (('sample(256)', lambda: dev.sample(256)), ('sample_prioritized(256)', lambda: dev.sample_prioritized(256)),
             ('prioritized_draws(256)', lambda: dev.prioritized_draws(256)), ('refresh_priorities(), all clean', dev.refresh_priorities))
    say('sample: %d episodes held (%d steps, capacity 2000 x %d), K 5, td 10, batch 256, the prefixes clean; ms per call, %d repetitions after 5, '
        'the calls alternating' % (len(dev), int(dev.lengths().sum()), dev.max_episode_steps, args.reps))
    ms = {name: [] for name, _ in calls}
    wall = {name: [] for name, _ in calls}
    for rep in range(args.reps + 5):
        for name, fn in calls:
            t0 = time.perf_counter()
            x = timed(torch, fn)
            if rep >= 5:
                ms[name].append(x)
                wall[name].append(1e3 * (time.perf_counter() - t0))
    for name, _ in calls:
        say('  %-32s events %s | host clock incl. synchronise median %.3f' % (name, spread(ms[name]), statistics.median(wall[name])))
    dev.close()


def part_refresh(args, torch, say):
    from rlzero_amd.muzero import MuZeroReanalyser
    agent, sp, dev = filled(args, torch)
    rean = MuZeroReanalyser(agent.net, dev, n_sims=args.sims, batch=2048, seed=args.seed)
    dev.refresh_priorities()
    after_ingest, after_reanalyse, handed = [], [], []
    for rep in range(args.reps + 3):
        handed.append(len(sp.collect(20, replay=dev)))
        a = timed(torch, dev.refresh_priorities)
        rean.reanalyse_sample(2048)
        b = timed(torch, dev.refresh_priorities)
        if rep >= 3:
            after_ingest.append(a), after_reanalyse.append(b)
    say('refresh: %d episodes held (%d steps); ms per refresh_priorities() (k_mzr_prio + k_mzr_scan), %d repetitions after 3' % (
        len(dev), int(dev.lengths().sum()), args.reps))
    say('  after one iteration\'s hand-over (20 moves, median %d episodes stored)   %s' % (statistics.median(handed[3:]), spread(after_ingest)))
    say('  after a Reanalyse of 2048 positions                                    %s' % spread(after_reanalyse))
    rean.close()
    sp.close()
    dev.close()


def part_iteration(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    variants = [('off', here, as_here, {}), ('--prioritized-replay', here, as_here, dict(prioritized_replay=True)),
                ('--prioritized-replay --reanalyse 2048', here, as_here, dict(prioritized_replay=True, reanalyse=2048))]
    if args.parent:
        parent, as_parent = load_trainer(os.path.abspath(args.parent), 'rlzero_amd_parent')
        variants += [('parent commit (1)', parent, as_parent, {}), ('parent commit (2)', parent, as_parent, {})]
    pipes = []
    for name, mod, ctx, kw in variants:
        torch.manual_seed(args.seed)
        with ctx():
            pipes.append(mod.MuZeroPipeline(n_envs=args.envs, n_sims=args.sims, batch_size=256, updates_per_iteration=40, device_replay=True,
                                            seed=args.seed, **kw))

    def iteration(pipe):
        def body():
            pipe.collect_selfplay_data()
            pipe.reanalyse_targets()
            pipe.policy_update()
        return timed(torch, body)

    for _ in range(3):
        for pipe in pipes:
            iteration(pipe)
    ms = [[] for _ in pipes]
    for r in range(args.reps):
        for j in range(len(pipes)):   # the round starts one pipeline further on every time: no variant always follows the same one
            i = (r + j) % len(pipes)
            ms[i].append(iteration(pipes[i]))
    say('iteration: %d environments, collect %d moves, 40 updates of batch 256; ms per iteration, %d repetitions after 3, the pipelines '
        'alternating (each round starts one further on)' % (args.envs, pipes[0].moves_per_iteration, args.reps))
    med = {}
    for (name, _, _, _), xs in zip(variants, ms):
        med[name] = statistics.median(xs)
        say('  %-38s %s' % (name, spread(xs)))
    if args.parent:
        a, b = med['parent commit (1)'], med['parent commit (2)']
        say('  two runs of the parent commit differ by %.3f ms (medians %.3f and %.3f); off - parent (1) = %+.3f ms, off - parent (2) = %+.3f ms: '
            'off lies %s the parent runs\' spread' % (abs(a - b), a, b, med['off'] - a, med['off'] - b,
                                                     'inside' if min(a, b) - abs(a - b) <= med['off'] <= max(a, b) + abs(a - b) else 'OUTSIDE'))
        say('  the least disturbed iteration of each: off %.3f, parent (1) %.3f, parent (2) %.3f' % tuple(min(ms[i]) for i in (0, len(pipes) - 2, len(pipes) - 1)))
    else:
        say('  parent commit: not measured (no --parent)')


def part_learning(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    say('learning (ONE observation per variant, same seed; no claim): MuZeroPipeline(256 environments, device replay).run(60)')
    for name, kw in (('without', {}), ('prioritized replay, beta 1', dict(prioritized_replay=True))):
        torch.manual_seed(args.seed)
        with as_here():
            pipe = here.MuZeroPipeline(device_replay=True, seed=args.seed, **kw)
        t0 = time.perf_counter()
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            final = pipe.run(60)
        torch.cuda.synchronize()
        lens = [line.split('episode_len:')[1].split(',')[0] for line in log.getvalue().splitlines() if 'episode_len:' in line]
        say('  %-28s final episode_len %.1f   (%.1f s for the 60 iterations; episode_len every 10th iteration: %s)' % (
            name, final, time.perf_counter() - t0, ' '.join(lens[9::10])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mz_prioritized', 'ab.txt'))
    ap.add_argument('--envs', type=int, default=8192)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--parent', default='', help='a checkout of the parent commit with its library built')
    ap.add_argument('--parts', default='sample,refresh,iteration,learning')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_mz_prioritized.py measures on the GPU: none here')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_mz_prioritized.py --parts %s: %s; HIP events on the launch stream unless a line says otherwise' % (
        args.parts, torch.cuda.get_device_name(0)))
    for part in args.parts.split(','):
        {'sample': part_sample, 'refresh': part_refresh, 'iteration': part_iteration, 'learning': part_learning}[part](args, torch, say)
    out.close()


if __name__ == '__main__':
    main()
