#!/usr/bin/env python3
"""What the fused MuZero learner costs next to the PyTorch route (rlzero_amd/muzero/learner.py, csrc/rz_mz_learn.hip), in one
process, HIP events on the launch stream, medians after warm-up.

  learn       8192 CartPole environments fill a MuZeroDeviceReplay; one mini-batch of 256 (K 5) drawn there; ``MuZeroAgent.learn``
              on the device route (PyTorch; its four ``.item()`` reads inside the event pair, as the trainer pays them) against
              ``learn_async`` of a fused agent holding the same weights, alternating; then ``grads`` alone (k_mzl_grad +
              k_mzl_reduce) and the update alone (k_mzl_adam = learn_async - grads, the difference of the two medians), and the
              host clock of one ``learn_async`` call (the launches are enqueued, nothing is waited for).
  refresh     what handing the updated weights to the search costs: ``MuZeroSelfPlay._refresh_model`` after a fused step
              (``load_model``'s host copy: once per iteration), host clock including a synchronise.
  iteration   the learner iteration of tools/train_muzero.py (MuZeroPipeline: collect 20 moves, 40 updates of batch 256) at 8192
              environments with --device-replay: --fused-learner | without | the parent commit (--parent DIR: a checkout of it
              with its library built; run TWICE, as two pipelines, for the spread between two runs of the same code).  Same
              seed, alternating iteration by iteration, each round starting one pipeline further on (profiles/ab_mz_reanalyse.py:
              the same method, its loader reused).
  learning    ONE observation per route, no claim: MuZeroPipeline(256 environments, device replay).run(60), same seed; the
              final episode_len of each.
  accuracy    the pairs (HIP error, torch-f32 error) against the float64 twin per shape of tests/test_mz_learner_gpu.py, for the raw
              gradient and the four losses -> --accuracy-out (profiles/mz_learner/accuracy.txt).

    python profiles/ab_mz_learner.py [--out profiles/mz_learner/ab.txt] [--reps 30] [--parent DIR] [--parts learn,refresh,iteration,learning,accuracy]

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
    """(torch-route agent, fused agent with the same weights, self-play object on the fused agent's net, device replay)."""
    from rlzero_amd.muzero import CartPoleBatch, MuZeroAgent, MuZeroDeviceReplay, MuZeroSelfPlay
    torch.manual_seed(args.seed)
    ref = MuZeroAgent(device='cuda:0')
    fused = MuZeroAgent(device='cuda:0', fused_learner=True, unroll_steps=5, max_batch=256)
    fused.net.load_state_dict(ref.net.state_dict())
    env = CartPoleBatch(args.envs, 'cuda:0', seed=args.seed)
    sp = MuZeroSelfPlay(fused.net, env, n_sims=args.sims, seed=args.seed)
    dev = MuZeroDeviceReplay(4, 2, 2000, int(env.max_episode_steps), unroll_steps=5, td_steps=10, device='cuda:0', seed=args.seed)
    sp.collect(48, replay=dev)
    return ref, fused, sp, dev


def part_learn(args, torch, say):
    ref, fused, sp, dev = filled(args, torch)
    batch = dev.sample(256)
    calls = (('MuZeroAgent.learn, PyTorch, device batch', lambda: ref.learn(batch)), ('learn_async, fused (3 launches)', lambda: fused.learn_async(batch)),
             ('grads alone, fused (2 launches)', lambda: fused.fused.grads(batch)))
    say('learn: batch 256, K 5, one mini-batch of the device replay (%d episodes held); ms per call, %d repetitions after 5, the calls alternating' % (
        len(dev), args.reps))
    ms = {name: [] for name, _ in calls}
    wall = {name: [] for name, _ in calls}
    for rep in range(args.reps + 5):
        for name, fn in calls:
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            t1 = time.perf_counter()
            b.record()
            torch.cuda.synchronize()
            if rep >= 5:
                ms[name].append(a.elapsed_time(b))
                wall[name].append(1e3 * (t1 - t0))
    for name, _ in calls:
        say('  %-44s events %s | host clock of the call, median %.3f' % (name, spread(ms[name]), statistics.median(wall[name])))
    med = {name: statistics.median(ms[name]) for name, _ in calls}
    torch_ms, fused_ms, grads_ms = (med[name] for name, _ in calls)
    say('  the update alone (k_mzl_adam) = learn_async - grads, medians: %.3f ms' % (fused_ms - grads_ms))
    say('  PyTorch / fused = %.1f x; %.0f against %.0f updates/s back to back' % (torch_ms / fused_ms, 1e3 / torch_ms, 1e3 / fused_ms))
    # back to back, as the trainer enqueues them: 40 updates, one read at the end
    runs = []
    for rep in range(args.reps // 3 + 2):
        def forty():
            last = None
            for _ in range(40):
                last = fused.learn_async(batch)
            last.tolist()
        x = timed(torch, forty)
        if rep >= 2:
            runs.append(x)
    say('  40 x learn_async + one read of the last result           events %s  (= %.3f ms per update)' % (spread(runs), statistics.median(runs) / 40))
    fused.check()
    sp.close()
    dev.close()


def part_refresh(args, torch, say):
    ref, fused, sp, dev = filled(args, torch)
    batch = dev.sample(256)
    xs = []
    for rep in range(args.reps + 3):
        fused.learn_async(batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sp._refresh_model()
        torch.cuda.synchronize()
        if rep >= 3:
            xs.append(1e3 * (time.perf_counter() - t0))
    say('refresh: MuZeroSelfPlay._refresh_model after a fused step (the version counters moved: load_model + load_representation, a host copy '
        'of the weights), host clock incl. synchronise, ms, %d repetitions after 3: %s' % (args.reps, spread(xs)))
    sp.close()
    dev.close()


def part_iteration(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    variants = [('--fused-learner', here, as_here, dict(fused_learner=True)), ('without (PyTorch learner)', here, as_here, {})]
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
    say('iteration: %d environments, --device-replay, collect %d moves, 40 updates of batch 256; ms per iteration, %d repetitions after 3, the '
        'pipelines alternating (each round starts one further on)' % (args.envs, pipes[0].moves_per_iteration, args.reps))
    med = {}
    for (name, _, _, _), xs in zip(variants, ms):
        med[name] = statistics.median(xs)
        say('  %-38s %s' % (name, spread(xs)))
    off, on = med['without (PyTorch learner)'], med['--fused-learner']
    if args.parent:
        a, b = med['parent commit (1)'], med['parent commit (2)']
        gap = abs(a - b)
        say('  two runs of the parent commit differ by %.3f ms (medians %.3f and %.3f); without - parent (1) = %+.3f ms, without - parent (2) = %+.3f ms'
            % (gap, a, b, off - a, off - b))
        say('  --fused-learner is %.3f ms (%.1f x) below the PyTorch learner of this tree and %.3f ms below the slower parent run: %s the spread '
            'between the two parent runs' % (off - on, off / on, max(a, b) - on, 'MORE than' if min(off, a, b) - on > gap else 'NOT more than'))
    else:
        say('  parent commit: not measured (no --parent); --fused-learner is %.3f ms (%.1f x) below the PyTorch learner' % (off - on, off / on))


def part_learning(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    say('learning (ONE observation per route, same seed; no claim): MuZeroPipeline(256 environments, device replay).run(60)')
    for name, kw in (('PyTorch learner', {}), ('fused learner', dict(fused_learner=True))):
        torch.manual_seed(args.seed)
        with as_here():
            pipe = here.MuZeroPipeline(device_replay=True, seed=args.seed, **kw)
        t0 = time.perf_counter()
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            final = pipe.run(60)
        torch.cuda.synchronize()
        lens = [line.split('episode_len:')[1].split(',')[0] for line in log.getvalue().splitlines() if 'episode_len:' in line]
        say('  %-18s final episode_len %.1f   (%.1f s for the 60 iterations; episode_len every 10th iteration: %s)' % (
            name, final, time.perf_counter() - t0, ' '.join(lens[9::10])))


def part_accuracy(args, torch, say):
    """The yardstick's two sides per shape (tests/test_mz_learner_gpu.py: test_grads_against_the_twin computes the same numbers)."""
    import numpy as np
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import test_mz_learner_gpu as tg
    os.makedirs(os.path.dirname(os.path.abspath(args.accuracy_out)), exist_ok=True)
    with open(args.accuracy_out, 'w') as out:
        def line(text):
            print(text, flush=True)
            out.write(text + '\n')
        line('# profiles/ab_mz_learner.py --parts accuracy: %s.  Largest absolute error against the float64 twin (MuZeroAgent.learn\'s' % torch.cuda.get_device_name(0))
        line('# expressions under torch autograd on float64 copies, CPU) of the fused learner (HIP) and of the torch float32 route on the GPU; the')
        line('# tests hold HIP <= 4 x torch-f32 per parameter tensor (gradient: the worst tensor is shown) and per loss.  Shape = (n, K, A, D).')
        line('%-18s %-9s %-12s %-12s %-12s %-12s' % ('shape', 'weights', 'grad HIP', 'grad f32', 'losses HIP', 'losses f32'))
        for shape in tg.GRAD_SHAPES:
            for weighted in (False, True):
                net, batch, weights, want, want_losses, ref32, ref32_losses = tg.reference(*shape, weighted)
                agent = tg.fused_agent(net, shape[1], shape[0])
                grad, out4 = agent.fused.grads(*tg.on_device(batch, weights))
                line('%-18s %-9s %-12.3e %-12.3e %-12.3e %-12.3e' % (shape, 'yes' if weighted else 'no', np.abs(grad.cpu().numpy() - want).max(),
                                                                 np.abs(ref32 - want).max(), np.abs(out4.cpu().numpy() - want_losses).max(),
                                                                 np.abs(ref32_losses - want_losses).max()))
                agent.fused.close()
    say('accuracy: written to %s' % os.path.relpath(args.accuracy_out, REPO))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mz_learner', 'ab.txt'))
    ap.add_argument('--accuracy-out', default=os.path.join(REPO, 'profiles', 'mz_learner', 'accuracy.txt'))
    ap.add_argument('--envs', type=int, default=8192)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--parent', default='', help='a checkout of the parent commit with its library built')
    ap.add_argument('--parts', default='learn,refresh,iteration,learning,accuracy')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_mz_learner.py measures on the GPU: none here')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_mz_learner.py --parts %s: %s; HIP events on the launch stream unless a line says otherwise' % (args.parts, torch.cuda.get_device_name(0)))
    parts = {'learn': part_learn, 'refresh': part_refresh, 'iteration': part_iteration, 'learning': part_learning, 'accuracy': part_accuracy}
    for part in args.parts.split(','):
        parts[part](args, torch, say)
    out.close()


if __name__ == '__main__':
    main()
