#!/usr/bin/env python3
"""What the fused MuZero learner costs with categorical heads (k_mzl_grad<R, true>), and that the scalar route costs what it did: one
process, HIP events on the launch stream, the routes alternating, medians after warm-up (the method and helpers of
profiles/ab_mz_learner.py).

  learn       a net with support 20 (41 bins a head): one mini-batch of 256 (K 5) of a device replay filled by 8192 Acrobot
              environments; ``MuZeroAgent.learn`` on the PyTorch route (its four ``.item()`` reads inside the event pair) against
              ``learn_async`` of a fused agent holding the same weights.
  iteration   tools/train_muzero.py's iteration (--env acrobot --device-replay --value-transform --support 20, 8192 environments, 40 updates of
              batch 256) with and without --fused-learner, same seed, alternating.
  scalar      a scalar net: ``learn_async`` of this tree's fused route against two agents of the parent commit (--parent DIR: a
              checkout of it with its library built, loaded under another package name) in the same rounds; whether this tree lies
              inside the two parent players' spread.
  accuracy    (HIP error, torch-f32 error) against the float64 twin per shape of tests/test_mz_learner_support_gpu.py -> --accuracy-out.

    python profiles/ab_mz_learner_support.py [--out profiles/mz_learner_support/ab.txt] [--reps 30] [--parent DIR] [--parts learn,iteration,scalar,accuracy]

No figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ab_mz_learner import timed  # noqa: E402
from ab_mz_reanalyse import load_trainer, spread  # noqa: E402

S = 20


def alternate(torch, calls, reps, warm=5):
    """ms per call of each (name, fn), the calls alternating, ``reps`` repetitions after ``warm``."""
    ms = {name: [] for name, _ in calls}
    for rep in range(reps + warm):
        for name, fn in calls:
            torch.cuda.synchronize()
            x = timed(torch, fn)
            if rep >= warm:
                ms[name].append(x)
    return ms


def part_learn(args, torch, say):
    from rlzero_amd.muzero import AcrobotBatch, MuZeroAgent, MuZeroDeviceReplay, MuZeroSelfPlay
    torch.manual_seed(args.seed)
    shape = dict(obs_dim=AcrobotBatch.obs_dim, n_actions=AcrobotBatch.n_actions, value_transform=True, support=S, device='cuda:0')
    ref, fused = MuZeroAgent(**shape), MuZeroAgent(fused_learner=True, unroll_steps=5, max_batch=256, **shape)
    fused.net.load_state_dict(ref.net.state_dict())
    env = AcrobotBatch(args.envs, 'cuda:0', seed=args.seed, max_episode_steps=24)
    sp = MuZeroSelfPlay(fused.net, env, n_sims=args.sims, seed=args.seed)
    dev = MuZeroDeviceReplay(env.obs_dim, env.n_actions, 2000, 24, unroll_steps=5, td_steps=10, device='cuda:0', seed=args.seed, value_transform=True)
    sp.collect(30, replay=dev)
    batch = dev.sample(256)
    calls = (('MuZeroAgent.learn, PyTorch, support %d' % S, lambda: ref.learn(batch)), ('learn_async, fused, support %d (3 launches)' % S, lambda: fused.learn_async(batch)),
             ('grads alone, fused, support %d (2 launches)' % S, lambda: fused.fused.grads(batch)))
    ms = alternate(torch, calls, args.reps)
    say('learn: support %d, batch 256, K 5, one mini-batch of the device replay (%d episodes held); ms per call, %d repetitions after 5, alternating' % (S, len(dev), args.reps))
    for name, _ in calls:
        say('  %-48s %s' % (name, spread(ms[name])))
    a, b = (statistics.median(ms[name]) for name, _ in calls[:2])
    say('  PyTorch / fused = %.1f x' % (a / b))
    fused.check()
    sp.close()
    dev.close()


def part_iteration(args, torch, say):
    here, as_here = load_trainer(REPO, 'rlzero_amd')
    variants = [('--fused-learner', dict(fused_learner=True)), ('without (PyTorch learner)', {})]
    pipes = []
    for name, kw in variants:
        torch.manual_seed(args.seed)
        with as_here():
            pipes.append(here.MuZeroPipeline(env='acrobot', n_envs=args.envs, n_sims=args.sims, batch_size=256, updates_per_iteration=40, device_replay=True,
                                             value_transform=True, support=S, max_episode_steps=24, seed=args.seed, **kw))

    def iteration(pipe):
        def body():
            pipe.collect_selfplay_data()
            pipe.reanalyse_targets()
            pipe.policy_update()
        return timed(torch, body)
    for pipe in pipes:   # (an episode of 24 steps ends in the second collection: no update meets an empty buffer)
        pipe.collect_selfplay_data(), pipe.collect_selfplay_data()
    ms = alternate(torch, [(name, lambda p=pipe: iteration(p)) for (name, _), pipe in zip(variants, pipes)], args.reps, warm=3)
    say('iteration: --env acrobot --max-episode-steps 24 --value-transform --support %d --device-replay, %d environments, collect %d moves, 40 updates of '
        'batch 256; ms per iteration (events around the whole iteration), %d repetitions after 3, alternating' % (S, args.envs, pipes[0].moves_per_iteration, args.reps))
    for name, _ in variants:
        say('  %-28s %s' % (name, spread(ms[name])))
    on, off = (statistics.median(ms[name]) for name, _ in variants)
    say('  --fused-learner is %.3f ms (%.1f x) below the PyTorch learner' % (off - on, off / on))


def part_scalar(args, torch, say):
    import importlib
    from rlzero_amd.muzero import MuZeroAgent
    players = [('this tree', MuZeroAgent)]
    if args.parent:
        load_trainer(os.path.abspath(args.parent), 'rlzero_amd_parent')   # (the parent's package under another name, its own library beside it)
        parent = importlib.import_module('rlzero_amd_parent.muzero').MuZeroAgent
        players += [('parent commit (1)', parent), ('parent commit (2)', parent)]
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    from test_mz_learner_host import make_batch
    batch, _ = make_batch(256, 5, 2, 4, seed=args.seed)
    batch = tuple(torch.from_numpy(a).cuda() for a in batch)
    agents = [(name, cls(device='cuda:0', fused_learner=True, unroll_steps=5, max_batch=256)) for name, cls in players]
    ms = alternate(torch, [(name, lambda a=agent: a.learn_async(batch)) for name, agent in agents], args.reps)
    say('scalar: scalar heads, batch 256, K 5, learn_async (3 launches); ms per call, %d repetitions after 5, the players alternating' % args.reps)
    for name, _ in agents:
        say('  %-20s %s' % (name, spread(ms[name])))
    if args.parent:
        med = [statistics.median(ms[name]) for name, _ in agents]
        lo, hi = min(med[1:]), max(med[1:])
        say('  this tree %.4f ms; the two parent players %.4f and %.4f ms: %s their spread (%+.4f ms from the nearer one)' % (
            med[0], med[1], med[2], 'INSIDE' if lo <= med[0] <= hi else 'OUTSIDE', med[0] - (lo if med[0] < lo else hi if med[0] > hi else med[0])))
    else:
        say('  parent commit: not measured (no --parent)')


def part_accuracy(args, torch, say):
    import numpy as np
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import test_mz_learner_support_gpu as tg
    with open(args.accuracy_out, 'w') as out:
        def line(text):
            print(text, flush=True)
            out.write(text + '\n')
        line('# profiles/ab_mz_learner_support.py --parts accuracy: %s.  Largest absolute error against the float64 twin (agent.support_losses under' % torch.cuda.get_device_name(0))
        line('# torch autograd on float64 copies, CPU) of the fused learner (HIP) and of the torch float32 route on the GPU; the tests hold HIP <= 4 x')
        line('# torch-f32 per parameter tensor (gradient: the worst tensor is shown) and per loss.  Shape = (n, K, A, D, S).')
        line('%-22s %-9s %-12s %-12s %-12s %-12s' % ('shape', 'weights', 'grad HIP', 'grad f32', 'losses HIP', 'losses f32'))
        for shape in tg.GRAD_SHAPES:
            for weighted in (False, True):
                net, batch, weights, want, want_losses, ref32, ref32_losses = tg.reference(*shape, weighted)
                agent = tg.agent_of(net, shape[1], shape[0])
                grad, out4 = agent.fused.grads(*tg.on_device(batch, weights))
                line('%-22s %-9s %-12.3e %-12.3e %-12.3e %-12.3e' % (shape, 'yes' if weighted else 'no', np.abs(grad.cpu().numpy() - want).max(), np.abs(ref32 - want).max(),
                                                                 np.abs(out4.cpu().numpy() - want_losses).max(), np.abs(ref32_losses - want_losses).max()))
                agent.fused.close()
    say('accuracy: written to %s' % os.path.relpath(args.accuracy_out, REPO))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mz_learner_support', 'ab.txt'))
    ap.add_argument('--accuracy-out', default=os.path.join(REPO, 'profiles', 'mz_learner_support', 'accuracy.txt'))
    ap.add_argument('--envs', type=int, default=8192)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--parent', default='', help='a checkout of the parent commit with its library built')
    ap.add_argument('--parts', default='learn,iteration,scalar,accuracy')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_mz_learner_support.py measures on the GPU: none here')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        def say(line):
            print(line, flush=True)
            out.write(line + '\n')
            out.flush()
        say('# profiles/ab_mz_learner_support.py --parts %s: %s; HIP events on the launch stream' % (args.parts, torch.cuda.get_device_name(0)))
        for part in args.parts.split(','):
            {'learn': part_learn, 'iteration': part_iteration, 'scalar': part_scalar, 'accuracy': part_accuracy}[part](args, torch, say)


if __name__ == '__main__':
    main()
