#!/usr/bin/env python3
"""What a MuZero update costs on the two replay routes: 8192 CartPole environments, batch 256, K = 5, td_steps = 10, a random-init
net.  One stretch of whole-move self-play fills BOTH buffers with the same episodes (capacity 2000 each: the host ReplayBuffer by
``add`` of the returned EpisodeSeq, the MuZeroDeviceReplay by the hand-over from the launches' device arena), then the routes
alternate in one process, --reps repetitions after warm-up; median, min and max.

  host route    ReplayBuffer.sample (CPython loops over K + 1 unroll steps and td_steps rewards per entry) and MuZeroAgent.learn,
                which pushes the six numpy arrays to the GPU
  device route  MuZeroDeviceReplay.sample (one launch into torch tensors) and MuZeroAgent.learn on the device tensors

Measured with the host clock, every figure ending in a device synchronise: ms per ``sample``, ms per ``learn`` INCLUDING the
formation of its input, and the updates per second that follow from the latter.  The two learners start from equal weights and
see different batches (each route draws from its own stream).  Also: ms to fill either buffer from the stretch's episodes.

    python profiles/ab_mz_replay.py [--out profiles/mz_replay/ab.txt] [--reps 30]

No figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(xs):
    return 'median %.3f  min %.3f  max %.3f' % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mz_replay', 'ab.txt'))
    ap.add_argument('--envs', type=int, default=8192)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--moves', type=int, default=48)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    from rlzero_amd.muzero import CartPoleBatch, MuZeroAgent, MuZeroDeviceReplay, MuZeroSelfPlay, ReplayBuffer
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_mz_replay.py measures on the GPU: none here')
    K, td, capacity = 5, 10, 2000
    torch.manual_seed(args.seed)
    host_agent = MuZeroAgent(device='cuda:0')
    torch.manual_seed(args.seed)
    dev_agent = MuZeroAgent(device='cuda:0')
    env = CartPoleBatch(args.envs, 'cuda:0', seed=args.seed)
    sp = MuZeroSelfPlay(host_agent.net, env, n_sims=args.sims, seed=args.seed)
    dev = MuZeroDeviceReplay(4, 2, capacity, int(env.max_episode_steps), unroll_steps=K, td_steps=td, device='cuda:0', seed=args.seed)
    host = ReplayBuffer(capacity=capacity, unroll_steps=K, td_steps=td, seed=args.seed)
    sp.collect(16)   # warm-up of the launch path
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    episodes = sp.collect(args.moves)
    torch.cuda.synchronize()
    plain_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    more = sp.collect(args.moves, replay=dev)
    torch.cuda.synchronize()
    handed_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    for ep in more:
        host.add(ep)
    host_fill_ms = 1e3 * (time.perf_counter() - t0)
    sp.close()
    assert len(dev) == len(host) and list(dev.lengths()) == [len(ep) for ep in host.episodes]
    lines = ['# profiles/ab_mz_replay.py: %d environments, %d simulations, batch %d, K = %d, td_steps = %d, %d repetitions, %s' % (
        args.envs, args.sims, args.batch, K, td, args.reps, torch.cuda.get_device_name(0)),
        '# %d episodes ended in the stretch of %d moves handed over (mean length %.1f); both buffers hold the last %d' % (
            len(more), args.moves, float(more.lengths().mean()), len(host)),
        'collect(%d moves), ms: without a replay buffer %.1f (%d episodes) | with replay=MuZeroDeviceReplay %.1f (%d episodes)' % (
            args.moves, plain_ms, len(episodes), handed_ms, len(more)),
        'host buffer: add of the %d returned episodes, ms: %.1f' % (len(more), host_fill_ms)]

    def host_sample():
        out = host.sample(args.batch, 2)
        torch.cuda.synchronize()
        return out

    def dev_sample():
        out = dev.sample(args.batch)
        torch.cuda.synchronize()
        return out

    def host_learn():
        host_agent.learn(host.sample(args.batch, 2))
        torch.cuda.synchronize()

    def dev_learn():
        dev_agent.learn(dev.sample(args.batch))
        torch.cuda.synchronize()

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(3):   # warm-up of both routes
        host_sample(), dev_sample(), host_learn(), dev_learn()
    hs, ds, hl, dl = [], [], [], []
    for _ in range(args.reps):
        hs.append(clock(host_sample))
        ds.append(clock(dev_sample))
        hl.append(clock(host_learn))
        dl.append(clock(dev_learn))
    lines.append('sample, ms:                       host route %s | device route %s' % (spread(hs), spread(ds)))
    lines.append('learn incl. input formation, ms:  host route %s | device route %s' % (spread(hl), spread(dl)))
    lines.append('updates/s (1000 / median learn):  host route %.1f | device route %.1f' % (1e3 / statistics.median(hl), 1e3 / statistics.median(dl)))
    dev.close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
