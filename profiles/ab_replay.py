#!/usr/bin/env python3
"""What a mini-batch costs on the two replay routes, 15 x 15: a buffer of 512 synthetic games (seeded random legal move lists of about
100 plies with Dirichlet pi rows -- no search), batch sizes 32, 512 and 4096.

  host route    random.sample on the trainer's ReplayBuffer + stacking + AlphaZeroAgent._tensor for the three columns, ending in a
                device synchronise (host clock)
  device route  DeviceReplay.sample: one launch into fresh torch tensors (device events around the call; the host clock of the call
                ending in a synchronise beside it)

The routes alternate in one process, --reps repetitions of each shape after warm-up; median, min and max.  Also: ms per 512-game round
of ingest on either route (extend_samples(training_samples()) / add), and the gather kernel's achieved bytes/s -- the bytes the shapes
imply (below) over the device-event time of back-to-back launches into the same tensors -- next to the HBM peak.

    python profiles/ab_replay.py [--out profiles/replay/ab.txt] [--reps 50]

No figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import importlib.util
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12       # bytes/s, specification
HBM_MEASURED = 6.29e12  # bytes/s, a float4 copy on this chip


def entry_bytes(A):
    """Bytes one gathered entry moves: the position's record (two bitboards, meta, the pi row), the two table rows, and the rows
    written (four planes, pi, z)."""
    read = 2 * 4 * 8 + 4 + 4 * A + 2 * 2 * A
    written = 4 * 4 * A + 4 * A + 4
    return read + written


def synthetic_games(board, n_games, seed):
    import numpy as np
    from rlzero_amd.selfplay import Trajectory
    rs, A = np.random.RandomState(seed), board * board
    games = []
    for g in range(n_games):
        plies = int(rs.randint(80, 121))
        moves = rs.permutation(A)[:plies]
        pis = rs.dirichlet(np.full(A, 0.3), size=plies)
        games.append(Trajectory(g, board, 5, moves.tolist(), pis, int(rs.randint(-1, 2))))
    return games


def spread(xs):
    return 'median %.3f  min %.3f  max %.3f' % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'replay', 'ab.txt'))
    ap.add_argument('--board', type=int, default=15)
    ap.add_argument('--games', type=int, default=512)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--batches', type=int, nargs='+', default=[32, 512, 4096])
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    from rlzero_amd.games.gomoku.alphazero_agent import AlphaZeroAgent
    from rlzero_amd.replay import DeviceReplay
    spec = importlib.util.spec_from_file_location('train_alphazero', os.path.join(REPO, 'tools', 'train_alphazero.py'))
    trainer = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(trainer)
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_replay.py measures on the GPU: none here')
    random.seed(args.seed)
    A = args.board ** 2
    games = synthetic_games(args.board, args.games, args.seed)
    positions = sum(len(t.moves) for t in games)
    agent = AlphaZeroAgent(args.board, device='cuda:0')
    lines = ['# profiles/ab_replay.py: %d x %d, %d synthetic games, %d positions (%d entries), %d repetitions per shape, %s' % (
        args.board, args.board, args.games, positions, 8 * positions, args.reps, torch.cuda.get_device_name(0))]

    lines.append('# the store: %.1f MB of records (it fits the 256 MiB Infinity Cache: the rate below is no pure HBM rate)' % (
        positions * (2 * 4 * 8 + 4 + 4 * A) / 1e6))
    # ingest: a round of games into either buffer
    host_ms, dev_ms = [], []
    for _ in range(3):
        buf = trainer.ReplayBuffer(8 * positions, args.board)
        t0 = time.perf_counter()
        for t in games:
            buf.extend_samples(t.training_samples())
        host_ms.append(1e3 * (time.perf_counter() - t0))
        dr = DeviceReplay(args.board, positions, device='cuda:0', seed=args.seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dr.add(games)
        torch.cuda.synchronize()
        dev_ms.append(1e3 * (time.perf_counter() - t0))
        if _ < 2:
            dr.close()
    lines.append('ingest, ms per %d-game round (3 runs):  host extend_samples(training_samples()) %s | device add %s' % (
        args.games, spread(host_ms), spread(dev_ms)))
    assert len(dr) == len(buf)

    def host_batch(n):
        batch = random.sample(buf, n)
        cols = [list(col) for col in zip(*batch)]
        out = [agent._tensor(col) for col in cols]
        torch.cuda.synchronize()
        return out

    for n in args.batches:
        for _ in range(3):   # warm-up of both routes at this shape
            host_batch(n)
            dr.sample(n)
        torch.cuda.synchronize()
        host, dev_ev, dev_wall = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            host_batch(n)
            host.append(1e3 * (time.perf_counter() - t0))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            dr.sample(n)
            e1.record()
            torch.cuda.synchronize()
            dev_wall.append(1e3 * (time.perf_counter() - t0))
            dev_ev.append(e0.elapsed_time(e1))
        # the kernel alone: back-to-back launches into the same tensors
        out = dr.sample(n)
        burst, kernel_us = 20, []
        for rep in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(burst):
                rc = dr.lib.rz_replay_sample(dr.handle, args.seed, 1000 + rep * burst + i, n, out[0].data_ptr(), out[1].data_ptr(),
                                             out[2].data_ptr(), dr._stream())
                assert rc == 0
            e1.record()
            torch.cuda.synchronize()
            kernel_us.append(1e3 * e0.elapsed_time(e1) / burst)
        k = statistics.median(kernel_us)
        rate = n * entry_bytes(A) / (k * 1e-6)
        lines.append('batch %5d  host route ms: %s | device route ms (events): %s | device route ms (host clock, synchronised): %s' % (
            n, spread(host), spread(dev_ev), spread(dev_wall)))
        lines.append('batch %5d  k_replay_sample: %.2f us per launch (median of 10 bursts of %d), %d bytes per entry -> %.3f TB/s = %.1f %% of '
                     'the %.1f TB/s HBM specification, %.1f %% of the %.2f TB/s a copy reaches' % (
                         n, k, burst, entry_bytes(A), rate / 1e12, 100 * rate / HBM_PEAK, HBM_PEAK / 1e12, 100 * rate / HBM_MEASURED,
                         HBM_MEASURED / 1e12))
    dr.close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
