#!/usr/bin/env python3
"""What a Connect4 mini-batch costs on either replay buffer, and what one Reanalyse chunk costs, in one process.

  batches     --games synthetic 6 x 7 games (random legal drops that complete no line) in the trainer's host ReplayBuffer(game=
              'connect4') and in a DeviceReplay(game='connect4'); for every batch size the two routes ALTERNATE, --reps times each
              after warm-up, an event on the stream before and after each:
                host route    random.sample + stacking + AlphaZeroAgent._tensor for the three columns (the host-to-device copies end it);
                device route  DeviceReplay.sample (one launch: k_replay_sample<true>).
              The events of the host route bracket host work too (the stream is idle until its copies arrive); the host clock,
              synchronised, is printed next to both.
  reanalyse   one chunk of --slots positions drawn on the device and searched again at --playouts simulations
              (ReplayReanalyser.reanalyse_sample), events from the first mark to the last, and the split by stage.

    python profiles/ab_replay_connect4.py [--out profiles/replay_connect4/ab.txt] [--games 512] [--reps 30] [--batches 32 512 4096]

No figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import importlib.util
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ('positions', 'roots', 'search', 'update')


def spread(xs):
    return 'median %.3f  min %.3f  max %.3f' % (statistics.median(xs), min(xs), max(xs))


def synthetic_games(rows, cols, n_in_row, n_games, seed):
    """Legal games of seeded random drops none of which completes a line (to a full board, or until no such drop is left), with the
    uniform pi over the columns that are not full."""
    import numpy as np
    from rlzero_amd.games.connect4.connect4_env import _start_masks
    from rlzero_amd.games.gomoku.gomoku_env import has_line
    from rlzero_amd.selfplay import Trajectory
    masks = _start_masks(rows, cols, n_in_row)
    games = []
    for g in range(n_games):
        rs = np.random.RandomState(seed * 100003 + g)
        bits, height, moves, pis = [0, 0], [0] * cols, [], []
        for p in range(rows * cols):
            open_ = [c for c in range(cols) if height[c] < rows]
            safe = [int(c) for c in rs.permutation(open_) if not has_line(bits[p & 1] | (1 << (height[c] * cols + c)), masks, n_in_row)]
            if not safe:
                break
            row = np.zeros(cols, dtype=np.float32)
            row[open_] = 1.0 / len(open_)
            pis.append(row)
            c = safe[0]
            bits[p & 1] |= 1 << (height[c] * cols + c)
            height[c] += 1
            moves.append(c)
        games.append(Trajectory(g, (rows, cols), n_in_row, moves, np.array(pis, dtype=np.float32).reshape(len(moves), cols), g % 3 - 1, game='connect4'))
    return games


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'replay_connect4', 'ab.txt'))
    ap.add_argument('--rows', type=int, default=6)
    ap.add_argument('--cols', type=int, default=7)
    ap.add_argument('--n-in-row', type=int, default=4)
    ap.add_argument('--games', type=int, default=512)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batches', type=int, nargs='+', default=[32, 512, 4096])
    ap.add_argument('--playouts', type=int, default=400)
    ap.add_argument('--slots', type=int, default=512)
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_replay_connect4.py measures on the GPU: none here')
    from rlzero_amd.games.gomoku.alphazero_agent import AlphaZeroAgent
    from rlzero_amd.replay import DeviceReplay, ReplayReanalyser
    spec = importlib.util.spec_from_file_location('train_alphazero', os.path.join(REPO, 'tools', 'train_alphazero.py'))
    trainer = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(trainer)
    random.seed(args.seed)
    torch.manual_seed(args.seed)
    board = (args.rows, args.cols)
    games = synthetic_games(args.rows, args.cols, args.n_in_row, args.games, args.seed)
    positions = sum(len(t.moves) for t in games)
    agent = AlphaZeroAgent(args.rows, device='cuda:0', board_width=args.cols, n_actions=args.cols)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_replay_connect4.py: Connect4 %d x %d, %d synthetic games, %d positions (%d entries: two symmetries), %s' % (
        args.rows, args.cols, args.games, positions, 2 * positions, torch.cuda.get_device_name(0)))
    buf = trainer.ReplayBuffer(2 * positions, board, game='connect4')
    t0 = time.perf_counter()
    for t in games:
        buf.extend_samples(t.training_samples())
    host_ingest = 1e3 * (time.perf_counter() - t0)
    dr = DeviceReplay(board, positions, device='cuda:0', seed=args.seed, game='connect4')
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dr.add(games)
    torch.cuda.synchronize()
    say('ingest of the %d games, ms (one run, host clock): host extend_samples(training_samples()) %.1f | device add %.1f' % (
        args.games, host_ingest, 1e3 * (time.perf_counter() - t0)))
    assert len(dr) == len(buf) == 2 * positions

    def host_batch(n):
        batch = random.sample(buf, n)
        return [agent._tensor(list(col)) for col in zip(*batch)]

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn(n)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)

    say('batches: ms per mini-batch, the two routes alternating, %d repetitions after 3' % args.reps)
    for n in args.batches:
        n = min(n, len(buf))   # (random.sample draws without replacement)
        for _ in range(3):
            host_batch(n)
            dr.sample(n)
        torch.cuda.synchronize()
        host, device = [], []
        for _ in range(args.reps):
            host.append(timed(host_batch, n))
            device.append(timed(dr.sample, n))
        say('  batch %5d  host route:   events %s | host clock %s' % (n, spread([a for a, _ in host]), spread([b for _, b in host])))
        say('  batch %5d  device route: events %s | host clock %s' % (n, spread([a for a, _ in device]), spread([b for _, b in device])))

    # one Reanalyse chunk
    marks = []

    def mark(label):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append((label, ev))
    rean = ReplayReanalyser(agent.policy_value_net, dr, args.n_in_row, args.playouts, slots=args.slots, seed=args.seed)
    rean.timer = mark
    route = rean.evaluator.route(rean.engine)
    totals, stages = [], {k: [] for k in STAGES}
    for rep in range(args.reps + 3):
        marks.clear()
        rean.reanalyse_sample(args.slots)
        torch.cuda.synchronize()
        if rep < 3:
            continue
        totals.append(marks[0][1].elapsed_time(marks[-1][1]))
        for (_, a), (label, b) in zip(marks, marks[1:]):
            stages[label].append(a.elapsed_time(b))
    rean.check()
    med = statistics.median(totals)
    say('reanalyse: one chunk of %d drawn positions at %d playouts (route %s), ms, %d repetitions after 3: events first to last %s' % (
        args.slots, args.playouts, 'resident' if getattr(route, 'resident', False) else 'by steps', args.reps, spread(totals)))
    say('  medians: positions %.3f | roots + discarded-tree flush %.3f | search %.3f | visits + update %.3f' % tuple(
        statistics.median(stages[k]) for k in STAGES))
    say('  %.0f positions/s, %.2f M searched simulations/s' % (args.slots / med * 1e3, args.slots * args.playouts / med / 1e3))
    rean.close()
    dr.close()
    out.close()


if __name__ == '__main__':
    main()
