#!/usr/bin/env python3
"""A / B of continuous self-play (BatchedSelfPlay.stream_collect) against the round the trainer plays (run_device of slots x 1 fresh
ids), in ONE process: 15x15, 800 playouts, 512 slots, one random-init net with constant weights.  After a warm-up the two routes
alternate, ``--rounds`` rounds each: finished games / s and moves / s per round, the medians, A's own spread; then one run_device of
eight rounds' ids as the steady rate, and a whole move by HIP events with the ring queue and with the linear one.

    python profiles/ab_continuous.py > profiles/continuous/ab.txt

(The trainer's wall time per round with and without --continuous-selfplay, and the parent commit run twice, are separate runs of
tools/train_alphazero.py: see the notes at the end of profiles/continuous/ab.txt.)"""
import argparse
import statistics
import sys
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--board', type=int, default=15)
    ap.add_argument('--playouts', type=int, default=800)
    ap.add_argument('--slots', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steady', type=int, default=8, help='rounds of ids in the one long run_device')
    args = ap.parse_args()
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    from rlzero_amd.selfplay import BatchedSelfPlay
    torch.manual_seed(0)
    net = PolicyValueNet(args.board).to('cuda:0')
    kw = dict(board=args.board, n_in_row=5, n_games=args.slots, n_playout=args.playouts, device='cuda:0', seed=1)
    a = BatchedSelfPlay.for_network(net, **kw)
    b = BatchedSelfPlay.for_network(net, **kw)
    print('# %dx%d, %d playouts, %d slots, %d lane(s); %s' % (args.board, args.board, args.playouts, args.slots, len(a.lanes), torch.cuda.get_device_name(0)))
    n, next_id = args.slots, [0]

    def round_a():
        ids = range(next_id[0], next_id[0] + n)
        next_id[0] += n
        t0 = time.perf_counter()
        out = a.run_device(ids)
        return out, time.perf_counter() - t0

    def round_b():
        t0 = time.perf_counter()
        out = b.stream_collect(n)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    round_a()                       # warm-up: A's attach and first round
    b.stream_start(first_game_id=10 ** 6)
    round_b()
    round_b()                       # (the stream's first rounds start every slot at ply 0, like A's: not its steady state)
    rates = {'A': [], 'B': []}
    print('route round games seconds games/s moves/s')
    for r in range(args.rounds):
        for name, fn in (('A', round_a), ('B', round_b)):
            out, dt = fn()
            moves = sum(len(t.moves) for t in out)
            rates[name].append((len(out) / dt, moves / dt))
            print('%s %d %d %.3f %.1f %.0f' % (name, r, len(out), dt, len(out) / dt, moves / dt), flush=True)
    dropped = b.stream_stop()
    for name in 'AB':
        g = [x[0] for x in rates[name]]
        print('# %s: median %.1f games/s (min %.1f, max %.1f, spread %.1f), median %.0f moves/s' % (
            name, statistics.median(g), min(g), max(g), max(g) - min(g), statistics.median([x[1] for x in rates[name]])))
    ga, gb = [x[0] for x in rates['A']], [x[0] for x in rates['B']]
    print('# B / A = %.3f; B above A by more than A\'s spread: %s (%d games were running when the stream stopped)' % (
        statistics.median(gb) / statistics.median(ga), statistics.median(gb) - statistics.median(ga) > max(ga) - min(ga), dropped))
    ids = range(next_id[0], next_id[0] + args.steady * n)
    t0 = time.perf_counter()
    out = a.run_device(ids)
    dt = time.perf_counter() - t0
    print('# steady: run_device of %d ids: %.1f games/s, %.0f moves/s' % (len(out), len(out) / dt, sum(len(t.moves) for t in out) / dt))
    # a whole move by HIP events: the same object attached with the linear queue and with the ring, every slot mid-game
    for ring in (False, True):
        if ring:
            a.stream_start(first_game_id=2 * 10 ** 6)
            step = a._stream_round
        else:
            a.device_attach(queue_capacity=4 * n)
            a.device_queue(range(3 * 10 ** 6, 3 * 10 ** 6 + 4 * n))
            step = a.play_move_device
        for _ in range(6):
            step()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(a.lanes[0].stream)
        for _ in range(8):
            step()
        ev[1].record(a.lanes[0].stream)
        torch.cuda.synchronize()
        print('# a whole move, %s queue: %.3f ms (8 moves by HIP events on lane 0)' % ('ring' if ring else 'linear', ev[0].elapsed_time(ev[1]) / 8))
        if ring:
            a.stream_stop()
        else:
            a.device_drain()
            a.device_stop()


if __name__ == '__main__':
    main()
