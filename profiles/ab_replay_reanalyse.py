#!/usr/bin/env python3
"""What Reanalyse for the AlphaZero device replay costs (rlzero_amd/replay.py: ReplayReanalyser), in one process, HIP events on the
launch stream, medians after warm-up.

  refresh     a DeviceReplay of --positions synthetic positions (random legal games of --plies plies without a line of five: what
              is measured is the search of a stored position, not where it came from); a ReplayReanalyser(--playouts, --slots)
              refreshes --slots, 4 x --slots and all positions drawn on the device, the sizes alternating, --reps times each.
              Events between the stages of every chunk give the split: positions (one launch per refresh) | roots (rz_set_roots,
              with the flush of the PREVIOUS chunk's discarded trees: see flush) | search (the bases of the new roots and the
              resident search) | visits + update, summed over the refresh's chunks; positions and searched simulations per second.
  flush       the share of the discarded trees' prior flush: the roots stage of a chunk whose engine has pending priors against
              the same stage after an explicit flush_deferred() (timed on its own), --reps chunks each.
  selfplay    the self-play rate of the same process for comparison: BatchedSelfPlay.for_network at --slots games, --playouts,
              moves on the device, simulations per second over --selfplay-moves moves after warm-up.

    python profiles/ab_replay_reanalyse.py [--out profiles/replay_reanalyse/ab.txt] [--board 15] [--playouts 800] [--slots 512] [--reps 30]

No figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ('positions', 'roots', 'search', 'update')


def spread(xs):
    return 'median %.3f  min %.3f  max %.3f' % (statistics.median(xs), min(xs), max(xs))


class StageEvents(object):
    """ReplayReanalyser.timer: an event on the stream at every mark; ``take`` -> ms per stage (summed over chunks) and in all."""

    def __init__(self, torch):
        self.torch, self.marks = torch, []

    def __call__(self, label):
        ev = self.torch.cuda.Event(enable_timing=True)
        ev.record()
        self.marks.append((label, ev))

    def take(self):
        self.torch.cuda.synchronize()
        out = dict.fromkeys(STAGES, 0.0)
        for (_, a), (label, b) in zip(self.marks, self.marks[1:]):
            out[label] += a.elapsed_time(b)
        out['total'] = self.marks[0][1].elapsed_time(self.marks[-1][1])
        self.marks = []
        return out


def synthetic_games(board, n_in_row, plies, n_games, seed):
    """Legal games of ``plies`` seeded random moves none of which completes a line, with the uniform pi over the empty cells."""
    import numpy as np
    from rlzero_amd.games.gomoku.gomoku_env import _start_masks, has_line
    from rlzero_amd.selfplay import Trajectory
    A = board * board
    masks = _start_masks(board, n_in_row)
    games = []
    for g in range(n_games):
        rs = np.random.RandomState(seed * 100003 + g)
        bits, moves = [0, 0], []
        for p in range(plies):
            for c in rs.permutation(A):
                c = int(c)
                if not ((bits[0] | bits[1]) >> c) & 1 and not has_line(bits[p & 1] | (1 << c), masks, n_in_row):
                    moves.append(c)
                    bits[p & 1] |= 1 << c
                    break
            else:
                break
        pis = np.zeros((len(moves), A), dtype=np.float32)
        for p in range(len(moves)):
            pis[p] = 1.0 / (A - p)
            pis[p, moves[:p]] = 0.0
        games.append(Trajectory(g, board, n_in_row, moves, pis, -1))
    return games


def part_refresh(args, torch, say, net, dev):
    from rlzero_amd.replay import ReplayReanalyser
    rean = ReplayReanalyser(net, dev, args.n_in_row, args.playouts, slots=args.slots, seed=args.seed)
    rean.timer = StageEvents(torch)
    sizes = (args.slots, 4 * args.slots, dev.positions)
    route = rean.evaluator.route(rean.engine)
    say('refresh: %d positions held, %d x %d, %d playouts, %d slots, route %s; ms per refresh, %d repetitions after 3, the sizes alternating' % (
        dev.positions, args.board, args.board, args.playouts, args.slots,
        'k_delta_res' if route.resident_delta else 'resident' if route.resident else 'by steps', args.reps))
    for _ in range(3):
        for n in sizes:
            rean.reanalyse_sample(n)
            rean.timer.take()
    got = {n: [] for n in sizes}
    wall = {n: [] for n in sizes}
    for _ in range(args.reps):
        for n in sizes:
            t0 = time.perf_counter()
            rean.reanalyse_sample(n)
            got[n].append(rean.timer.take())
            wall[n].append(1e3 * (time.perf_counter() - t0))
    for n in sizes:
        med = {k: statistics.median(r[k] for r in got[n]) for k in STAGES + ('total', )}
        say('  %6d positions (%d chunks): events first to last %s | host clock incl. synchronise median %.3f' % (
            n, -(-n // args.slots), spread([r['total'] for r in got[n]]), statistics.median(wall[n])))
        say('         medians: positions %.3f | roots + discarded-tree flush %.3f | bases + search %.3f | visits + update %.3f' % (
            med['positions'], med['roots'], med['search'], med['update']))
        say('         %.0f positions/s, %.2f M searched simulations/s (first to last event)' % (
            n / med['total'] * 1e3, n * args.playouts / med['total'] / 1e3))
    rean.check()
    return rean


def part_flush(args, torch, say, rean, dev):
    """The roots stage with and without the pending priors of the previous chunk's trees."""
    eng = rean.engine
    where, stones, to_move, last_move, _ = dev.position_roots(None, n=args.slots, seed=args.seed, step=1 << 20, pad_to=args.slots)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def roots():
        eng.set_roots_device(stones, to_move, last_move, reset_trees=True)
    with_flush, flush_alone, roots_alone = [], [], []
    for rep in range(args.reps + 3):
        roots()
        eng.simulate(rean.evaluator, args.playouts)
        pending = eng._def_pending
        x = timed(roots)                      # (flushes the search's priors, then sets the roots)
        eng.simulate(rean.evaluator, args.playouts)
        y = timed(eng.flush_deferred)
        z = timed(roots)                      # (nothing pending)
        if rep >= 3:
            with_flush.append(x), flush_alone.append(y), roots_alone.append(z)
    say('flush: one chunk of %d searched roots, %d repetitions after 3 (%d steps of priors pending after a search)' % (args.slots, args.reps, pending))
    say('  roots with the discarded trees\' flush  %s' % spread(with_flush))
    say('  the flush alone                        %s' % spread(flush_alone))
    say('  roots with nothing pending             %s' % spread(roots_alone))


def part_selfplay(args, torch, say, net):
    from rlzero_amd.selfplay import BatchedSelfPlay
    sp = BatchedSelfPlay.for_network(net, args.board, args.n_in_row, n_games=args.slots, n_playout=args.playouts, c_puct=5,
                                     device='cuda:0', temperature=1.0, seed=args.seed)
    rates = []
    for rep in range(3):
        ids = list(range(rep * args.slots, (rep + 1) * args.slots))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trajs = sp.run_device(ids)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rates.append(sum(len(t.moves) for t in trajs) * args.playouts / dt / 1e6)
    say('selfplay: %d games in flight, %d playouts, run_device of %d games, three rounds (the first warms up): %s M simulations/s (host clock)' % (
        args.slots, args.playouts, args.slots, ' '.join('%.2f' % r for r in rates)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'replay_reanalyse', 'ab.txt'))
    ap.add_argument('--board', type=int, default=15)
    ap.add_argument('--n-in-row', type=int, default=5)
    ap.add_argument('--playouts', type=int, default=800)
    ap.add_argument('--slots', type=int, default=512)
    ap.add_argument('--positions', type=int, default=4096)
    ap.add_argument('--plies', type=int, default=64)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--parts', default='refresh,flush,selfplay')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_replay_reanalyse.py measures on the GPU: none here')
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    from rlzero_amd.replay import DeviceReplay
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_replay_reanalyse.py --parts %s: %s; HIP events on the launch stream unless a line says otherwise' % (
        args.parts, torch.cuda.get_device_name(0)))
    torch.manual_seed(args.seed)
    net = PolicyValueNet(args.board).to('cuda:0')
    dev = DeviceReplay(args.board, args.positions, device='cuda:0', seed=args.seed)
    dev.add(synthetic_games(args.board, args.n_in_row, args.plies, -(-args.positions // args.plies), args.seed))
    parts = args.parts.split(',')
    rean = None
    if 'refresh' in parts or 'flush' in parts:
        if 'refresh' in parts:
            rean = part_refresh(args, torch, say, net, dev)
        else:
            from rlzero_amd.replay import ReplayReanalyser
            rean = ReplayReanalyser(net, dev, args.n_in_row, args.playouts, slots=args.slots, seed=args.seed)
        if 'flush' in parts:
            part_flush(args, torch, say, rean, dev)
        rean.close()
    dev.close()
    if 'selfplay' in parts:
        part_selfplay(args, torch, say, net)
    out.close()


if __name__ == '__main__':
    main()
