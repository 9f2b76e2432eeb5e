#!/usr/bin/env python3
"""What the value targets from the search cost (rz_play_set_root_values, rz_replay_set_value_mix, rz_replay_update_values), in one
process, HIP events on the launch streams, medians of --reps after warm-up.

  move        a WHOLE move of self-play (BatchedSelfPlay.for_network at --board, --playouts, --slots games, moves on the device: the
              whole-move hipGraph where the route has one) on four objects measured in turn, move by move: one with the side ring
              of root values on, three with it off.  The three are identical code on identical settings: their spread is the
              spread of identical code, the yardstick for the ring's difference.  (A library of the parent commit cannot be loaded
              beside this one -- one process holds one ABI --; k_play_draw with the ring off differs from the parent's by one
              test of a kernel argument, profiles/value_targets/kernel_resources.txt.)  Per move: first event on a lane's stream to
              the last, the slowest lane.
  sample      DeviceReplay.sample(--batch) on a buffer with search values at lam = 0 (the kernels without q) and at lam = 0.5.
  reanalyse   ONE chunk of --slots positions (ReplayReanalyser.reanalyse_sample(--slots)) with targets 'pi', 'value' and 'both',
              in turn; first to last event of the refresh.

    python profiles/ab_value_targets.py [--out profiles/value_targets/ab.txt] [--board 15] [--playouts 800] [--slots 512] [--reps 30]

These are measurements, not gates: no figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(xs):
    return 'median %.3f  min %.3f  max %.3f' % (statistics.median(xs), min(xs), max(xs))


def one_move(sp, torch):
    """Enqueue one move of every lane between two events per lane -> ms of the slowest lane; the log rows are read as run_device
    reads them (stalls are answered, finished games leave their slots to the queue)."""
    pairs = []
    for lane in sp.lanes:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with sp._on(lane):
            a.record(lane.stream)
            if lane.move_graph is not None:
                lane.uncopied.append(lane.eng.play_move_replay(lane.move_graph))
            else:
                sp._simulate_lane(lane, host_counts=False)
                lane.uncopied.append(lane.eng.play_move())
            b.record(lane.stream)
        pairs.append((a, b))
        sp._read_back(lane)
    for lane in sp.lanes:
        sp._harvest(lane, keep=0)
    torch.cuda.synchronize()
    return max(a.elapsed_time(b) for a, b in pairs)


def part_move(args, torch, say, net):
    from rlzero_amd.selfplay import BatchedSelfPlay
    names = ['ring on', 'ring off (1)', 'ring off (2)', 'ring off (3)']
    players = []
    for i, name in enumerate(names):
        sp = BatchedSelfPlay.for_network(net, args.board, args.n_in_row, n_games=args.slots, n_playout=args.playouts, c_puct=5, device='cuda:0',
                                         temperature=1.0, seed=args.seed, root_values=(i == 0))
        sp.device_attach(queue_capacity=1 << 14)
        sp.device_queue(list(range(1 << 14)))
        players.append(sp)
    lane = players[0].lanes[0]
    say('move: %d x %d, %d playouts, %d games in flight, %d lane(s), whole-move graph %s; ms per move, %d moves after %d, the four objects in turn' % (
        args.board, args.board, args.playouts, args.slots, len(players[0].lanes), 'yes' if lane.move_graph is not None else 'no', args.reps, args.warm))
    got = dict((name, []) for name in names)
    for rep in range(args.warm + args.reps):
        for name, sp in zip(names, players):
            ms = one_move(sp, torch)
            if rep >= args.warm:
                got[name].append(ms)
    for name in names:
        say('  %-13s %s' % (name, spread(got[name])))
    off = [statistics.median(got[name]) for name in names[1:]]
    say('  medians of the three identical objects span %.3f ms; ring on minus their mean %.3f ms' % (
        max(off) - min(off), statistics.median(got[names[0]]) - sum(off) / len(off)))
    for sp in players:
        sp.device_stop()
        sp.check()
        for ln in sp.lanes:
            ln.eng.close()


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def part_sample(args, torch, say, dev):
    say('sample: %d entries of a buffer of %d positions (%d x %d) with search values; ms per launch, %d after %d, the two settings in turn' % (
        args.batch, dev.positions, args.board, args.board, args.reps, args.warm))
    got = {0.0: [], 0.5: []}
    for rep in range(args.warm + args.reps):
        for lam in got:
            dev.set_value_mix(lam)
            ms = timed(torch, lambda: dev.sample(args.batch, step=rep))
            if rep >= args.warm:
                got[lam].append(ms)
    for lam in got:
        say('  lam = %.1f (%s)  %s' % (lam, 'k_replay_sample<., false>' if lam == 0.0 else 'k_replay_sample<., true> ', spread(got[lam])))
    dev.set_value_mix(0.0)


def part_reanalyse(args, torch, say, net, dev):
    from rlzero_amd.replay import ReplayReanalyser
    kinds = ('pi', 'value', 'both')
    reans = dict((k, ReplayReanalyser(net, dev, args.n_in_row, args.playouts, slots=args.slots, seed=args.seed, targets=k)) for k in kinds)
    say('reanalyse: one chunk of %d positions, %d playouts; ms per refresh (first to last event), %d after %d, the three targets in turn' % (
        args.slots, args.playouts, args.reps, args.warm))
    got = dict((k, []) for k in kinds)
    for rep in range(args.warm + args.reps):
        for k in kinds:
            ms = timed(torch, lambda: reans[k].reanalyse_sample(args.slots, step=rep))
            if rep >= args.warm:
                got[k].append(ms)
    for k in kinds:
        say('  targets = %-6s %s' % (k, spread(got[k])))
    for r in reans.values():
        r.check()
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'value_targets', 'ab.txt'))
    ap.add_argument('--board', type=int, default=15)
    ap.add_argument('--n-in-row', type=int, default=5)
    ap.add_argument('--playouts', type=int, default=800)
    ap.add_argument('--slots', type=int, default=512)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--positions', type=int, default=4096)
    ap.add_argument('--plies', type=int, default=64)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warm', type=int, default=3)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--parts', default='move,sample,reanalyse')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, 'profiles'))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_value_targets.py measures on the GPU: none here')
    from ab_replay_reanalyse import synthetic_games
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    from rlzero_amd.replay import DeviceReplay
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_value_targets.py --parts %s: %s; HIP events on the launch streams' % (args.parts, torch.cuda.get_device_name(0)))
    torch.manual_seed(args.seed)
    net = PolicyValueNet(args.board).to('cuda:0')
    parts = args.parts.split(',')
    if 'move' in parts:
        part_move(args, torch, say, net)
    if 'sample' in parts or 'reanalyse' in parts:
        dev = DeviceReplay(args.board, args.positions, device='cuda:0', seed=args.seed, search_values=True)
        games = synthetic_games(args.board, args.n_in_row, args.plies, -(-args.positions // args.plies), args.seed)
        rs = np.random.RandomState(args.seed)
        for t in games:   # (what is measured is the kernels' work, not where the values came from)
            t.root_values = rs.uniform(-1.0, 1.0, size=len(t.moves)).astype(np.float32)
        dev.add(games)
        if 'sample' in parts:
            part_sample(args, torch, say, dev)
        if 'reanalyse' in parts:
            part_reanalyse(args, torch, say, net, dev)
        dev.close()
    out.close()


if __name__ == '__main__':
    main()
