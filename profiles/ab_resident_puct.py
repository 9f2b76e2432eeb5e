#!/usr/bin/env python3
"""The resident search under PUCT (rz_net_search_resident_puct, HipNetEvaluator.resident_puct) against the three-launch PUCT step as
self-play runs it (hipGraph chunks of 16 simulations, use_graph=True): HIP events on the stream, the routes alternating search by
search, medians of --reps searches after --warm; one run.

  search   per cell (board, simulations, games): every rep resets the roots (outside the timed window) and times ONE search of every
           game -- three-launch on this tree, resident on this tree and, with --parent-tree, three-launch on a build of the parent
           commit.  One process holds one ABI, so the parent's library runs in a child process started before this one touches the
           GPU; the child measures its search in the same round, when it is told to, while this process waits (and the other way
           round): the two never run together.  The three-launch code is the same in both trees, so the two baselines differ by the
           spread of identical code; the file states it.
  move     a WHOLE move of run_device (Connect4, 256 games, 400 playouts; the move step on the device) with the switch off and on,
           move by move in turn: first to last event on the lane's stream.

    python profiles/ab_resident_puct.py [--out profiles/resident_puct/ab.txt] [--parent-tree DIR] [--reps 30] [--warm 3]

A measurement, not a gate: nothing here is asserted anywhere; README and DESIGN quote only what the file holds."""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, game, board, n_in_row, simulations, games)
CELLS = [('connect4', 'connect4', (6, 7), 4, 400, 64), ('connect4', 'connect4', (6, 7), 4, 400, 256), ('gomoku 9x9', 'gomoku', 9, 5, 200, 64),
         ('gomoku 6x6', 'gomoku', 6, 4, 400, 16), ('tictactoe', 'gomoku', 3, 3, 25, 1)]


def spread(xs):
    return 'median %8.3f  min %8.3f  max %8.3f' % (statistics.median(xs), min(xs), max(xs))


class Cell(object):
    """One engine + evaluator of a cell on one route; ``search()`` -> ms of one search of every game from fresh roots."""

    def __init__(self, torch, cell, resident, seed=3):
        from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
        from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
        _, game, board, n_in_row, sims, games = cell
        rows, cols = board if game == 'connect4' else (board, board)
        acts = cols if game == 'connect4' else rows * cols
        torch.manual_seed(seed)
        net = PolicyValueNet(rows, cols, cols) if game == 'connect4' else PolicyValueNet(rows)
        with torch.no_grad():
            net.act_fc1.weight.mul_(20.0)   # (priors that shape the search, as in tests/test_resident_puct_gpu.py)
        self.torch, self.sims, self.resident = torch, sims, resident
        self.eng = MCTSEngine(board, n_in_row, n_games=games, n_playout=sims, c_puct=5.0, device='cuda:0', game=game, score_mode='puct',
                              add_noise=True, noise_seed=seed)
        self.ev = HipNetEvaluator(net, (rows, cols, acts), 'cuda:0', max_boards=games)
        if resident:
            self.ev.resident_puct = True
            if not self.ev.resident_ok(self.eng):
                raise SystemExit('the resident PUCT route does not serve cell %r' % (cell, ))
        self.per = self.eng.graph_chunk(16)
        self.eng.reset_games()
        if not resident:
            self.eng.warm_graph(self.ev, self.per)

    def search(self):
        t = self.torch
        self.eng.reset_games()
        self.eng.set_noise_keys()
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        a.record()
        self.eng.simulate(self.ev, self.sims, use_graph=not self.resident, sims_per_graph=self.per)
        b.record()
        t.cuda.synchronize()
        return a.elapsed_time(b)

    def close(self):
        self.eng.check()
        self.eng.close()
        self.ev.hip.close()


def worker(tree):
    """The child: the three-launch step of the tree at ``tree`` (a built checkout of the parent commit), told what to do line by line."""
    sys.path.insert(0, tree)
    import torch
    import rlzero_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(rlzero_amd.__file__))) == os.path.abspath(tree)
    cell = None
    print('ready', flush=True)
    for line in sys.stdin:
        word = line.split()
        if word[0] == 'cell':
            cell = Cell(torch, CELLS[int(word[1])], False)
            print('ok', flush=True)
        elif word[0] == 'go':
            print('%.6f' % cell.search(), flush=True)
        elif word[0] == 'done':
            cell.close()
            cell = None
            print('ok', flush=True)
        else:
            break


class Parent(object):
    def __init__(self, tree):
        env = dict(os.environ)
        env['PYTHONPATH'] = tree   # (this tree's package must not shadow the child's)
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', '--parent-tree', tree], stdin=subprocess.PIPE,
                                     stdout=subprocess.PIPE, universal_newlines=True, env=env, cwd=tree)
        assert self.ask(None) == 'ready'

    def ask(self, line):
        if line is not None:
            self.proc.stdin.write(line + '\n')
            self.proc.stdin.flush()
        got = self.proc.stdout.readline().strip()
        if not got:
            raise SystemExit('the parent tree\'s worker ended (exit %r)' % self.proc.poll())
        return got

    def close(self):
        self.proc.stdin.write('quit\n')
        self.proc.stdin.flush()
        self.proc.wait(timeout=60)


def one_move(sp, torch):
    """One move of every lane between two events per lane -> ms of the slowest lane (profiles/ab_value_targets.py's)."""
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


def part_move(args, torch, say):
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    from rlzero_amd.selfplay import BatchedSelfPlay
    games, sims = 256, 400
    players = {}
    for name, on in (('three-launch', False), ('resident', True)):
        torch.manual_seed(args.seed)
        net = PolicyValueNet(6, 7, 7)
        with torch.no_grad():
            net.act_fc1.weight.mul_(20.0)
        sp = BatchedSelfPlay.for_network(net, (6, 7), 4, n_games=games, n_playout=sims, c_puct=5.0, device='cuda:0', game='connect4',
                                         net_shape=(6, 7, 7), temperature=1.0, seed=args.seed, score_mode='puct', resident_puct=on)
        sp.device_attach(queue_capacity=1 << 14)
        sp.device_queue(list(range(1 << 14)))
        players[name] = sp
    say('move: Connect4, %d games in flight, %d playouts, run_device\'s move (the move step on the device), %d lane(s); whole-move graph: '
        'three-launch %s, resident %s; ms per move, %d moves after %d, the two objects in turn' % (
            games, sims, len(players['resident'].lanes), 'yes' if players['three-launch'].lanes[0].move_graph is not None else 'no',
            'yes' if players['resident'].lanes[0].move_graph is not None else 'no', args.reps, args.warm))
    got = dict((name, []) for name in players)
    for rep in range(args.warm + args.reps):
        for name, sp in players.items():
            ms = one_move(sp, torch)
            if rep >= args.warm:
                got[name].append(ms)
    med = dict((name, statistics.median(xs)) for name, xs in got.items())
    for name in players:
        say('  %-13s %s   %7.2f M simulations / s' % (name, spread(got[name]), games * sims / med[name] / 1e3))
    say('  resident / three-launch (simulations / s): %.3f' % (med['three-launch'] / med['resident']))
    for sp in players.values():
        sp.device_stop()
        sp.check()
        for ln in sp.lanes:
            ln.eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'resident_puct', 'ab.txt'))
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit (its three-launch step is timed in the same rounds)')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warm', type=int, default=3)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--parts', default='search,move')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.parent_tree))
    parent = Parent(os.path.abspath(args.parent_tree)) if args.parent_tree else None   # (before this process opens the GPU)
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        if parent is not None:
            parent.close()
        raise SystemExit('profiles/ab_resident_puct.py measures on the GPU: none here')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_resident_puct.py --parts %s: %s; HIP events on the stream; ONE run' % (args.parts, torch.cuda.get_device_name(0)))
    say('# PUCT, c_puct 5, Dirichlet noise on, nets with act_fc1.weight x 20; every search from fresh roots; ms per search of all games')
    if 'search' in args.parts.split(','):
        gaps = []
        for i, cell in enumerate(CELLS):
            name, _, _, _, sims, games = cell
            routes = {'three-launch': Cell(torch, cell, False), 'resident': Cell(torch, cell, True)}
            if parent is not None:
                assert parent.ask('cell %d' % i) == 'ok'
            got = dict((k, []) for k in list(routes) + (['three-launch (parent)'] if parent else []))
            for rep in range(args.warm + args.reps):
                for k, c in routes.items():
                    ms = c.search()
                    if rep >= args.warm:
                        got[k].append(ms)
                if parent is not None:
                    ms = float(parent.ask('go'))
                    if rep >= args.warm:
                        got['three-launch (parent)'].append(ms)
            say('search: %s, %d simulations, %d game(s); %d searches after %d, the routes in turn' % (name, sims, games, args.reps, args.warm))
            med = dict((k, statistics.median(xs)) for k, xs in got.items())
            for k in got:
                say('  %-22s %s   %8.3f M simulations / s' % (k, spread(got[k]), games * sims / med[k] / 1e3))
            say('  resident / three-launch (simulations / s): %.3f' % (med['three-launch'] / med['resident']))
            if parent is not None:
                gap = med['three-launch'] / med['three-launch (parent)'] - 1.0
                gaps.append(gap)
                say('  three-launch, this tree against the parent\'s build (the same code): %+.2f %% of the time' % (100.0 * gap))
                assert parent.ask('done') == 'ok'
            for c in routes.values():
                c.close()
        if gaps:
            say('# the same three-launch code in two builds and two processes: medians %.2f %% .. %+.2f %% apart over the cells -- the spread '
                'of identical code in this run' % (100.0 * min(gaps), 100.0 * max(gaps)))
        else:
            say('# no --parent-tree: the parent\'s build was not timed in this run')
    if parent is not None:
        parent.close()
    if 'move' in args.parts.split(','):
        part_move(args, torch, say)
    out.close()


if __name__ == '__main__':
    main()
