#!/usr/bin/env python3
"""What forced playouts and policy target pruning cost a whole move of run_device (rz_set_forced_playouts, rz_play_set_pruned_visits):
Connect4, 256 games in flight, 400 playouts, the resident PUCT route, the move step on the device (one whole-move hipGraph per move).
HIP events on the lane's stream, first to last event of a move; medians of --reps moves after --warm; one run.

Three players of this tree in one process -- the option off, on (k = 2, pruning: the launch of k_root_pruned in front of the draw and
its ring), on without pruning -- take their moves in turn.  With --parent-tree two more players, both of a build of the parent commit
(one process holds one ABI, so each is a child process started before this one touches the GPU), move in the same rounds when they
are told to, while this process waits: the processes never run together.  The two parent players run identical code; how far their
medians lie apart is the spread against which "off" is read.  A sixth player -- this tree with the option off, in a child process of
its own like the parent's two -- tells the code apart from the company: the three players of this process share it, the parent's do not.

    python profiles/ab_forced_playouts.py [--out profiles/forced_playouts/ab.txt] [--parent-tree DIR] [--reps 30] [--warm 5]

A measurement, not a gate: nothing here is asserted anywhere; README and DESIGN quote only what the file holds."""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES, SIMS = 256, 400


def spread(xs):
    return 'median %8.3f  min %8.3f  max %8.3f' % (statistics.median(xs), min(xs), max(xs))


def player(torch, seed, forced=None):
    """A BatchedSelfPlay on the resident PUCT route with the move step attached and games queued."""
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    from rlzero_amd.selfplay import BatchedSelfPlay
    torch.manual_seed(seed)
    net = PolicyValueNet(6, 7, 7)
    with torch.no_grad():
        net.act_fc1.weight.mul_(20.0)   # (priors that shape the search, as in tests/test_resident_puct_gpu.py)
    kw = {} if forced is None else dict(forced_playouts=forced)
    sp = BatchedSelfPlay.for_network(net, (6, 7), 4, n_games=GAMES, n_playout=SIMS, c_puct=5.0, device='cuda:0', game='connect4',
                                     net_shape=(6, 7, 7), temperature=1.0, seed=seed, score_mode='puct', resident_puct=True, **kw)
    sp.device_attach(queue_capacity=1 << 14)
    sp.device_queue(list(range(1 << 14)))
    assert sp.lanes[0].move_graph is not None
    return sp


def one_move(sp, torch):
    """One move of every lane between two events per lane -> ms of the slowest lane (profiles/ab_resident_puct.py's)."""
    pairs = []
    for lane in sp.lanes:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with sp._on(lane):
            a.record(lane.stream)
            lane.uncopied.append(lane.eng.play_move_replay(lane.move_graph))
            b.record(lane.stream)
        pairs.append((a, b))
        sp._read_back(lane)
    for lane in sp.lanes:
        sp._harvest(lane, keep=0)
    torch.cuda.synchronize()
    return max(a.elapsed_time(b) for a, b in pairs)


def close(sp):
    sp.device_stop()
    sp.check()
    for lane in sp.lanes:
        lane.eng.close()


def worker(tree, seed):
    """The child: one player of the tree at ``tree`` (a built checkout of the parent commit), told line by line when to move."""
    sys.path.insert(0, tree)
    import torch
    import rlzero_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(rlzero_amd.__file__))) == os.path.abspath(tree)
    sp = player(torch, seed)
    print('ready', flush=True)
    for line in sys.stdin:
        if line.split()[0] != 'go':
            break
        print('%.6f' % one_move(sp, torch), flush=True)
    close(sp)


class Parent(object):
    def __init__(self, tree, seed):
        env = dict(os.environ)
        env['PYTHONPATH'] = tree   # (this tree's package must not shadow the child's)
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', '--parent-tree', tree, '--seed', str(seed)],
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE, universal_newlines=True, env=env, cwd=tree)
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
        self.proc.wait(timeout=120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'forced_playouts', 'ab.txt'))
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit (two players of it move in the same rounds)')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warm', type=int, default=5)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.parent_tree), args.seed)
    # (the children first, one after the other, before this process opens the GPU)
    parents = [Parent(os.path.abspath(args.parent_tree), args.seed) for _ in range(2)] if args.parent_tree else []
    own = [Parent(REPO, args.seed)] if args.parent_tree else []   # (this tree, option off, alone in its process)
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        for p in parents + own:
            p.close()
        raise SystemExit('profiles/ab_forced_playouts.py measures on the GPU: none here')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    players = [('off', player(torch, args.seed)), ('on (k = 2, pruning)', player(torch, args.seed, (2.0, True))),
               ('on, no pruning', player(torch, args.seed, (2.0, False)))]
    say('# profiles/ab_forced_playouts.py: %s; HIP events on the lane\'s stream; ONE run' % torch.cuda.get_device_name(0))
    say('# a whole move of run_device: Connect4, %d games in flight, %d playouts, PUCT (c_puct 5, Dirichlet noise on, act_fc1.weight x 20), the '
        'resident PUCT route, one whole-move hipGraph per move, %d lane(s)' % (GAMES, SIMS, len(players[0][1].lanes)))
    say('# ms per move: medians of %d moves after %d; the players move in turn, round by round (the games go on from move to move, so the '
        'boards fill up alike for all)' % (args.reps, args.warm))
    names = [n for n, _ in players] + ['parent commit, player %d' % (i + 1) for i in range(len(parents))] + ['off, own process'] * len(own)
    got = dict((n, []) for n in names)
    for rep in range(args.warm + args.reps):
        for name, sp in players:
            ms = one_move(sp, torch)
            if rep >= args.warm:
                got[name].append(ms)
        for i, p in enumerate(parents):
            ms = float(p.ask('go'))
            if rep >= args.warm:
                got['parent commit, player %d' % (i + 1)].append(ms)
        for p in own:
            ms = float(p.ask('go'))
            if rep >= args.warm:
                got['off, own process'].append(ms)
    med = dict((n, statistics.median(xs)) for n, xs in got.items())
    for n in names:
        say('  %-24s %s   %7.2f M simulations / s' % (n, spread(got[n]), GAMES * SIMS / med[n] / 1e3))
    say('  on / off (time per move): %.4f    on without pruning / off: %.4f' % (med[names[1]] / med['off'], med[names[2]] / med['off']))
    if parents:
        a, b = med['parent commit, player 1'], med['parent commit, player 2']
        lo, hi = min(a, b), max(a, b)
        say('  the two parent players (identical code, two processes): %.3f and %.3f ms, %.2f %% apart' % (a, b, 100.0 * (hi / lo - 1.0)))
        for name in ['off'] + ['off, own process'] * len(own):
            if lo <= med[name] <= hi:
                say('  "%s" lies between them' % name)
            else:
                edge = lo if med[name] < lo else hi
                say('  "%s" lies OUTSIDE them: %+.2f %% of the nearer one\'s time' % (name, 100.0 * (med[name] / edge - 1.0)))
    else:
        say('# no --parent-tree: the parent\'s build was not timed in this run')
    for p in parents + own:
        p.close()
    for _, sp in players:
        close(sp)
    out.close()


if __name__ == '__main__':
    main()
