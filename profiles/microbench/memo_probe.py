"""What the feature memo of k_delta_res<false> can serve (rlzero_amd/csrc/rz_memo.h), counted on the CPU with the oracle.

A leaf is a path of cells from the root of its move.  ``classify`` walks the leaves of ONE move in the order the search evaluated them
and applies the kernel's rule: a leaf of exactly two cells a, b with Chebyshev distance(a, b) >= 7 is a FAR pair; it is a HIT when an
earlier far pair of the same move has left the window of a (kind OWN) and the window of b (kind OPP_LAST), otherwise it runs its
passes and FILLS whichever of the two is missing -- over BOTH windows when neither is there, over the missing stone's window alone
when the other is (HALF_A: b's window served, a's run; HALF_B the other way round; rz_memo.h: served).  tests/test_delta_memo.py and
tests/test_delta_memo_half.py hold the kernel's counters to this function.

    python profiles/microbench/memo_probe.py [--moves 14] [--playouts 800] [--board 15] [--out profiles/r15/memo_probe.txt]

CPU only: RefSearch (oracle/mcts_ref.py) on the benchmark's net (torch.manual_seed(0)), a fresh search per move as the device's move
step makes one, moves drawn at T = 1 from the visit counts; about 2 s per move."""
import argparse
import os
import sys

MIN_DIST = 7   # rz_memo.h: kMinDist


def cheb(a, b, cols):
    return max(abs(a // cols - b // cols), abs(a % cols - b % cols))


def classify(paths, cols, min_dist=MIN_DIST, log=None):
    """``paths``: the leaves of one move in evaluation order, each a tuple of cells (y * cols + x) from the root.  -> dict of counts:
    leaves, depth1, depth2, deeper, far (depth 2, distance >= min_dist), b_seen / a_seen (far, and this b / a already in a far leaf
    of the move), hits (both), fills (entries written: the distinct a plus the distinct b of the far leaves), half_a (b seen, a new:
    a's window alone is run) and half_b (a seen, b new).  ``log``: a list that receives (kind, a, b) of every far leaf in order, kind one
    of 'hit', 'half_a', 'half_b', 'both' (both windows run)."""
    out = dict(leaves=0, depth0=0, depth1=0, depth2=0, deeper=0, far=0, a_seen=0, b_seen=0, hits=0, fills=0, half_a=0, half_b=0)
    own, opp = set(), set()
    for p in paths:
        out['leaves'] += 1
        out['depth%d' % len(p) if len(p) <= 2 else 'deeper'] += 1
        if len(p) != 2 or cheb(p[0], p[1], cols) < min_dist:
            continue
        a, b = p
        out['far'] += 1
        out['a_seen'] += a in own
        out['b_seen'] += b in opp
        if log is not None:
            log.append((('both', 'half_b', 'half_a', 'hit')[(a in own) + 2 * (b in opp)], a, b))
        if a in own and b in opp:
            out['hits'] += 1
        else:
            out['fills'] += (a not in own) + (b not in opp)
            out['half_a'] += a not in own and b in opp
            out['half_b'] += a in own and b not in opp
            own.add(a)
            opp.add(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--moves', type=int, default=14)
    ap.add_argument('--playouts', type=int, default=800)
    ap.add_argument('--board', type=int, default=15)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    import numpy as np
    import torch
    from oracle.evaluators import NetEvaluator
    from oracle.gomoku_ref import RefGomoku
    from oracle.mcts_ref import RefSearch, softmax
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.set_num_threads(1)
    torch.manual_seed(0)
    np.random.seed(0)
    B = args.board
    net, env = PolicyValueNet(B), RefGomoku(B, 5)
    fn = NetEvaluator({k: v.detach().numpy() for k, v in net.state_dict().items()}, B)
    keys = ('leaves', 'depth1', 'depth2', 'deeper', 'far', 'b_seen', 'a_seen', 'hits', 'fills', 'half_a', 'half_b')
    total = dict((k, 0) for k in keys)
    lines = ['memo_probe: board %d x %d, %d playouts a move, %d moves of one game, T = 1, a fresh search per move' % (B, B, args.playouts, args.moves),
             'move ' + ' '.join('%7s' % k for k in keys) + '  distinct_a distinct_b']
    with torch.no_grad():
        for move in range(args.moves):
            search = RefSearch(fn, args.playouts, 5)
            search.leaf_log = []
            for _ in range(args.playouts):
                search.playout(env.clone())
            paths = [p for p, _ in search.leaf_log]
            c = classify(paths, B)
            far = [p for p in paths if len(p) == 2 and cheb(p[0], p[1], B) >= MIN_DIST]
            lines.append('%4d ' % move + ' '.join('%7d' % c[k] for k in keys) + '  %10d %10d' % (len(set(p[0] for p in far)), len(set(p[1] for p in far))))
            for k in keys:
                total[k] += c[k]
            visits = np.array([k.n for k in search.root.kids])
            env.step(int(np.random.choice(search.root.acts, p=softmax(np.log(visits + 1e-10)))))
            if env.game_end_winner()[0]:
                break
    lines.append(' all ' + ' '.join('%7d' % total[k] for k in keys))
    lines.append('share of leaves: far %.1f %%, hits %.1f %%, one window %.1f %%' % (100.0 * total['far'] / total['leaves'], 100.0 * total['hits'] / total['leaves'],
                                                                                  100.0 * (total['half_a'] + total['half_b']) / total['leaves']))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
