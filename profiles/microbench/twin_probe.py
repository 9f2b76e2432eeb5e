"""What a second, foretold window in the one-window passes of k_delta_res<false> would serve, counted on the CPU with the oracle
(step 0 of round 17; the rule is the issue's, restated here so that nothing has to be built to count it).

memo_probe.classify is the memo's rule as the kernel has it (rounds 15 and 16).  ``classify_twin`` replays the same leaves of ONE move
with two additions:

  depth-1 twin   a leaf root + a whose (a, DEPTH1) entry is missing runs its pass; with it runs the window of t, the LOWEST legal cell
                 of the root with no (t, DEPTH1) entry and cheb(t, a) >= 7, and both entries are filled (its own too).  No such t: the
                 pass is today's and fills nothing (the issue's rule: "no candidate means no twin, and the pass is today's").  A depth-1
                 leaf whose entry is there is a HIT.
  filling twin   a far pair root + a + b with b's window served and a's missing (memo_probe's half_a) runs a's window and that of t,
                 the lowest legal cell with no (t, OWN) entry, cheb(t, a) >= 7 and cheb(t, b) >= 7, and fills both OWN entries.

A twin is USED when a later leaf of the move is served from the entry it filled, WASTED otherwise.  The far pair that runs both windows
and the pass around b alone (half_b) get no twin: two windows are the budget (4 changed cells, 8 conv3 tiles).

    python profiles/microbench/twin_probe.py [--moves 14] [--playouts 800] [--board 15] [--out profiles/r17/twin_probe.txt]

CPU only, the same game, net and draws as memo_probe.py; about 2 s per move."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from memo_probe import MIN_DIST, cheb, classify  # noqa: E402


def pick_twin(legal, valid, cols, far_from):
    """the lowest legal cell without an entry that is MIN_DIST or more from every cell of ``far_from``; None when there is none"""
    for t in legal:
        if t not in valid and all(cheb(t, c, cols) >= MIN_DIST for c in far_from):
            return t
    return None


def classify_twin(paths, legal, cols, depth1=True):
    """``paths`` as memo_probe.classify takes them, ``legal`` the root's candidate cells in ascending order (Gomoku: its empty cells, which
    are its legal ones; the kernel takes the empty cells on every board).  ``depth1=False``: the filling twin alone, which is what
    rz_memo.h's twin_cell and k_delta_res build (RZ_DELTA_MEMO=3) -- the depth-1 leaves then run as they do today.  -> dict of counts:
    d1_run / d1_hit (depth-1 leaves that ran a pass / were served), d1_twins, d1_used, d1_wasted, d1_nocand (passes that found no t),
    half_a (filling passes), own_twins, own_used, own_wasted, own_nocand, hits2 (far pairs served whole) and base_hits2 (the same under
    memo_probe.classify: what round 16 serves), new_hits = d1_hit + hits2 - base_hits2, fills (entries written, the twins' among them:
    the kernel's 'memo_fills' with depth1=False)."""
    out = dict(leaves=len(paths), d1_run=0, d1_hit=0, d1_twins=0, d1_used=0, d1_nocand=0, half_a=0, half_b=0, both=0, own_twins=0, own_used=0,
               own_nocand=0, hits2=0, fills=0)
    d1, own, opp = set(), set(), set()
    d1_twin, own_twin = set(), set()      # entries a twin filled and no leaf has been served from yet
    for p in paths:
        if len(p) == 1 and depth1:
            a = p[0]
            if a in d1:
                out['d1_hit'] += 1
                if a in d1_twin:
                    d1_twin.discard(a)
                    out['d1_used'] += 1
                continue
            out['d1_run'] += 1
            t = pick_twin(legal, d1, cols, (a,))
            if t is None:
                out['d1_nocand'] += 1
                continue
            out['d1_twins'] += 1
            d1.update((a, t))
            d1_twin.add(t)
            continue
        if len(p) != 2 or cheb(p[0], p[1], cols) < MIN_DIST:
            continue
        a, b = p
        if a in own and a in own_twin:        # any service of a's entry uses the twin: a hit, or the pass around b alone
            own_twin.discard(a)
            out['own_used'] += 1
        if a in own and b in opp:
            out['hits2'] += 1
            continue
        out['fills'] += (a not in own) + (b not in opp)
        if b in opp:                          # a missing, b served: the filling pass
            out['half_a'] += 1
            t = pick_twin(legal, own, cols, (a, b))
            if t is None:
                out['own_nocand'] += 1
            else:
                out['own_twins'] += 1
                out['fills'] += 1
                own.add(t)
                own_twin.add(t)
        elif a in own:
            out['half_b'] += 1
        else:
            out['both'] += 1
        own.add(a)
        opp.add(b)
    out['d1_wasted'] = len(d1_twin)
    out['own_wasted'] = len(own_twin)
    out['base_hits2'] = classify(paths, cols)['hits']
    out['new_hits'] = out['d1_hit'] + out['hits2'] - out['base_hits2']
    return out


KEYS = ('leaves', 'd1_run', 'd1_hit', 'd1_twins', 'd1_used', 'd1_wasted', 'd1_nocand', 'half_a', 'own_twins', 'own_used', 'own_wasted',
        'own_nocand', 'base_hits2', 'hits2', 'new_hits')


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
    total = dict((k, 0) for k in KEYS)
    lines = ['twin_probe: board %d x %d, %d playouts a move, %d moves of one game, T = 1, a fresh search per move' % (B, B, args.playouts, args.moves),
             'move ' + ' '.join('%10s' % k for k in KEYS) + '   new_hits %']
    with torch.no_grad():
        for move in range(args.moves):
            legal = sorted(int(a) for a in env.leagel_actions())
            search = RefSearch(fn, args.playouts, 5)
            search.leaf_log = []
            for _ in range(args.playouts):
                search.playout(env.clone())
            c = classify_twin([p for p, _ in search.leaf_log], legal, B)
            lines.append('%4d ' % move + ' '.join('%10d' % c[k] for k in KEYS) + '   %9.1f' % (100.0 * c['new_hits'] / c['leaves']))
            for k in KEYS:
                total[k] += c[k]
            visits = np.array([k.n for k in search.root.kids])
            env.step(int(np.random.choice(search.root.acts, p=softmax(np.log(visits + 1e-10)))))
            if env.game_end_winner()[0]:
                break
    lines.append(' all ' + ' '.join('%10d' % total[k] for k in KEYS) + '   %9.1f' % (100.0 * total['new_hits'] / total['leaves']))
    n = float(total['leaves'])
    lines.append('share of leaves: served whole %.1f %% (round 16: %.1f %%), of them depth 1 %.1f %%; leaves that BECOME hits %.1f %%'
                 % (100.0 * (total['d1_hit'] + total['hits2']) / n, 100.0 * total['base_hits2'] / n, 100.0 * total['d1_hit'] / n,
                    100.0 * total['new_hits'] / n))
    lines.append('twins: depth 1 %d run, %d used, %d wasted; OWN %d run, %d used, %d wasted'
                 % (total['d1_twins'], total['d1_used'], total['d1_wasted'], total['own_twins'], total['own_used'], total['own_wasted']))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
