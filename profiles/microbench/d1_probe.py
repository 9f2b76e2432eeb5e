"""What a foretold twin window in the depth-1 passes of k_delta_res<false> would serve when the tree is KEPT across moves, counted on the
CPU with the oracle (step 0 of round 18).

twin_probe.py counted the depth-1 twin with a fresh search per move.  The timed search reuses its tree: the new root is a child of the
old one, its lower children were expanded by earlier searches, and "the lowest cell without an entry" may then be a cell that never
comes as a leaf again.  This probe replays the same 14 moves with RefSearch.update_with_move and counts two rules for the twin t of a
depth-1 leaf root + a that runs its pass:

  R1   the lowest cell empty at the root with no (t, D1) entry and cheb(t, a) >= 7
  R2   the same, restricted to t > a (the reference visits a node's unvisited children in index order, so a cell below a has been a leaf)

``classify_d1`` is the rule as rz_memo.h and the kernel have it (d1_hit, d1_twin_cell): a depth-1 leaf whose (a, D1) entry is there is a
HIT and runs no window; otherwise it runs its pass, and with it the window of t, and (t, D1) alone is filled -- a depth-1 leaf is
evaluated once a search, so its own window is never stored.  tests/test_delta_d1.py holds the kernel's counters to this function.

    python profiles/microbench/d1_probe.py [--moves 14] [--playouts 800] [--board 15] [--out profiles/r18/d1_probe.txt]

CPU only, the same game, net and draws as memo_probe.py and twin_probe.py."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from memo_probe import MIN_DIST, cheb  # noqa: E402

RULE = 'R2'   # the rule step 0 kept (profiles/r18/d1_probe.txt): rz_memo.h's d1_twin_cell


def pick_d1_twin(legal, valid, cols, a, rule=RULE):
    """the lowest cell of ``legal`` (ascending) with no entry that is MIN_DIST or more from a -- and above a under R2; None: no candidate"""
    for t in legal:
        if t not in valid and (rule == 'R1' or t > a) and cheb(t, a, cols) >= MIN_DIST:
            return t
    return None


def classify_d1(paths, legal, cols, rule=RULE, log=None):
    """``paths``: the leaves of one move in evaluation order, each a tuple of cells from the root; ``legal``: the root's empty cells in
    ascending order.  -> dict of counts: leaves, depth1, d1_run (depth-1 leaves that ran a pass), d1_hit (served), d1_twins (passes that ran a
    twin: the kernel's 'memo_d1_twins' and 'memo_d1_fills'), d1_used (twins a later leaf was served from), d1_wasted, d1_nocand.  ``log``: a
    list that receives (kind, a, t) of every depth-1 leaf in order, kind one of 'hit' (t None), 'twin', 'nocand' (t None)."""
    out = dict(leaves=len(paths), depth1=0, d1_run=0, d1_hit=0, d1_twins=0, d1_used=0, d1_nocand=0)
    d1, unused = set(), set()
    for p in paths:
        if len(p) != 1:
            continue
        a = p[0]
        out['depth1'] += 1
        if a in d1:
            out['d1_hit'] += 1
            if a in unused:
                unused.discard(a)
                out['d1_used'] += 1
            if log is not None:
                log.append(('hit', a, None))
            continue
        out['d1_run'] += 1
        t = pick_d1_twin(legal, d1, cols, a, rule)
        if log is not None:
            log.append(('nocand' if t is None else 'twin', a, t))
        if t is None:
            out['d1_nocand'] += 1
            continue
        out['d1_twins'] += 1
        d1.add(t)
        unused.add(t)
    out['d1_wasted'] = len(unused)
    return out


KEYS = ('leaves', 'depth1', 'd1_run', 'd1_hit', 'd1_twins', 'd1_used', 'd1_wasted', 'd1_nocand')


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
    rules = ('R1', 'R2')
    total = dict((r, dict((k, 0) for k in KEYS)) for r in rules)
    in_order = True
    lines = ['d1_probe: board %d x %d, %d playouts a move, %d moves of one game, T = 1, the tree KEPT across moves' % (B, B, args.playouts, args.moves),
             'move rule ' + ' '.join('%9s' % k for k in KEYS) + '   served %']
    search = RefSearch(fn, args.playouts, 5)
    with torch.no_grad():
        for move in range(args.moves):
            legal = sorted(int(a) for a in env.leagel_actions())
            search.leaf_log = []
            for _ in range(args.playouts):
                search.playout(env.clone())
            paths = [p for p, _ in search.leaf_log]
            firsts = [p[0] for p in paths if len(p) == 1]
            in_order = in_order and firsts == sorted(firsts)
            for r in rules:
                c = classify_d1(paths, legal, B, r)
                lines.append('%4d %4s ' % (move, r) + ' '.join('%9d' % c[k] for k in KEYS) + '   %8.1f' % (100.0 * c['d1_hit'] / c['leaves']))
                for k in KEYS:
                    total[r][k] += c[k]
            visits = np.array([k.n for k in search.root.kids])
            a = int(np.random.choice(search.root.acts, p=softmax(np.log(visits + 1e-10))))
            env.step(a)
            search.update_with_move(a)
            if env.game_end_winner()[0]:
                break
    for r in rules:
        t = total[r]
        lines.append(' all %4s ' % r + ' '.join('%9d' % t[k] for k in KEYS) + '   %8.1f' % (100.0 * t['d1_hit'] / t['leaves']))
    lines.append("the depth-1 leaves of every move came in ascending cell order: %s" % ('yes' if in_order else 'NO'))
    for r in rules:
        t = total[r]
        lines.append('%s: depth-1 leaves %.1f %% of all, served %.1f %% of all; twins %d run, %d used, %d wasted (%.1f %%), %d passes without a candidate'
                     % (r, 100.0 * t['depth1'] / t['leaves'], 100.0 * t['d1_hit'] / t['leaves'], t['d1_twins'], t['d1_used'], t['d1_wasted'],
                        100.0 * t['d1_wasted'] / max(1, t['d1_twins']), t['d1_nocand']))
    keep = min(rules, key=lambda r: (total[r]['d1_wasted'], r != 'R2'))
    t = total[keep]
    go = 100.0 * t['d1_hit'] >= 10.0 * t['leaves'] and 100.0 * t['d1_wasted'] < 5.0 * max(1, t['d1_twins'])
    lines.append('kept rule: %s (fewer wasted twins); gate (serves >= 10 %% of leaves, wastes < 5 %% of its twins): %s' % (keep, 'GO' if go else 'STOP'))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
