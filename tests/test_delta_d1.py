"""Kind D1 of k_delta_res<false>'s feature memo (rz_memo.h: d1_hit, d1_twin_cell; rz_delta.h: ResHook::d1_twin_of, the twin's stone and
second last cell in pass -1's planes, the hit branch, the fill behind delta_passes): under RZ_DELTA_MEMO=4 -- the default -- a depth-1
leaf root + a that runs its pass also runs the window of a foretold cell t and fills (t, D1), and the later depth-1 leaf root + t is
served without a trunk.  Only which leaves are served changes: the search must build the same trees, bit for bit, as itself under
RZ_DELTA_MEMO=3, under 0 and as the resident full-board kernel; 'memo_d1_hits' and 'memo_d1_twins' (= 'memo_d1_fills') must equal what
profiles/microbench/d1_probe.py's classify_d1 derives from the leaves' paths in evaluation order and the root's empty cells; the far
pairs' counters (words 8 .. 11: memo_hits, memo_fills, memo_half, memo_twins) must equal mode 3's; the tile counters of
tests/test_delta_gather.py must be equal across the routes (a served leaf counts the tiles its pass would have run, a twin pass its own
leaf's tiles); and the D1 counters are 0 under modes 0 .. 3.  64 playouts a search (tests/test_delta_twin.py's way).

Roots, helpers and the leaves' order are tests/test_delta_memo.py's: nearly full 15 x 15 boards of 8 .. 14 empty cells, Connect4 on
11 x 16 (BH != BW), and the EMPTY 15 x 15 board (no stone at the root, no last move: 63 depth-1 leaves in 64 playouts).  The reference
visits a root's children in index order, so on the first set of empty cells -- 0, 1, 14, 15, 112, 210, 223, 224 -- the rule alone gives:
a = 0 takes the corner 14 for its twin, a = 1 takes 112 at distance exactly 7, a = 14 and a = 112 are served, a = 15 takes the corner
210, and a = 223 and a = 224 find no candidate.  The test asserts these from the rule's own log before any comparison.  A REUSED tree: a
move is played with its subtree kept and the next search runs on it; the order of ITS leaves is reconstructed the same way and the
counters are held to the rule on the new root's empty cells (test_a_reused_tree)."""
import importlib.util
import os

import numpy as np
import pytest

import test_delta_gather as tdg
import test_delta_memo as tdm
from conftest import REPO

pytestmark = pytest.mark.gpu

SIMS = 64
MEMO = ('memo_hits', 'memo_fills', 'memo_half', 'memo_twins')
D1 = ('memo_d1_hits', 'memo_d1_twins', 'memo_d1_fills')


@pytest.fixture(autouse=True)
def _sixty_four_playouts(monkeypatch):
    monkeypatch.setattr(tdm, 'SIMS', SIMS)


def _d1_probe():
    spec = importlib.util.spec_from_file_location('d1_probe', os.path.join(REPO, 'profiles', 'microbench', 'd1_probe.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mode(mode):
    def then(evaluator, eng, once):
        os.environ['RZ_DELTA_MEMO'] = mode   # (read when the first search reserves the cache; tdm._search puts the variable back)
        return once()
    return then


def _root_empties(roots, S):
    from rlzero_amd.engine import bits_to_int
    out = []
    for st in roots[0]:
        occ = bits_to_int(st[0]) | bits_to_int(st[1])
        out.append([c for c in range(S) if not (occ >> c) & 1])
    return out


def _expected(probe, leaves, empties, cols, log=None):
    tot = dict(depth1=0, d1_run=0, d1_hit=0, d1_twins=0, d1_used=0, d1_wasted=0, d1_nocand=0)
    for g, seq in enumerate(leaves):
        one = [] if log is not None else None
        c = probe.classify_d1(seq[:SIMS], empties[g], cols, log=one)
        if log is not None:
            log.append(one)
        for k in tot:
            tot[k] += c[k]
    return tot


def _routes_agree(net, B, roots, want):
    t4, s4 = tdm._search(net, B, roots, then=_mode('4'))
    t3, s3 = tdm._search(net, B, roots, then=_mode('3'))
    t0, s0 = tdm._search(net, B, roots, memo=False)
    tf, _ = tdm._search(net, B, roots, delta=False)
    print(B, want, s4, s3)
    assert t4 == t3 and t4 == t0 and t4 == tf
    assert (s4['memo_d1_hits'], s4['memo_d1_twins'], s4['memo_d1_fills']) == (want['d1_hit'], want['d1_twins'], want['d1_twins']), (s4, want)
    assert [s4[k] for k in MEMO] == [s3[k] for k in MEMO], (s4, s3)
    assert [s3[k] for k in D1] == [0, 0, 0] and [s0[k] for k in D1] == [0, 0, 0]
    for k in tdg.STATS:
        assert s4[k] == s3[k] == s0[k], (k, s4, s3, s0)
    return s4


def test_trees_and_counters_on_nearly_full_boards_and_the_modes_below():
    probe = _d1_probe()
    B = 15
    S = B * B
    net = tdg._net(B, 450 + B)
    roots = tdg._roots(B, tdm._empties(B))
    empties = _root_empties(roots, S)
    leaves = tdm._ordered_leaves(net, B, roots)
    log = []
    want = _expected(probe, leaves, empties, B, log)
    # the input conditions, from the rule's own log (kind, a, t) of every depth-1 leaf
    first = log[0]
    assert [a for _, a, _ in first][:len(empties[0])] == empties[0], first                  # the children come in index order
    assert ('twin', 0, B - 1) in first and ('twin', B, S - B) in first                       # twins in corners
    assert ('twin', 1, (B // 2) * B + B // 2) in first and probe.cheb(1, (B // 2) * B + B // 2, B) == 7   # a twin at distance exactly 7
    assert ('hit', B - 1, None) in first and ('hit', S - B, None) in first                   # twins later served
    assert ('nocand', S - 2, None) in first and ('nocand', S - 1, None) in first             # passes without a candidate
    assert want['d1_hit'] > 0 and want['d1_used'] == want['d1_hit'] and want['d1_nocand'] > 0, want
    _routes_agree(net, B, roots, want)
    # modes 1 and 2 count nothing of the kind either
    for mode in ('1', '2'):
        _, s = tdm._search(net, B, roots, then=_mode(mode))
        assert [s[k] for k in D1] == [0, 0, 0], (mode, s)


def test_the_empty_board():
    """No stone at the root (nst == 0), no last move: the changed cell of a depth-1 leaf is its one stone; 63 depth-1 leaves, whose twins
    lie 7 columns to the right while the row lasts."""
    probe = _d1_probe()
    B = 15
    net = tdg._net(B, 471)
    roots = (np.zeros((1, 2, 4), dtype=np.uint64), [0], [-1])
    empties = _root_empties(roots, B * B)
    assert len(empties[0]) == B * B
    leaves = tdm._ordered_leaves(net, B, roots)
    log = []
    want = _expected(probe, leaves, empties, B, log)
    assert want['depth1'] == SIMS - 1 and log[0][0] == ('twin', 0, 7) and ('hit', 7, None) in log[0], log[0][:9]
    assert want['d1_hit'] > 0 and want['d1_wasted'] > 0, want            # (a search cut at 64 playouts leaves twins that no leaf came to use)
    _routes_agree(net, B, roots, want)


def test_a_rectangular_board_11x16():
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    probe = _d1_probe()
    B = (tdm.C4_ROWS, tdm.C4_COLS)
    torch.manual_seed(491)
    net = PolicyValueNet(tdm.C4_ROWS, tdm.C4_COLS, tdm.C4_COLS)
    roots = tdm._c4_roots(8)
    leaves = tdm._ordered_leaves(net, B, roots)
    empties = _root_empties(roots, tdm.C4_ROWS * tdm.C4_COLS)
    want = _expected(probe, leaves, empties, tdm.C4_COLS)
    print(want)
    assert want['d1_twins'] > 0, want
    _routes_agree(net, B, roots, want)


FIRST = 16   # playouts of the search BEFORE the move of test_a_reused_tree


def _second_search(mode, second_counts=None):
    """tdm._search's `then`: the first search (tdm._search's `counts`: FIRST playouts a game), the most visited move played with its subtree
    kept (advance + step), then the search the test is about, of SIMS playouts a game or of `second_counts`.
    -> (its trees, its counters, the kept trees, the moves)"""
    def then(evaluator, eng, once):
        if mode is not None:
            os.environ['RZ_DELTA_MEMO'] = mode
        once()
        moves = np.array([int(np.argmax(v)) for v in eng.root_visits()], dtype=np.int32)
        eng.advance(moves)
        _, ended = eng.step(moves)
        assert not np.asarray(ended).any()
        kept = [eng.tree_dump(g) for g in range(len(moves))]
        eng.set_playouts(None if second_counts is None else np.asarray(second_counts, dtype=np.int32))
        evaluator.hip.delta_stats(reset=True)
        eng.simulate(evaluator, SIMS, use_graph=False)
        eng.check()
        return [eng.tree_dump(g) for g in range(len(moves))], evaluator.hip.delta_stats(), kept, [int(m) for m in moves]
    return then


def test_a_reused_tree():
    """A search of FIRST playouts, the most visited move played with its subtree kept, then the search this test is about, on a root that
    has children already.  Its leaves' order is reconstructed as tests/test_delta_memo.py reconstructs a fresh search's: every root at
    every count 1 .. SIMS of the SECOND search in one launch of the kernel without the memo, the leaf of simulation k being the deepest
    node whose visits grew from count k - 1 to k (count 0: the kept subtree).  FIRST is small, so the move's node has had one or two
    visits and most of its children are still to come, in index order, as depth-1 leaves: the rule must give twins AND served leaves
    there (asserted from the rule alone), and 'memo_d1_hits' / 'memo_d1_twins' must equal classify_d1 on the new root's empty cells --
    with the twin chosen among all far cells instead of those above a they would not: the cells below a that the kept tree holds
    already never come again.  The trees as under modes 3 and 0 and the full-board kernel, the far pairs' counters and the tile
    counters as under mode 3."""
    probe = _d1_probe()
    B = 15
    net = tdg._net(B, 492)
    roots = tdg._roots(B, tdm._empties(B))
    G = len(roots[0])
    # the order: G x SIMS games, replica k of root g stops its second search after k + 1 playouts
    rep = (np.repeat(roots[0], SIMS, axis=0), list(np.repeat(roots[1], SIMS)), list(np.repeat(roots[2], SIMS)))
    trees, _, kept_rep, moves_rep = tdm._search(net, B, rep, counts=[FIRST] * (G * SIMS), memo=False,
                                                then=_second_search(None, np.tile(np.arange(1, SIMS + 1), G)))
    leaves, moves, kept = [], [], []
    for g in range(G):
        assert len(set(moves_rep[g * SIMS:(g + 1) * SIMS])) == 1 and all(t == kept_rep[g * SIMS] for t in kept_rep[g * SIMS:(g + 1) * SIMS])
        moves.append(moves_rep[g * SIMS])
        kept.append(kept_rep[g * SIMS])
        seq, before = [], kept[g]
        for k in range(SIMS):
            tree = trees[g * SIMS + k]
            assert tree[()][0] == kept[g][()][0] + k + 1
            grown = [p for p, (n, _) in tree.items() if n > before.get(p, (0, 0.0))[0]]
            seq.append(max(grown, key=len))
            assert sorted(grown, key=len) == [seq[-1][:i] for i in range(len(seq[-1]) + 1)]   # one path grew
            before = tree
        leaves.append(seq)
    empties = [[c for c in e if c != moves[g]] for g, e in enumerate(_root_empties(roots, B * B))]
    log = []
    want = _expected(probe, leaves, empties, B, log)
    r1 = sum(probe.classify_d1(seq, empties[g], B, rule='R1')['d1_hit'] for g, seq in enumerate(leaves))
    print(want, r1, [t[()][0] for t in kept])
    assert min(t[()][0] for t in kept) > 1 and all(len(t) > 1 for t in kept)   # every game's tree was carried: its root has children already
    assert want['d1_twins'] > 0 and want['d1_hit'] > 0 and want['d1_nocand'] > 0, want
    assert r1 != want['d1_hit'], (r1, want)                       # these inputs tell the kept rule from the one without "above a"
    first = [FIRST] * G
    t4, s4, k4, m4 = tdm._search(net, B, roots, counts=first, then=_second_search('4'))
    t3, s3, _, _ = tdm._search(net, B, roots, counts=first, then=_second_search('3'))
    t0, s0, _, _ = tdm._search(net, B, roots, counts=first, memo=False, then=_second_search(None))
    tf, _, _, _ = tdm._search(net, B, roots, counts=first, delta=False, then=_second_search(None))
    print(s4, s3)
    assert m4 == moves and k4 == kept
    assert t4 == t3 and t4 == t0 and t4 == tf
    assert t4 == [trees[g * SIMS + SIMS - 1] for g in range(G)]
    assert (s4['memo_d1_hits'], s4['memo_d1_twins'], s4['memo_d1_fills']) == (want['d1_hit'], want['d1_twins'], want['d1_twins']), (s4, want)
    assert [s4[k] for k in MEMO] == [s3[k] for k in MEMO] and [s3[k] for k in D1] == [0, 0, 0] and [s0[k] for k in D1] == [0, 0, 0]
    for k in tdg.STATS:
        assert s4[k] == s3[k] == s0[k], (k, s4, s3, s0)
