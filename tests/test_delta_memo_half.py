"""The one-window route of k_delta_res<false>'s feature memo (rz_memo.h: served; rz_delta.h: ResHook::memo_word's serve bits, the
dropped rows of ResHook::leaf, the patch behind delta_passes in the simulation loop): a leaf root + a + b, the stones 7 or more apart,
with exactly ONE of its two entries in the memo runs its passes over the missing stone's window alone and takes the other stone's
7 x 7 of value features from the entry.  Only where the bits come from changes: the search must build the same trees, bit for bit, as
itself with RZ_DELTA_MEMO=2 (the memo without this route), with RZ_DELTA_MEMO=0, as the resident full-board kernel and as the
two-launch step; 'memo_half' must equal what profiles/microbench/memo_probe.py's classify counts as half_a + half_b from the leaves'
paths in evaluation order, 'memo_hits' / 'memo_fills' its hits / fills, and the counters of tests/test_delta_gather.py (a one-window
leaf reports the tiles of the two-window pass) must be equal across the routes.

The helpers, the roots and the leaves' order are tests/test_delta_memo.py's (nearly full boards of 8 .. 14 empty cells; Connect4 on
11 x 16 for the rectangle).  Under the reference's rule a's k-th visit at depth 2 meets the k-th empty cell in index order, so with the
corner cell 0 empty almost every a far from it meets b = 0 first -- the first such leaf fills both entries, the later ones are served
b's window, clipped by the corner, and run a's (half_a) -- and its second reply is new when the first two empty cells are neighbours
(half_b); the set with cells 7, 7 B and 7 B + 7 empty puts three such a at distance exactly 7 from cell 0.  Whether the roots do all
of that is asserted from classify's log alone, before any comparison.  (The roots were not run through oracle/mcts_ref.py beforehand:
the order of a's second visits depends on the net's values, and the assertions below read it from the search itself.)"""
import os

import pytest

import test_delta_gather as tdg
import test_delta_memo as tdm

pytestmark = pytest.mark.gpu

SIMS = tdm.SIMS


def _classified(probe, leaves, cols, counts=None):
    """-> (hits, fills, half_a, half_b, the far leaves' log) over the games, each game's first counts[g] leaves"""
    tot, log = [0, 0, 0, 0], []
    for g, seq in enumerate(leaves):
        c = probe.classify(seq[:SIMS if counts is None else counts[g]], cols, log=log)
        for i, k in enumerate(('hits', 'fills', 'half_a', 'half_b')):
            tot[i] += c[k]
    return tot[0], tot[1], tot[2], tot[3], log


def _inputs_do_what_the_test_is_about(probe, log, rows, cols):
    halves = [(kind, a, b) for kind, a, b in log if kind in ('half_a', 'half_b')]
    assert any(k == 'half_a' for k, _, _ in halves) and any(k == 'half_b' for k, _, _ in halves), log
    assert any(probe.cheb(a, b, cols) == 7 for _, a, b in halves), halves                      # the windows' closest approach

    def cornered(c):   # within 3 of two edges: the 7 x 7 window is clipped in both directions
        y, x = divmod(c, cols)
        return (y < 3 or y >= rows - 3) and (x < 3 or x >= cols - 3)
    assert any(cornered(b if kind == 'half_a' else a) for kind, a, b in halves), halves        # a SERVED window clipped by a corner
    assert any(kind == 'hit' for kind, _, _ in log) and any(kind == 'both' for kind, _, _ in log)


def _without_the_route(evaluator, eng, once):
    os.environ['RZ_DELTA_MEMO'] = '2'   # (read when the first search reserves the cache; tdm._search puts the variable back)
    return once()


def _routes_agree(probe, net, B, roots, leaves, rows, cols):
    hits, fills, half_a, half_b, log = _classified(probe, leaves, cols)
    _inputs_do_what_the_test_is_about(probe, log, rows, cols)
    t_half, s_half = tdm._search(net, B, roots)
    t_m2, s_m2 = tdm._search(net, B, roots, then=_without_the_route)
    t_off, s_off = tdm._search(net, B, roots, memo=False)
    t_full, _ = tdm._search(net, B, roots, delta=False)
    t_two, s_two = tdm._search(net, B, roots, resident=False)
    print(B, s_half, s_m2, (hits, fills, half_a, half_b))
    assert t_half == t_m2 and t_half == t_off and t_half == t_full and t_half == t_two
    assert s_half['memo_half'] == half_a + half_b, (s_half, half_a, half_b)
    assert (s_half['memo_hits'], s_half['memo_fills']) == (hits, fills), (s_half, hits, fills)
    assert (s_m2['memo_hits'], s_m2['memo_fills'], s_m2['memo_half']) == (hits, fills, 0), (s_m2, hits, fills)
    assert (s_off['memo_hits'], s_off['memo_fills'], s_off['memo_half']) == (0, 0, 0) and s_two['memo_half'] == 0
    for k in tdg.STATS:   # a one-window leaf counts the tiles of the two-window pass, and its two changed cells
        assert s_half[k] == s_m2[k] == s_off[k] == s_two[k], (k, s_half, s_m2, s_off, s_two)


@pytest.mark.parametrize('B', [15, 11, 16])
def test_trees_and_counters_across_the_routes(B):
    probe = tdm._probe()
    net = tdg._net(B, 250 + B)
    empties = tdm._empties(B)
    roots = tdg._roots(B, empties)
    leaves = tdm._ordered_leaves(net, B, roots)
    _routes_agree(probe, net, B, roots, leaves, B, B)
    # per-game counts of 1, 2 and 31: a game's memo ends with its search
    counts = [(1, 2, 31, SIMS)[g % 4] for g in range(len(empties))]
    hits, fills, half_a, half_b, _ = _classified(probe, leaves, B, counts)
    t_c, s_c = tdm._search(net, B, roots, counts=counts)
    t_cf, _ = tdm._search(net, B, roots, counts=counts, delta=False)
    assert t_c == t_cf
    assert (s_c['memo_hits'], s_c['memo_fills'], s_c['memo_half']) == (hits, fills, half_a + half_b), (s_c, hits, fills, half_a, half_b)


def test_a_rectangular_board_11x16():
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    probe = tdm._probe()
    B = (tdm.C4_ROWS, tdm.C4_COLS)
    torch.manual_seed(291)
    net = PolicyValueNet(tdm.C4_ROWS, tdm.C4_COLS, tdm.C4_COLS)
    roots = tdm._c4_roots(8)
    leaves = tdm._ordered_leaves(net, B, roots)
    _routes_agree(probe, net, B, roots, leaves, tdm.C4_ROWS, tdm.C4_COLS)


def test_a_new_search_and_a_weight_reload_start_from_cleared_bits():
    """As tests/test_delta_memo.py's test of the same name, with the one-window leaves counted: a second search of the same roots
    begins with cleared bits (it serves nothing of the first), and behind a weight reload nothing of the old entries is served."""
    B = 15
    net, net2 = tdg._net(B, 281), tdg._net(B, 282)
    roots = tdg._roots(B, tdm._empties(B))

    def twice(evaluator, eng, once):
        first = once()
        second = once()
        evaluator.hip.load_state_dict(net2.state_dict())
        third = once()
        return first, second, third
    first, second, third = tdm._search(net, B, roots, then=twice)
    fresh = tdm._search(net2, B, roots)
    keys = ('memo_hits', 'memo_fills', 'memo_half')
    assert first[1]['memo_half'] > 0
    assert second[0] == first[0] and [second[1][k] for k in keys] == [first[1][k] for k in keys]
    assert third[0] == fresh[0] and third[0] != first[0]
    assert [third[1][k] for k in keys] == [fresh[1][k] for k in keys]
