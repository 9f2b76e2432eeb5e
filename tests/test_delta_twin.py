"""The twin window of k_delta_res<false>'s feature memo (rz_memo.h: twin_cell; rz_delta.h: ResHook::twin_of, the stone wave 0 adds to
pass -1's planes, the fill behind delta_passes): under RZ_DELTA_MEMO=3 -- the default -- the pass that runs a's window alone also runs
the window of a foretold cell t and fills (t, OWN).  Only which leaves are served changes: the search must build the same trees, bit
for bit, as itself with RZ_DELTA_MEMO=1 (no twins), with RZ_DELTA_MEMO=0 and as the resident full-board kernel; 'memo_hits',
'memo_fills' and 'memo_half' must equal what profiles/microbench/twin_probe.py's classify_twin(depth1=False) derives from the leaves'
paths in evaluation order and the root's empty cells (a twin's entry counts among the fills), 'memo_twins' its own_twins; and the tile
counters of tests/test_delta_gather.py must be equal across the routes (a twin pass counts its own leaf's tiles).  64 playouts a
search: the helpers of tests/test_delta_memo.py run `tdm.SIMS` of them, which a fixture sets for this module and puts back.

Roots, helpers and the leaves' order are tests/test_delta_memo.py's: nearly full boards of 8 .. 14 empty cells on 15 x 15, Connect4 on
11 x 16.  With so few empty cells the roots cover, and the test asserts from the rule's own log before any comparison: passes without a
candidate, twins in a corner and on an edge, twins that are used later and (in the searches cut short) twins that never are,
per-game counts of 1 and 2.  A REUSED tree (test_a_reused_tree...): a move is played with its subtree kept and the next search runs
on it -- many of the new root's grandchildren exist already, so a twin's cell may never come as a leaf again.  The order of that
search's leaves is not reconstructed; the trees are compared across the routes, and the twins that were never used are counted by an
identity of the rule: every far leaf with first cell t fills (t, OWN) where no twin has, so the entries filled with twins exceed those
filled without by exactly the twins whose cell never came."""
import importlib.util
import os

import pytest

import test_delta_gather as tdg
import test_delta_memo as tdm
from conftest import REPO

pytestmark = pytest.mark.gpu

SIMS = 64


@pytest.fixture(autouse=True)
def _sixty_four_playouts(monkeypatch):
    monkeypatch.setattr(tdm, 'SIMS', SIMS)


def _twin_probe():
    spec = importlib.util.spec_from_file_location('twin_probe', os.path.join(REPO, 'profiles', 'microbench', 'twin_probe.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _root_empties(roots, S):
    from rlzero_amd.engine import bits_to_int
    out = []
    for st in roots[0]:
        occ = bits_to_int(st[0]) | bits_to_int(st[1])
        out.append([c for c in range(S) if not (occ >> c) & 1])
    return out


def _expected(probe, leaves, empties, cols, counts=None):
    tot = dict(hits2=0, fills=0, half_a=0, half_b=0, own_twins=0, own_used=0, own_wasted=0, own_nocand=0, base_hits2=0)
    for g, seq in enumerate(leaves):
        c = probe.classify_twin(seq[:SIMS if counts is None else counts[g]], empties[g], cols, depth1=False)
        for k in tot:
            tot[k] += c[k]
    return tot


def _with_twins(evaluator, eng, once):
    os.environ['RZ_DELTA_MEMO'] = '3'   # (read when the first search reserves the cache; tdm._search puts the variable back)
    return once()


def _memo(st):
    return st['memo_hits'], st['memo_fills'], st['memo_half'], st['memo_twins']


def _rule(want):
    return want['hits2'], want['fills'], want['half_a'] + want['half_b'], want['own_twins']


def _routes_agree(probe, net, B, roots, leaves, rows, cols):
    empties = _root_empties(roots, rows * cols)
    want = _expected(probe, leaves, empties, cols)
    print(B, want)
    assert want['own_twins'] > 0 and want['own_used'] > 0 and want['own_nocand'] > 0, want
    assert want['hits2'] > want['base_hits2']                       # the twins serve leaves the memo alone does not
    t_twin, s_twin = tdm._search(net, B, roots, then=_with_twins)
    t_one, s_one = tdm._search(net, B, roots)
    t_off, s_off = tdm._search(net, B, roots, memo=False)
    t_full, _ = tdm._search(net, B, roots, delta=False)
    print(s_twin, s_one)
    assert t_twin == t_one and t_twin == t_off and t_twin == t_full
    assert _memo(s_twin) == _rule(want), (s_twin, want)
    assert s_one['memo_hits'] == want['base_hits2'] and s_one['memo_twins'] == 0 and _memo(s_off) == (0, 0, 0, 0)
    for k in tdg.STATS:
        assert s_twin[k] == s_one[k] == s_off[k], (k, s_twin, s_one, s_off)
    return empties


@pytest.mark.parametrize('B', [15])
def test_trees_and_counters_with_twins(B):
    probe = _twin_probe()
    net = tdg._net(B, 350 + B)
    roots = tdg._roots(B, tdm._empties(B))
    leaves = tdm._ordered_leaves(net, B, roots)
    empties = _routes_agree(probe, net, B, roots, leaves, B, B)
    # twins in a corner and on an edge, from the rule's own choices
    S = B * B
    picked = set()
    for g, seq in enumerate(leaves):
        own, opp = set(), set()
        for p in seq:
            if len(p) == 2 and probe.cheb(p[0], p[1], B) >= 7:
                a, b = p
                if a not in own and b in opp:
                    t = probe.pick_twin(empties[g], own, B, (a, b))
                    if t is not None:
                        picked.add(t)
                        own.add(t)
                own.add(a)
                opp.add(b)
    assert picked & {0, B - 1, S - B, S - 1}, picked
    assert any(t // B in (0, B - 1) or t % B in (0, B - 1) for t in picked - {0, B - 1, S - B, S - 1}), picked
    # per-game counts of 1 and 2, and a search that ends with the pass that ran its first twin (that twin is never used): a game's
    # memo ends with its search
    def first_twin(g):
        for k in range(1, SIMS + 1):
            if probe.classify_twin(leaves[g][:k], empties[g], B, depth1=False)['own_twins']:
                return k
        return 31
    counts = [1, 2] + [first_twin(g) for g in range(2, len(empties) - 1)] + [SIMS]
    want = _expected(probe, leaves, empties, B, counts)
    print(counts, want)
    assert want['own_wasted'] > 0, want                             # a search that ends before a twin's cell is visited: never used
    t_c, s_c = tdm._search(net, B, roots, counts=counts, then=_with_twins)
    t_cf, _ = tdm._search(net, B, roots, counts=counts, delta=False)
    assert t_c == t_cf
    assert _memo(s_c) == _rule(want), (s_c, want)


def test_a_rectangular_board_11x16():
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    probe = _twin_probe()
    B = (tdm.C4_ROWS, tdm.C4_COLS)
    torch.manual_seed(291)
    net = PolicyValueNet(tdm.C4_ROWS, tdm.C4_COLS, tdm.C4_COLS)
    roots = tdm._c4_roots(8)
    leaves = tdm._ordered_leaves(net, B, roots)
    empties = _root_empties(roots, tdm.C4_ROWS * tdm.C4_COLS)
    want = _expected(probe, leaves, empties, tdm.C4_COLS)
    print(want)
    assert want['own_twins'] > 0 and want['own_used'] > 0 and want['hits2'] > want['base_hits2'], want   # a twin's entry is served here too
    assert want['own_wasted'] > 0, want                              # ... and, in a full search, some twins are never used
    t_twin, s_twin = tdm._search(net, B, roots, then=_with_twins)
    t_one, s_one = tdm._search(net, B, roots)
    t_off, s_off = tdm._search(net, B, roots, memo=False)
    t_full, _ = tdm._search(net, B, roots, delta=False)
    assert t_twin == t_one and t_twin == t_off and t_twin == t_full
    assert s_one['memo_hits'] == want['base_hits2'] and _memo(s_off) == (0, 0, 0, 0)
    assert _memo(s_twin) == _rule(want), (s_twin, want)
    for k in tdg.STATS:
        assert s_twin[k] == s_one[k] == s_off[k], (k, s_twin, s_one, s_off)


def test_a_new_search_and_a_weight_reload_start_from_cleared_bits():
    """A second search of the same roots begins with cleared bits -- it serves nothing the first one's twins left --, and behind a
    weight reload no twin's entry of the old weights is served."""
    B = 15
    net, net2 = tdg._net(B, 381), tdg._net(B, 382)
    roots = tdg._roots(B, tdm._empties(B))

    def twice(evaluator, eng, once):
        os.environ['RZ_DELTA_MEMO'] = '3'
        first = once()
        second = once()
        evaluator.hip.load_state_dict(net2.state_dict())
        third = once()
        return first, second, third
    first, second, third = tdm._search(net, B, roots, then=twice)
    fresh = tdm._search(net2, B, roots, then=_with_twins)
    plain = tdm._search(net, B, roots)
    # (a used twin's entry replaces the fill of its cell's own pass: the fills may be equal, the served leaves are more)
    assert first[1]['memo_hits'] > plain[1]['memo_hits'] and first[0] == plain[0]        # twins ran and were used, the trees are the same
    assert second[0] == first[0] and _memo(second[1]) == _memo(first[1])
    assert third[0] == fresh[0] and third[0] != first[0] and _memo(third[1]) == _memo(fresh[1])


def test_a_reused_tree_whose_children_exist_already():
    """A search, the most visited move played with its subtree kept (advance + step), then the search this test is about: the same
    trees under modes 3, 1 and 0 and the full-board kernel; twins run, and the never-used ones are bounded by the module docstring's identity."""
    import numpy as np
    B = 15
    net = tdg._net(B, 391)
    roots = tdg._roots(B, tdm._empties(B))

    def second_move(mode):
        def then(evaluator, eng, once):
            if mode is not None:
                os.environ['RZ_DELTA_MEMO'] = mode
            once()
            moves = np.array([int(np.argmax(v)) for v in eng.root_visits()], dtype=np.int32)
            eng.advance(moves)
            _, ended = eng.step(moves)
            assert not np.asarray(ended).any()
            kept = [eng.tree_dump(g)[()][0] for g in range(len(moves))]
            evaluator.hip.delta_stats(reset=True)
            eng.simulate(evaluator, SIMS, use_graph=False)
            eng.check()
            return [eng.tree_dump(g) for g in range(len(moves))], evaluator.hip.delta_stats(), kept
        return then
    t3, s3, kept = tdm._search(net, B, roots, then=second_move('3'))
    t1, s1, _ = tdm._search(net, B, roots, then=second_move(None))
    t0, s0, _ = tdm._search(net, B, roots, memo=False, then=second_move(None))
    tf, _, _ = tdm._search(net, B, roots, delta=False, then=second_move(None))
    print(kept, s3, s1)
    assert min(kept) > 1                                        # every game's tree was carried: its root has children already
    assert t3 == t1 and t3 == t0 and t3 == tf
    assert s3['memo_twins'] > 0 and s1['memo_twins'] == 0 and _memo(s0) == (0, 0, 0, 0)
    wasted = s3['memo_fills'] - s1['memo_fills']
    # (the twins that were never used, no more of them than ran.  On these roots every twin of the reused tree is used -- the
    # difference is 0 --; a full search with never-used twins is the 11 x 16 case, the searches cut short are the other)
    assert 0 <= wasted <= s3['memo_twins'], (s3, s1)
    assert s3['memo_hits'] >= s1['memo_hits']
    for k in tdg.STATS:
        assert s3[k] == s1[k] == s0[k], (k, s3, s1, s0)
