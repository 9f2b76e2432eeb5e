"""The feature memo of k_delta_res<false> (rz_memo.h; rz_delta.h: ResHook::memo_word, the hit branch and the fill of the simulation
loop): a leaf root + a + b whose stones are 7 or more cells apart, and whose two 7 x 7 windows of value features an earlier leaf of the
move has left in the game's memo, takes them and the base's planes instead of running the trunk.  Only where the bits come from
changes: the search must build the same trees, bit for bit, as the resident full-board kernel, as the two-launch step and as itself
with RZ_DELTA_MEMO=0, and its counters memo_hits / memo_fills must equal what profiles/microbench/memo_probe.py's classify derives on
the host from the leaves' paths in the order the search evaluated them.

The order: a game with k simulations ends with the tree of the first k simulations of a longer search (set_playouts), so ONE launch of
every root at every count 1 .. SIMS gives the leaf of simulation k as the deepest node whose visit count grew from count k - 1 to k.

Roots (tests/test_delta_gather.py's nearly full boards): 8 .. 14 empty cells -- the four corners (windows clipped twice), pairs
exactly 6 and exactly 7 apart, neighbours (overlapping windows), cells on both sides of the 64-cell word boundaries -- so that within
48 simulations the depth-2 leaves repeat their a and their b; a root where the reply at depth 2 wins (a terminal leaf behind a hit);
simulation counts of 1, 2 and 31 among the counts of the launch above.  15 x 15, 11 x 11 and 16 x 16 (S = 256: the last word of the
valid bits, cells at the top of the hand-over's 8-bit fields).

11 rows x 16 columns: MCTSEngine plays Gomoku on square boards only, so the rectangle comes through the engine's other game -- Connect4
on 11 x 16 with a net of 16 actions: the same kernel (k_delta_res knows cells, not rules: a leaf's cells are where the columns' stones
land), with BH != BW in the width's reciprocal, S = 176, the value row's stride S against the base planes' stride 256."""
import importlib.util
import os

import numpy as np
import pytest

import test_delta_gather as tdg
import test_delta_release as tdr
from conftest import REPO

pytestmark = pytest.mark.gpu

SIMS = 48


def _probe():
    spec = importlib.util.spec_from_file_location('memo_probe', os.path.join(REPO, 'profiles', 'microbench', 'memo_probe.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _empties(B):
    S = B * B
    y6 = 2 * B + 1
    sets = [
        (0, B - 1, S - B, S - 1, (B // 2) * B + B // 2, 1, B, S - 2),                              # corners, the centre, neighbours of corners
        (y6, y6 + 6, y6 + 7, y6 + 7 * B, y6 + 6 * B, S - 1, S - B, 0),                             # exactly 6 and exactly 7 along a row and a column
        (63, 64, 127, 128, 0, S - 1, B - 1, S - B, 65, 5 * B + 5) if S > 128 else (63, 64, 0, S - 1, B - 1, S - B, 65, 5 * B + 5),
        (0, 1, 2, B, B + 1, S - 1, S - 2, S - 3, S - B - 1, S - B - 2),                            # two clusters in opposite corners
        tuple(range(0, S, S // 11 | 1))[:12],                                                     # spread over the board
        (0, 7, 14 if B > 14 else B - 1, 7 * B, 7 * B + 7, S - 1, S - 8, 3 * B + 3, 4 * B + 10 if B > 10 else 4 * B + 9),
    ]
    return [tuple(sorted(set(int(c) for c in s))) for s in sets]


def _search(net, B, roots, counts=None, memo=True, resident=True, delta=True, then=None):
    """One search of SIMS simulations (per-game `counts`) on demand -> (trees, counters); `then(evaluator, eng)` runs behind it and its
    result is returned instead.  B: the side of a Gomoku board, or (rows, cols) of a Connect4 board (the net has `cols` actions)."""
    c4 = isinstance(B, tuple)
    import rlzero_amd.route as route
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    stones, to_move, last = roots
    was = os.environ.get('RZ_DELTA_MEMO')
    os.environ['RZ_DELTA_MEMO'] = '1' if memo else '0'
    decide = route.policy_on_demand
    try:
        evaluator = HipNetEvaluator(net, (B[0], B[1], B[1]) if c4 else B, 'cuda:0', max_boards=len(stones))
        evaluator.resident_search = resident
        evaluator.delta_trunk = delta
        eng = MCTSEngine(B, C4_ROW if c4 else 5, n_games=len(stones), n_playout=SIMS, device='cuda:0', add_noise=True, noise_seed=3,
                         game='connect4' if c4 else 'gomoku')
        if resident and delta:
            assert evaluator.resident_delta_ok(eng)
            route.policy_on_demand = lambda *a, **k: True

        def once():
            eng.set_roots(stones, to_move, last, reset_trees=True)
            eng.set_noise_keys()
            if counts is not None:
                eng.set_playouts(np.asarray(counts, dtype=np.int32))
            evaluator.hip.delta_stats(reset=True)
            eng.simulate(evaluator, SIMS, use_graph=False)
            st = evaluator.hip.delta_stats()
            trees = [eng.tree_dump(g) for g in range(len(stones))]
            if c4:   # paths of columns -> paths of the cells their stones land on (what the kernel's rule is about)
                trees = [_cell_paths(eng, tree, stones[g]) for g, tree in enumerate(trees)]
            eng.check()
            return trees, st
        out = once() if then is None else then(evaluator, eng, once)
        if counts is not None:
            eng.set_playouts(None)
        eng.close()
        evaluator.hip.close()
        return out
    finally:
        route.policy_on_demand = decide
        if was is None:
            del os.environ['RZ_DELTA_MEMO']
        else:
            os.environ['RZ_DELTA_MEMO'] = was


def _cell_paths(eng, tree, stones):
    from rlzero_amd.engine import bits_to_int
    occ0 = bits_to_int(stones[0]) | bits_to_int(stones[1])
    out = {}
    for path, nw in tree.items():
        occ, cells = occ0, []
        for a in path:
            cells.append(eng.cell_of_action(occ, a))
            occ |= 1 << cells[-1]
        out[tuple(cells)] = nw
    return out


def _ordered_leaves(net, B, roots):
    """-> per root the leaves' paths of simulations 1 .. SIMS in order: every root at every count, one launch of the full-board kernel."""
    stones, to_move, last = roots
    G = len(stones)
    rep = (np.repeat(stones, SIMS, axis=0), list(np.repeat(to_move, SIMS)), list(np.repeat(last, SIMS)))
    counts = np.tile(np.arange(1, SIMS + 1), G)
    trees, _ = _search(net, B, rep, counts=counts, memo=False)
    leaves = []
    for g in range(G):
        seq, before = [], {}
        for k in range(SIMS):
            tree = trees[g * SIMS + k]
            assert tree[()][0] == k + 1
            grown = [p for p, (n, _) in tree.items() if n > before.get(p, (0, 0.0))[0]]
            seq.append(max(grown, key=len))
            assert sorted(grown, key=len) == [seq[-1][:i] for i in range(len(seq[-1]) + 1)]   # one path grew
            before = tree
        leaves.append(seq)
    return leaves


def _expected(probe, leaves, B, counts=None):
    hits = fills = 0
    for g, seq in enumerate(leaves):
        c = probe.classify(seq[:SIMS if counts is None else counts[g]], B)
        hits, fills = hits + c['hits'], fills + c['fills']
    return hits, fills


@pytest.mark.parametrize('B', [15, 11, 16])
def test_trees_counters_and_the_switch(B):
    probe = _probe()
    net = tdg._net(B, 150 + B)
    empties = _empties(B)
    roots = tdg._roots(B, empties)
    leaves = _ordered_leaves(net, B, roots)
    pairs = [(p[0], p[1]) for seq in leaves for p in seq if len(p) == 2]
    dists = set(probe.cheb(a, b, B) for a, b in pairs)
    assert 6 in dists and 7 in dists and min(dists) <= 3 and max(dists) >= B - 1, dists   # overlapping, exactly 6, exactly 7, corner to corner
    hits, fills = _expected(probe, leaves, B)
    assert hits > 0 and fills > 0
    t_memo, s_memo = _search(net, B, roots)
    t_off, s_off = _search(net, B, roots, memo=False)
    t_full, _ = _search(net, B, roots, delta=False)
    t_two, s_two = _search(net, B, roots, resident=False)
    print(B, s_memo, s_off, (hits, fills))
    assert t_memo == t_off and t_memo == t_full and t_memo == t_two
    for g, seq in enumerate(leaves):   # (the order was derived from the same search)
        assert set(t_memo[g]) == set(p[:i] for p in seq for i in range(len(p) + 1))
    assert (s_memo['memo_hits'], s_memo['memo_fills']) == (hits, fills), (s_memo, hits, fills)
    assert s_off['memo_hits'] == 0 and s_off['memo_fills'] == 0 and s_two['memo_hits'] == 0
    for k in tdg.STATS:   # a served leaf counts the tiles its passes would have run
        assert s_memo[k] == s_off[k] == s_two[k], (k, s_memo, s_off, s_two)
    # per-game counts of 1, 2 and 31: a game's memo ends with its search
    counts = [(1, 2, 31, SIMS)[g % 4] for g in range(len(empties))]
    t_c, s_c = _search(net, B, roots, counts=counts)
    t_cf, _ = _search(net, B, roots, counts=counts, delta=False)
    assert t_c == t_cf
    assert (s_c['memo_hits'], s_c['memo_fills']) == _expected(probe, leaves, B, counts)


C4_ROWS, C4_COLS, C4_ROW = 11, 16, 9   # (nine in a row: no line among the roots below or two stones on)


def _c4_roots(n_games):
    """Connect4 positions on 11 x 16: column x of game g holds (3 x + 5 g) mod 10 stones (0 .. 9 of 11 rows, so every column stays
    legal and the landing cells lie on many rows), colours in runs of two along rows and diagonals as tdg._roots lays them; the side
    to move is the parity of the stones, the last move the top stone of a column of the other side."""
    rows, cols = C4_ROWS, C4_COLS
    stones = np.zeros((n_games, 2, 4), dtype=np.uint64)
    to_move, last = [], []
    for g in range(n_games):
        tops, n = {}, 0
        for x in range(cols):
            for y in range((3 * x + 5 * g) % 10):
                c, p = y * cols + x, 0 if (x + 2 * y) % 4 < 2 else 1
                stones[g, p, c >> 6] |= np.uint64(1) << np.uint64(c & 63)
                tops[x], n = (c, p), n + 1
        tm = n & 1
        to_move.append(tm)
        last.append([c for c, p in tops.values() if p == 1 - tm][g % 3])
    return stones, to_move, last


def test_a_rectangular_board_11x16():
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    probe = _probe()
    B = (C4_ROWS, C4_COLS)
    torch.manual_seed(191)
    net = PolicyValueNet(C4_ROWS, C4_COLS, C4_COLS)
    roots = _c4_roots(6)
    leaves = _ordered_leaves(net, B, roots)
    pairs = [p for seq in leaves for p in seq if len(p) == 2]
    assert any(p[0] // C4_COLS != p[1] // C4_COLS and abs(p[0] % C4_COLS - p[1] % C4_COLS) >= 7 for p in pairs)   # far pairs across rows
    assert any(p[1] == p[0] + C4_COLS for p in pairs)                                                               # b on top of a
    hits, fills = _expected(probe, leaves, C4_COLS)
    assert hits > 0 and fills > 0
    t_memo, s_memo = _search(net, B, roots)
    t_off, s_off = _search(net, B, roots, memo=False)
    t_full, _ = _search(net, B, roots, delta=False)
    t_two, s_two = _search(net, B, roots, resident=False)
    print(B, s_memo, (hits, fills))
    assert t_memo == t_off and t_memo == t_full and t_memo == t_two
    assert (s_memo['memo_hits'], s_memo['memo_fills']) == (hits, fills), (s_memo, hits, fills)
    assert s_off['memo_hits'] == 0 and s_two['memo_hits'] == 0
    for k in tdg.STATS:
        assert s_memo[k] == s_off[k] == s_two[k], (k, s_memo, s_off, s_two)


def test_a_terminal_leaf_behind_a_hit():
    """tests/test_delta_release.py's 'win2' roots: the reply at (2, 2) wins at depth 2 and is visited again and again; 7 or more cells
    from the first stone, its second and later visits are served from the memo, and the trees equal the full-board kernel's."""
    B = 15
    probe = _probe()
    win, S = 2 * B + 2, B * B
    roots, kinds, empties = tdr._terminal_roots(B)
    keep = [g for g, k in enumerate(kinds) if k == 'win2'][:4]
    roots = (roots[0][keep], [roots[1][g] for g in keep], [roots[2][g] for g in keep])
    net = tdg._net(B, 171)
    leaves = _ordered_leaves(net, B, roots)
    t_memo, s_memo = _search(net, B, roots)
    t_full, _ = _search(net, B, roots, delta=False)
    assert t_memo == t_full
    assert (s_memo['memo_hits'], s_memo['memo_fills']) == _expected(probe, leaves, B)
    far_wins = [p for seq in leaves for p in seq if len(p) == 2 and p[1] == win and probe.cheb(p[0], p[1], B) >= 7]
    assert len(far_wins) > len(set(far_wins)) and s_memo['memo_hits'] > 0   # the same terminal leaf again: a hit


def test_a_new_search_and_a_weight_reload_start_from_cleared_bits():
    """Every search here begins with the bases of its roots (select_first), so what clears the bits each time is k_memo_clear in front
    of the base build: the test holds THAT path -- without it the second search would fill nothing and the third would serve the old
    weights' windows.  The clear that comes with the headers (weight upload, rz_net_delta_invalidate) is not isolated here: behind it
    a continued search finds no valid base (base_ok false), so it neither serves nor fills until the next base build clears again."""
    B = 15
    net, net2 = tdg._net(B, 181), tdg._net(B, 182)
    roots = tdg._roots(B, _empties(B))

    def twice(evaluator, eng, once):
        first = once()
        second = once()                                        # the same roots again: the bases are rebuilt, the fills begin again
        evaluator.hip.load_state_dict(net2.state_dict())
        third = once()                                         # other weights: nothing of the old entries may be served
        return first, second, third
    first, second, third = _search(net, B, roots, then=twice)
    fresh = _search(net2, B, roots)
    assert first[1]['memo_hits'] > 0 and first[1]['memo_fills'] > 0
    assert second[0] == first[0] and (second[1]['memo_hits'], second[1]['memo_fills']) == (first[1]['memo_hits'], first[1]['memo_fills'])
    assert third[0] == fresh[0] and third[0] != first[0]
    assert (third[1]['memo_hits'], third[1]['memo_fills']) == (fresh[1]['memo_hits'], fresh[1]['memo_fills'])
