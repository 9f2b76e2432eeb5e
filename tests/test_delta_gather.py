"""The base records of a receptive-field leaf, gathered record by record (rz_delta.h, delta_passes<SETS>; rz_gather.h): which lane moves
which 16 bytes is all that changes, so the resident search on the receptive-field trunk (k_delta_res) must build the same trees, bit
for bit, as the resident search on the full-board kernel and as the two-launch step -- with the policy features written to the store
during the search and formed on demand.

The roots are nearly full boards whose few empty cells sit where the gather's bookkeeping can go wrong: on both sides of the
boundaries between the 64-cell words of a set (cells 63 | 64, 127 | 128, 191 | 192), in the corners, and -- on 16 x 16 -- at (4, 4) +
(11, 11), the fullest budget that board admits.  A leaf's changed cells are the stones added below the root (or, for the root
itself, its last move): a subset of the root's empty cells, so every leaf's windows are known here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMES, SIMS = 16, 32
MAX_D = 4                                      # changed cells a delta pass handles (rz_delta.h: kMaxD)
BUDGET = (128, 128, 128, 164)                  # cells of W1 .. W4: 4 conv1 tiles of 32, 8 conv2 / conv3 tiles of 16 (and 128 conv1 slots), 164 conv2 slots
STATS = ('delta', 'no_base', 'cells', 'tiles3', 'tiles2')


def _totals(B, cells):
    """|W1| .. |W4| of a leaf whose changed cells are `cells`: the cells within Chebyshev distance r of one of them."""
    idx = np.arange(B * B)
    y, x = idx // B, idx % B
    d = np.full(B * B, 1000)
    for c in cells:
        d = np.minimum(d, np.maximum(np.abs(y - c // B), np.abs(x - c % B)))
    return tuple(int((d <= r).sum()) for r in (1, 2, 3, 4))


def _within(B, cells):
    return len(cells) <= MAX_D and all(t <= b for t, b in zip(_totals(B, cells), BUDGET))


def _empties(B):
    """16 sets of 2 .. 4 empty cells, all within the budget even when every one of them has changed."""
    S = B * B
    sets = [(b - 1, b) for b in (64, 128, 192) if b < S]
    sets += [(b - 1, b, S - 1 if b < S // 2 else 0) for b in (64, 128, 192) if b < S]
    sets += [(0, B - 1, S - B, S - 1), (0, S - 1), (B - 1, S - B), (0, B - 1, S - 1)]
    if B == 16:
        sets.append((4 * 16 + 4, 11 * 16 + 11))
    rs = np.random.RandomState(100 + B)
    while len(sets) < GAMES:
        cand = tuple(sorted(int(c) for c in rs.choice(S, 2 + len(sets) % 3, replace=False)))
        if _within(B, cand):
            sets.append(cand)
    sets = sets[:GAMES]
    assert all(2 <= len(s) <= MAX_D and _within(B, s) for s in sets)
    return sets


def _roots(B, empties):
    """(stones [G][2][4] uint64, sides to move, last moves): cell (y, x) holds a stone of player 0 where (x + 2 y) mod 4 < 2, of player 1
    elsewhere -- runs of two along rows and diagonals, alternating down the columns, so no line of five -- except the empty cells; the
    side to move is the parity of the stones, the last move a stone of the other side."""
    stones = np.zeros((len(empties), 2, 4), dtype=np.uint64)
    to_move, last = [], []
    for g, empty in enumerate(empties):
        cells = [[], []]
        for c in range(B * B):
            if c not in empty:
                cells[0 if (c % B + 2 * (c // B)) % 4 < 2 else 1].append(c)
        for p in (0, 1):
            for c in cells[p]:
                stones[g, p, c >> 6] |= np.uint64(1) << np.uint64(c & 63)
        tm = (len(cells[0]) + len(cells[1])) & 1
        to_move.append(tm)
        last.append(cells[1 - tm][(7 * g) % len(cells[1 - tm])])
    return stones, to_move, last


def _net(B, seed):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(seed)
    return PolicyValueNet(B)


def _search(net, B, roots, resident=True, delta=True, on_demand=False):
    """One search from `roots` -> (root visits, whole trees, delta counters of the search)."""
    import rlzero_amd.route as route
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    stones, to_move, last = roots
    evaluator = HipNetEvaluator(net, B, 'cuda:0', max_boards=len(stones))
    evaluator.resident_search = resident
    evaluator.delta_trunk = delta
    eng = MCTSEngine(B, 5, n_games=len(stones), n_playout=SIMS, device='cuda:0', add_noise=True, noise_seed=3)
    assert evaluator.resident_ok(eng) == resident and evaluator.deferred_ok(eng) and evaluator.delta_ok(eng) == delta
    eng.set_roots(stones, to_move, last, reset_trees=True)
    eng.set_noise_keys()
    evaluator.hip.delta_stats(reset=True)
    decide = route.policy_on_demand
    if on_demand:   # (an engine without the move step searches on demand only when told to: the decision is forced)
        assert evaluator.resident_delta_ok(eng)
        route.policy_on_demand = lambda *a, **k: True
    try:
        eng.simulate(evaluator, SIMS, use_graph=False)
        if resident:
            assert eng.search_launches[on_demand] > 0 and eng.search_launches[not on_demand] == 0
        st = evaluator.hip.delta_stats()
        visits = eng.root_visits().copy()
        trees = [eng.tree_dump(g) for g in range(len(stones))]
        eng.check()
    finally:
        route.policy_on_demand = decide
    eng.close()
    evaluator.hip.close()
    return visits, trees, {k: st[k] for k in STATS}


@pytest.mark.parametrize('B', [11, 13, 15, 16])
def test_trees_equal_the_full_board_kernel_and_the_two_launch_step(B):
    """16 roots, 32 simulations: visits and whole trees of the resident receptive-field search, in both modes, equal the resident
    full-board kernel's and the two-launch step's; every leaf stays within the budget, so none takes the passes without a base."""
    net = _net(B, 30 + B)
    roots = _roots(B, _empties(B))
    v_res, t_res, s_res = _search(net, B, roots)
    v_dem, t_dem, s_dem = _search(net, B, roots, on_demand=True)
    v_full, t_full, _ = _search(net, B, roots, delta=False)
    v_two, t_two, s_two = _search(net, B, roots, resident=False)
    print(B, s_res, s_dem, s_two)
    assert s_res['no_base'] == 0 and s_res['delta'] == GAMES * SIMS, s_res
    assert s_res['tiles3'] > 0 and s_res['tiles2'] > 0 and s_res['cells'] >= GAMES * SIMS, s_res
    assert s_dem == s_res and s_two == s_res
    for v, t, what in ((v_dem, t_dem, 'on demand'), (v_full, t_full, 'full board'), (v_two, t_two, 'two launches')):
        assert np.array_equal(v_res, v), what
        assert t_res == t, what


def test_a_root_past_the_budget_takes_the_passes_without_a_base():
    """16 x 16, four empty cells far apart: two of them changed stay within the budget (two 8 x 8 windows of radius 4), three do not
    (192 > 164 conv2 slots).  1 + 4 + 12 nodes lie within two stones of the root, fewer than the simulations, so leaves three stones
    deep are evaluated: without a base.  The trees equal the full-board kernel's all the same."""
    B = 16
    over = (3 * 16 + 3, 3 * 16 + 12, 12 * 16 + 3, 12 * 16 + 12)
    assert all(_within(B, (a, b)) for a in over for b in over if a < b)
    assert not any(_within(B, tuple(c for c in over if c != out)) for out in over)
    assert 1 + 4 + 12 < SIMS
    net = _net(B, 47)
    roots = _roots(B, [over] * 4)
    for on_demand in (False, True):
        v_res, t_res, s_res = _search(net, B, roots, on_demand=on_demand)
        print(on_demand, s_res)
        assert s_res['no_base'] > 0 and s_res['delta'] > 0 and s_res['delta'] + s_res['no_base'] == 4 * SIMS, s_res
        if not on_demand:
            v_full, t_full, _ = _search(net, B, roots, delta=False)
        assert np.array_equal(v_res, v_full)
        assert t_res == t_full
