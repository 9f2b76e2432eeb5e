"""The early release of k_delta_res' trunk waves (rz_delta.h, ResHook::leaf; rz_tree.h, select_body's hook behind the descent): the
moment a selection has chosen the leaf's cell, waves 1 .. 3 go on to the next leaf's prologue and gather the base's records among the
three of them (rz_gather.h, Split<3>), while wave 0 finishes the selection -- the stash, the terminal test, the leaf's stores -- and
then writes the planes and runs every tile of conv1 in front of the pass's one barrier before conv2.  Only which wave moves which bytes,
and when, changes: the resident search on the receptive-field trunk must build the same trees, bit for bit, as the resident search on
the full-board kernel and as the two-launch step, with the policy features written during the search and formed on demand.

16 games, 32 simulations, nearly full boards (tests/test_delta_gather.py's roots and helpers).  Beside the word-boundary and corner
sets: roots whose leaves END behind the release -- a win at depth 1, a win at depth 2, a board that fills up --, the 16 x 16 root whose
three-stone leaves exceed the budget (the passes without a base, found out after an early release), and per-game simulation counts of
1, 2 and 31 beside an inactive game (the barrier counts when a game's last simulation has no selection)."""
import numpy as np
import pytest

import test_delta_gather as tdg

pytestmark = pytest.mark.gpu

GAMES, SIMS = tdg.GAMES, tdg.SIMS


def _colour(B, c):
    """The stone tdg._roots puts on cell c: player 0 where (x + 2 y) mod 4 < 2."""
    return 0 if (c % B + 2 * (c // B)) % 4 < 2 else 1


def _five(B, cells, c):
    """Whether `cells` (a set) + c holds five or more in a line through c."""
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        run = 1
        for s in (1, -1):
            y, x = c // B + s * dy, c % B + s * dx
            while 0 <= y < B and 0 <= x < B and (y * B + x) in cells:
                run += 1
                y, x = y + s * dy, x + s * dx
        if run >= 5:
            return True
    return False


def _terminal_roots(B):
    """-> (roots, kinds, empty cells): tdg._roots' boards, 16 games.  Games 0 .. 5 (kind 'win1'): two or three empty cells -- the count
    that leaves player 0 to move --, and cell (2, 2) completes five of player 0's along row 2 -- the stone at (2, 3) is player 0's
    instead of the pattern's player 1's --: a win at depth 1.  Games 6 .. 11 ('win2'): the same board with one empty cell more or less,
    so player 1 moves first and player 0's reply at (2, 2) wins at depth 2.  Games 12 .. 15 ('draw'): two empty cells on the plain
    pattern, where no move makes a line: the board fills up at depth 2."""
    S, win = B * B, 2 * B + 2
    flip = 2 * B + 3
    assert _colour(B, 2 * B) == 0 and _colour(B, 2 * B + 1) == 0 and _colour(B, flip) == 1 and _colour(B, 2 * B + 4) == 0
    others = [S - 1, S - B, B - 1, 6 * B + 5, 8 * B + 1, 9 * B + 7]
    empties, kinds = [], []
    n_win1 = 3 if S % 2 else 2   # (the side to move is the parity of the stones: an even count for player 0)
    for g in range(GAMES):
        if g < 6:
            empties.append((win, others[g], others[(g + 1) % 6])[:n_win1])
            kinds.append('win1')
        elif g < 12:
            empties.append((win, others[g - 6], others[(g - 5) % 6])[:5 - n_win1])
            kinds.append('win2')
        else:
            empties.append(((63, 64), (0, S - 1), (B - 1, S - B), (5 * B + 5, 5 * B + 6))[g - 12])
            kinds.append('draw')
    stones, to_move, last = tdg._roots(B, empties)
    for g in range(12):   # the stone at (2, 3) changes hands
        stones[g, 1, flip >> 6] &= ~(np.uint64(1) << np.uint64(flip & 63))
        stones[g, 0, flip >> 6] |= np.uint64(1) << np.uint64(flip & 63)
        if last[g] == flip:
            last[g] = 2 * B + 4 if to_move[g] == 1 else 0 * B + 2
    # what the kinds claim, restated on the host
    for g, (empty, kind) in enumerate(zip(empties, kinds)):
        mine = [set(c for c in range(S) if (int(stones[g, p, c >> 6]) >> (c & 63)) & 1) for p in (0, 1)]
        assert len(mine[0]) + len(mine[1]) == S - len(empty) and not (mine[0] & mine[1])
        assert not any(_five(B, mine[p] - {c}, c) for p in (0, 1) for c in mine[p]), 'the root itself has no line'
        assert (mine[1 - to_move[g]] | mine[to_move[g]]) >= {last[g]} and last[g] in mine[1 - to_move[g]]
        if kind == 'win1':
            assert to_move[g] == 0 and _five(B, mine[0], win)
        elif kind == 'win2':
            assert to_move[g] == 1 and _five(B, mine[0], win) and not any(_five(B, mine[1], c) for c in empty)
        else:
            assert not any(_five(B, mine[p], c) for p in (0, 1) for c in empty)
    return (stones, to_move, last), kinds, empties


def _compare(net, B, roots, expect_no_base=False):
    """k_delta_res in both modes against the resident full-board kernel and the two-launch step -> (trees, counters) of the first."""
    v_res, t_res, s_res = tdg._search(net, B, roots)
    v_dem, t_dem, s_dem = tdg._search(net, B, roots, on_demand=True)
    v_full, t_full, _ = tdg._search(net, B, roots, delta=False)
    v_two, t_two, s_two = tdg._search(net, B, roots, resident=False)
    print(B, s_res, s_dem, s_two)
    assert s_res['delta'] + s_res['no_base'] == len(roots[1]) * SIMS, s_res
    assert (s_res['no_base'] > 0) == expect_no_base, s_res
    assert s_dem == s_res and s_two == s_res
    for v, t, what in ((v_dem, t_dem, 'on demand'), (v_full, t_full, 'full board'), (v_two, t_two, 'two launches')):
        assert np.array_equal(v_res, v), what
        assert t_res == t, what
    return t_res, s_res


@pytest.mark.parametrize('B', [11, 15, 16])
def test_word_boundary_and_corner_roots(B):
    """(a) empty cells on both sides of the sets' word boundaries and in the corners: every leaf within the budget."""
    _compare(tdg._net(B, 60 + B), B, tdg._roots(B, tdg._empties(B)))


@pytest.mark.parametrize('B', [11, 15, 16])
def test_leaves_that_end_behind_the_release(B):
    """(b) a win at depth 1, a win at depth 2, a full board: the terminal test runs behind the release, its verdict is read one trunk
    later.  The trees show the terminal leaves: visited more than once, never expanded, every visit worth exactly +-1 (a win) or 0 (a
    draw)."""
    roots, kinds, empties = _terminal_roots(B)
    trees, _ = _compare(tdg._net(B, 70 + B), B, roots)
    win = 2 * B + 2
    for g, (kind, tree, empty) in enumerate(zip(kinds, trees, empties)):
        if kind == 'win1':
            ends = [p for p in tree if p == (win, )]
        elif kind == 'win2':
            ends = [p for p in tree if len(p) == 2 and p[1] == win]
        else:
            ends = [p for p in tree if len(p) == len(empty)]
        assert ends, (g, kind)
        for p in ends:
            n, w = tree[p]
            assert not any(len(q) > len(p) and q[:len(p)] == p for q in tree), (g, kind, p)
            assert abs(w) == (0 if kind == 'draw' else n), (g, kind, p, n, w)
        assert max(tree[p][0] for p in ends) >= 2, (g, kind)


def test_a_root_past_the_budget_after_an_early_release():
    """(c) 16 x 16, four empty cells far apart (tests/test_delta_gather.py): leaves three stones deep exceed the budget, which waves
    1 .. 3 find out in a prologue they began before wave 0 had finished the selection; they take the passes without a base."""
    B = 16
    over = (3 * 16 + 3, 3 * 16 + 12, 12 * 16 + 3, 12 * 16 + 12)
    assert not any(tdg._within(B, tuple(c for c in over if c != out)) for out in over) and 1 + 4 + 12 < SIMS
    _, s = _compare(tdg._net(B, 48), B, tdg._roots(B, [over] * GAMES), expect_no_base=True)   # (16 games: their last moves differ)
    assert s['delta'] > 0


@pytest.mark.parametrize('B', [11, 16])
def test_per_game_counts_and_an_inactive_game(B):
    """(d) simulation counts of 1, 2 and 31 (and the full 32) in one launch, one game inactive: a game's last simulation makes no
    selection and meets no release barrier, whatever the other games of the launch do.  Against the resident full-board kernel with
    the same counts (the two-launch step has no per-game counts)."""
    import rlzero_amd.route as route
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    net = tdg._net(B, 80 + B)
    stones, to_move, last = tdg._roots(B, tdg._empties(B))
    counts = np.array([(1, 2, 31, 32)[g % 4] for g in range(GAMES)], dtype=np.int32)
    active = np.ones(GAMES, dtype=np.uint8)
    active[5] = 0
    got = {}
    for name, delta, on_demand in (('store', True, False), ('on demand', True, True), ('full board', False, False)):
        ev = HipNetEvaluator(net, B, 'cuda:0', max_boards=GAMES)
        ev.delta_trunk = delta
        eng = MCTSEngine(B, 5, n_games=GAMES, n_playout=SIMS, device='cuda:0', add_noise=True, noise_seed=3)
        assert ev.resident_ok(eng) and ev.delta_ok(eng) == delta
        eng.set_roots(stones, to_move, last, reset_trees=True)
        eng.set_noise_keys()
        eng.set_active(active)
        eng.set_playouts(counts)
        decide = route.policy_on_demand
        if on_demand:
            assert ev.resident_delta_ok(eng)
            route.policy_on_demand = lambda *a, **k: True
        try:
            eng.simulate(ev, SIMS, use_graph=False)
            assert eng.search_launches[on_demand] > 0 and eng.search_launches[not on_demand] == 0
            visits = eng.root_visits().copy()
            trees = [eng.tree_dump(g) for g in range(GAMES)]
            eng.check()
        finally:
            route.policy_on_demand = decide
        eng.set_playouts(None)
        eng.close()
        ev.hip.close()
        got[name] = (visits, trees)
    visits, trees = got['store']
    for g in range(GAMES):
        assert int(visits[g].sum()) == (0 if g == 5 else counts[g] - 1), (g, visits[g].sum())
        assert trees[g][()][0] == (0 if g == 5 else counts[g]), g
    for name in ('on demand', 'full board'):
        assert np.array_equal(visits, got[name][0]), name
        assert trees == got[name][1], name
