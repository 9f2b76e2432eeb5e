"""The tree phase's loads of k_delta_res, asked for one phase early (rz_tree.h: backup_leaf_fetch, backup_path_fetch, select_root_fetch;
rz_delta.h: RZ_DELTA_EARLY): wave 0 requests the backup's leaf state in front of the value layer, the records of the path's nodes
behind its own quarter of that layer, and the next selection's root state in front of the barrier that orders the backup's stores.
Only WHERE loads are issued changes, so the resident search on the receptive-field trunk must build the same trees, bit for bit, as
the resident search on the full-board kernel and as the two-launch step (k_tree_step_def), with the policy features written during
the search and formed on demand.

Beside the 16-game sets of tests/test_delta_gather.py and tests/test_delta_release.py (their roots and helpers), the cases a value
fetched too early would get wrong: a parent whose child block grows and moves in the simulation whose backup reads it; every kind of
leaf in one search (first visit, old leaf expanded now, terminal leaf revisited, the root itself); a full arena and full prior
blocks inside a resident search; a game's last simulation (no selection, no selection fetch, one barrier less); two launches in a
row with a tree advance between them (the arena flips: nothing fetched in one launch may reach the next)."""
import numpy as np
import pytest

import arena_rules as ar
import test_delta_gather as tdg
import test_delta_release as tdl

pytestmark = pytest.mark.gpu

GAMES, SIMS = tdg.GAMES, tdg.SIMS
ARENA_FULL, BLOCKS_FULL = 1, 2   # include/rlzero_hip.h: RZ_FLAG_*


def _open_roots(B, n_games, n_empty, seed):
    """tdg._roots' boards with `n_empty` empty cells each, drawn per game."""
    rs = np.random.RandomState(seed)
    empties = [tuple(sorted(int(c) for c in rs.choice(B * B, n_empty, replace=False))) for _ in range(n_games)]
    return tdg._roots(B, empties)


def _run(net, B, roots, chunks, resident=True, delta=True, on_demand=False, moves_after=None, select_first_0=False, counts=None,
         active=None, **engine_kw):
    """Searches from `roots`, `chunks` simulations at a time -> what the search left: root visits, whole trees, the arenas' record
    arrays, error flags, delta counters.  moves_after: {chunk index: f(engine) -> moves}: behind that chunk every game keeps the
    subtree of its move and steps to it (the arena flips).  select_first_0: every chunk after the first is rz_select_step + the
    resident launch with select_first = 0."""
    import rlzero_amd.route as route
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine, check
    stones, to_move, last = roots
    G = len(stones)
    evaluator = HipNetEvaluator(net, B, 'cuda:0', max_boards=G)
    evaluator.resident_search = resident
    evaluator.delta_trunk = delta
    engine_kw.setdefault('n_playout', max(chunks))
    eng = MCTSEngine(B, 5, n_games=G, device='cuda:0', add_noise=True, noise_seed=3, **engine_kw)
    assert evaluator.resident_ok(eng) == resident and evaluator.deferred_ok(eng) and evaluator.delta_ok(eng) == delta
    eng.set_roots(stones, to_move, last, reset_trees=True)
    eng.set_noise_keys()
    if active is not None:
        eng.set_active(active)
    if counts is not None:
        eng.set_playouts(counts)
    evaluator.hip.delta_stats(reset=True)
    decide = route.policy_on_demand
    if on_demand:   # (an engine without the move step searches on demand only when told to: the decision is forced)
        assert evaluator.resident_delta_ok(eng)
        route.policy_on_demand = lambda *a, **k: True
    moved = []
    try:
        for i, n in enumerate(chunks):
            if resident and select_first_0 and i > 0:
                eng._ask(evaluator)[2]()   # (the evaluator's per-root work: the bases of the roots as they are now)
                assert eng._deferred_begin(evaluator, n) == n
                eng._search_mode(evaluator)
                check(eng.lib.rz_select_step(eng.handle, None, eng.stream()), 'rz_select_step')
                evaluator.search_resident(eng, n, False)
                eng._def_pending += n
                eng._def_stream = eng.torch.cuda.current_stream(eng.device)
            else:
                eng.simulate(evaluator, n, use_graph=False)
            if moves_after is not None and i in moves_after:
                moves = moves_after[i](eng)
                moved.append(moves)
                eng.advance_and_step(moves, moves)
        if resident:
            assert eng.search_launches[on_demand] > 0 and eng.search_launches[not on_demand] == 0
        st = evaluator.hip.delta_stats()
        out = {
            'visits': eng.root_visits().copy(),
            'trees': [eng.tree_dump(g) for g in range(G)],
            'arenas': [{k: np.array(v) for k, v in eng.arena(g).items() if k != 'PRI'} for g in range(G)],
            'flags': int(eng.stats().error_flags),
            'stats': {k: st[k] for k in tdg.STATS},
            'moves': moved,
        }
    finally:
        route.policy_on_demand = decide
    if counts is not None:
        eng.set_playouts(None)
    eng.close()
    evaluator.hip.close()
    return out


def _same(a, b, what, arenas=True):
    assert np.array_equal(a['visits'], b['visits']), what
    assert a['trees'] == b['trees'], what
    assert a['flags'] == b['flags'], (what, a['flags'], b['flags'])
    assert all(np.array_equal(x, y) for x, y in zip(a['moves'], b['moves'])), what
    if arenas:   # (slot for slot: N, W, first child, visited children, children, prior block; the top)
        for g, (x, y) in enumerate(zip(a['arenas'], b['arenas'])):
            assert sorted(x) == sorted(y) and int(x['top']) == int(y['top']), (what, g)
            used = _used_slots(x)
            assert used == _used_slots(y), (what, g)
            for k in ('N', 'W', 'FC', 'NV', 'K', 'PB'):
                assert np.array_equal(x[k][used].view(np.uint8), y[k][used].view(np.uint8)), (what, g, k)


def _used_slots(a):
    """The record slots of an arena that belong to its tree, walked from the root (the unused tail of a child block is not
    initialised)."""
    used, stack = [], [0]
    while stack:
        slot = stack.pop()
        used.append(slot)
        if int(a['K'][slot]) > 0 and int(a['NV'][slot]) > 0:
            stack.extend(range(int(a['FC'][slot]), int(a['FC'][slot]) + int(a['NV'][slot])))
    assert len(used) <= int(a['top'])
    return sorted(used)


def _all_routes(net, B, roots, chunks, two_launch=True, **kw):
    """k_delta_res in both modes against the resident full-board kernel and (two_launch) the two-launch step -> the first's result."""
    res = _run(net, B, roots, chunks, **kw)
    dem = _run(net, B, roots, chunks, on_demand=True, **kw)
    full = _run(net, B, roots, chunks, delta=False, **kw)
    print(B, chunks, res['stats'], res['flags'])
    assert dem['stats'] == res['stats']
    _same(res, dem, 'on demand')
    _same(res, full, 'full board')
    if two_launch:
        two = _run(net, B, roots, chunks, resident=False, **kw)
        assert two['stats'] == res['stats']
        _same(res, two, 'two launches')
    return res


@pytest.mark.parametrize('B', [11, 15, 16])
def test_sixteen_games_equal_every_other_route(B):
    """16 games x 32 simulations on the word-boundary and corner roots: root visits, whole trees and counters of k_delta_res, with
    features during the search and on demand, equal the resident full-board kernel's and the two-launch step's."""
    tdl._compare(tdg._net(B, 90 + B), B, tdg._roots(B, tdg._empties(B)))


def test_child_blocks_grow_and_move_under_the_early_fetch():
    """11 x 11 roots with 40 empty cells, 4 games x 96 simulations: the root's child block starts at kFirstCap records and doubles --
    and moves -- four times; select_body rewrites the parent's record (first child, visited children, capacity) in the simulation
    whose backup adds to that record from an early fetch.  Records compared slot by slot with the two-launch step's."""
    B, sims = 11, 96
    roots = _open_roots(B, 4, 40, 5)
    res = _all_routes(tdg._net(B, 101), B, roots, [sims])
    assert res['flags'] == 0
    for g, a in enumerate(res['arenas']):
        assert a['K'][0] == 40 and a['NV'][0] == 40 and a['N'][0] == sims, g     # every child of the root visited ...
        assert a['FC'][0] >= 1 + 4 + 8 + 16 + 32                                  # ... in a block that moved past the outgrown ones
        assert ar.FIRST_CAP == 4


@pytest.mark.parametrize('B', [11, 16])
def test_every_leaf_kind_in_one_search(B):
    """The terminal roots of tests/test_delta_release.py (a win at depth 1, at depth 2, a board that fills up).  The first
    simulation's leaf is the root itself -- depth 0, a path of one node, an OLD leaf expanded now (the `new_k > 0` rewrite of a record
    fetched early); every child is a first-visit leaf once (the whole-record write); the terminal leaves are visited again and
    again (`new_k == 0`: the record keeps what it has)."""
    roots, kinds, empties = tdl._terminal_roots(B)
    trees, _ = tdl._compare(tdg._net(B, 110 + B), B, roots)
    for g, (kind, tree, empty) in enumerate(zip(kinds, trees, empties)):
        assert tree[()][0] == SIMS, g
        depth1 = [p for p in tree if len(p) == 1]
        assert len(depth1) == len(empty), (g, kind)                                # the root was expanded, every child visited
        ends = [p for p in tree if tree[p][0] >= 2 and not any(len(q) > len(p) and q[:len(p)] == p for q in tree)]
        assert ends, (g, kind)                                                     # a terminal leaf visited again


def test_full_arena_and_full_prior_blocks_inside_a_resident_search():
    """An arena sized for 16 simulations with a minimal pool_factor (tests/test_arena_limits.py), searched for 640 on 11 x 11 roots
    of 40 empty cells: the prior blocks run out first (RZ_FLAG_BLOCKS_FULL: a leaf that stays a leaf), then the record slots
    (RZ_FLAG_ARENA_FULL: the selection stops at an expanded node, fresh == 2, and the backup must not expand it).  The engine flags
    both and goes on; flags, trees and records equal the two-launch step's."""
    B, n_playout, pf, total = 11, 16, 0.01, 640
    roots = _open_roots(B, 4, 40, 7)
    from rlzero_amd.engine import MCTSEngine
    probe = MCTSEngine(B, 5, n_games=4, n_playout=n_playout, pool_factor=pf, device='cuda:0')
    st = probe.stats()
    assert (st.arena_slots, st.prior_floats) == ar.capacities(pf, n_playout, B * B, 'uct_ref')
    probe.close()
    res = _all_routes(tdg._net(B, 103), B, roots, [n_playout] * (total // n_playout), n_playout=n_playout, pool_factor=pf)
    assert res['flags'] & BLOCKS_FULL and res['flags'] & ARENA_FULL and not res['flags'] & ~(BLOCKS_FULL | ARENA_FULL), res['flags']
    for g, a in enumerate(res['arenas']):
        assert a['N'][0] == total and int(a['top']) <= st.arena_slots, g


@pytest.mark.parametrize('B', [11, 16])
def test_last_simulations_and_an_inactive_game(B):
    """Per-game counts of 1, 2 and 31 (and the full 32) beside an inactive game: a game's last simulation makes no selection -- no
    selection fetch, one barrier less for every wave of its workgroup --, a game of one simulation backs up the root alone.  Against
    the resident full-board kernel with the same counts (the two-launch step has no per-game counts)."""
    counts = np.array([(1, 2, 31, 32)[g % 4] for g in range(GAMES)], dtype=np.int32)
    active = np.ones(GAMES, dtype=np.uint8)
    active[5] = 0
    res = _all_routes(tdg._net(B, 120 + B), B, tdg._roots(B, tdg._empties(B)), [SIMS], two_launch=False, counts=counts, active=active)
    assert res['flags'] == 0
    for g in range(GAMES):
        assert res['trees'][g][()][0] == (0 if g == 5 else counts[g]), g
        assert int(res['visits'][g].sum()) == (0 if g == 5 else counts[g] - 1), g


@pytest.mark.parametrize('select_first_0', [False, True], ids=['select_first', 'leaf_from_select_step'])
def test_two_searches_with_tree_reuse_between(select_first_0):
    """24 simulations, every game keeps the subtree of its most visited move and steps to it, 24 more: the arena flips, so cur_arena,
    top and the root position differ between the two launches.  The second launch selects its first leaf itself, or takes it from
    rz_select_step (select_first = 0)."""
    B = 11
    roots = _open_roots(B, 8, 12, 9)

    def best(eng):
        return np.argmax(eng.root_visits(), axis=1).astype(np.int32)
    res = _all_routes(tdg._net(B, 131), B, roots, [24, 24], moves_after={0: best}, select_first_0=select_first_0)
    assert res['flags'] == 0
    for g, tree in enumerate(res['trees']):
        assert tree[()][0] > 24, g    # the kept subtree's visits and the second search's
