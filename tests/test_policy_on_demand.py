"""Policy on demand (rz_net_search_resident_values, rz_net_policy_rows; route.policy_on_demand, MCTSEngine._search_mode): the resident
receptive-field search evaluates a leaf for the two value planes only, and a flush forms the four policy planes of exactly the records
it lists.  CPU: the mode decision as a truth table, the packing of the word a record carries for its leaf's planes, and the property of
the deep position the GPU test relies on.  GPU: twin engines -- one on demand, one writing the feature store during the search -- leave
the same log rows and, node by node, the same reachable trees and prior bytes (test_flush_kept's _reachable) wherever a flush can come
from.  Shapes are test_flush_kept's: 11 x 11, 6 .. 48 games, 48 .. 200 simulations."""
import itertools

import numpy as np
import pytest

import test_flush_kept as tfk
from move_step_twin import Twin as _Twin
from oracle.gomoku_ref import RefGomoku
from oracle.mcts_ref import RefSearch

SEED = tfk.SEED
B, N_ROW = 11, 5


# ----------------------------------------------------------------------------------------------- CPU
def test_mode_truth_table():
    """On demand exactly when: the route runs k_delta_res, the move step is attached, moves flush what they keep, no match, allowed."""
    from rlzero_amd import route
    base = route.decide(11, 11, n_games=8, n_cus=256, environ={})
    assert base.resident and base.resident_delta
    routes = {
        (True, True): base,
        (True, False): base._replace(resident_delta=False),   # the full-board resident kernel
        (False, True): base._replace(resident=False),          # the two-launch lanes
        (False, False): route.decide(6, 6, n_games=8, n_cus=256, environ={}),   # a smaller board
    }
    assert not routes[(False, False)].resident_delta
    seen = 0
    for (resident, delta), r in routes.items():
        for move_step, flush_kept, match, allowed in itertools.product([False, True], repeat=4):
            want = (r.resident and r.resident_delta) and move_step and flush_kept and not match and allowed
            assert route.policy_on_demand(r, move_step=move_step, flush_kept=flush_kept, match=match, allowed=allowed) is bool(want)
            seen += want
    assert seen == 1   # one row of 64
    assert route.policy_on_demand(base) is False   # (the defaults: no move step)
    # PUCT and several simulations in flight have no deferred route, hence no resident search, hence no policy on demand
    for how in ({'score_mode': 'puct'}, {'in_flight': 4}, {'deferred_priors': False}):
        r = route.decide(15, 15, n_games=8, n_cus=256, environ={}, **how)
        assert not route.policy_on_demand(r, move_step=True, flush_kept=True, match=False, allowed=True), how


def test_engine_switch_reads_the_environment():
    """RZ_POLICY_ON_DEMAND in the style of RZ_FLUSH_KEPT: '0' = off, read when the engine is made (engine.py); here its expression."""
    import inspect
    from rlzero_amd import engine
    src = inspect.getsource(engine.MCTSEngine.__init__)
    assert "os.environ.get('RZ_POLICY_ON_DEMAND', '1') != '0'" in src and "os.environ.get('RZ_FLUSH_KEPT', '1') != '0'" in src


def test_record_word_packing():
    """(side to move, last move) <-> the record's word: every pair of a 16 x 16 board and "no last move" comes back, no two collide, and
    the layout is rz_tree.h's (last + 1 in the low half, the side above)."""
    from rlzero_amd.route import pend_lw_pack, pend_lw_unpack
    words = {}
    for tm in (0, 1):
        for last in range(-1, 256):
            w = pend_lw_pack(tm, last)
            assert 0 <= w < 1 << 31 and pend_lw_unpack(w) == (tm, last)
            assert w == ((last + 1) | (tm << 16))
            words[w] = (tm, last)
    assert len(words) == 2 * 257
    assert pend_lw_pack(0, -1) == 0   # (zeroed memory reads as: first player to move, no last move)


def _deep_position():
    """A nearly full 11 x 11 board without a five and without a winning move: colour = ((x + 2 y) mod 4 < 2) has runs of at most two in
    every direction, and the empty cells share no line segment of five, so a stone on one makes a run of at most four...  checked
    below, not assumed.  Eight empty cells: 1 + 8 + 56 = 65 nodes within two stones of the root, fewer than the simulations."""
    empty = [(0, 0), (1, 6), (3, 2), (4, 9), (6, 4), (7, 10), (9, 1), (10, 7), (5, 0)]
    cells = {0: [], 1: []}
    for y in range(B):
        for x in range(B):
            if (y, x) not in empty:
                cells[0 if (x + 2 * y) % 4 < 2 else 1].append(y * B + x)
    n = min(len(cells[0]), len(cells[1]))
    moves = [c for pair in zip(cells[0][:n], cells[1][:n]) for c in pair]
    rest = cells[0][n:] + cells[1][n:]   # (the colours differ by a few cells: those stay empty too)
    env = RefGomoku.from_moves(B, N_ROW, moves)
    return env, len(empty) + len(rest)


def test_deep_position_has_kept_leaves_three_below_the_root():
    """What the GPU test below needs of its root: the oracle's search from it expands non-terminal leaves three or more stones below
    the root, also among those the most visited move keeps -- the records whose last move the stones do not tell."""
    env, n_empty = _deep_position()
    assert not env.game_end_winner()[0] and 6 <= n_empty <= 12
    search = RefSearch(tfk._value_fn, 200, 5)
    search.leaf_log = []
    search.simulate(env, 1.0)
    best = max(zip(search.root.kids, search.root.acts), key=lambda ka: ka[0].n)[1]

    def expanded(path):   # the node at `path` has children: the leaf was not terminal and got a block
        node = search.root
        for a in path:
            node = node.kids[node.acts.index(a)]
        return len(node.kids) > 0
    deep = [p for p, _ in search.leaf_log if len(p) >= 3 and expanded(p)]
    kept = [p for p in deep if p[0] == best]
    assert len(deep) >= 20 and len(kept) >= 3, (len(deep), len(kept))
    # from three stones on the last move is not a function of the stones: two kept leaves with the same stones, other last moves
    by_stones = {}
    for p in deep:
        by_stones.setdefault((frozenset(p[0::2]), frozenset(p[1::2])), set()).add(p[-1])
    assert any(len(v) > 1 for v in by_stones.values()) or len(deep) >= 20


# ----------------------------------------------------------------------------------------------- GPU: twins
def _net():
    return tfk._net('gomoku', B)[0]


def _pair(net, *args, **kw):
    return _Twin(True, net, *args, **kw), _Twin(False, net, *args, **kw)


def _same(a, b, rows, what):
    tfk._same_rows(rows, what)
    assert len(a.slot_of) == len(b.slot_of)
    tfk._same_trees(a, b, len(a.slot_of), what)


@pytest.mark.gpu
def test_flush_kept_twins_run_in_this_pairing():
    """tests/test_flush_kept.py's twins on the receptive-field route: the flush_kept twin searches on demand, the full-flush twin
    writes the store -- so those tests compare the two modes as well."""
    net, shape = tfk._net('gomoku', B)
    for graph in (False, True):
        kept, full = tfk._pair('gomoku', B, N_ROW, 6, 48, net, shape, graph=graph)
        rows = kept.move(), full.move()
        tfk._same_rows(rows, graph)
        assert kept.eng.search_launches == {True: 1, False: 0} and full.eng.search_launches == {True: 0, False: 1}
        kept.close()
        full.close()


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [False, True], ids=['play_move', 'move_graph'])
def test_full_flush_mid_search(graph):
    """sim_chunk, read the arena (a full flush on demand: every record with a block, by rows), sim_chunk, move; then more moves."""
    G, n = 6, 120
    a, b = _pair(_net(), G, n)
    for t in (a, b):
        t.search(70)
        t.slot_of = np.argsort(t.eng.play_state()[0], kind='stable')   # (which slot took which game is the refill's race)
    tfk._same_trees(a, b, G, 'mid-search')   # (reads the arenas: flushes)
    for t in (a, b):
        t.search(50)
    rows = a.move(search=False), b.move(search=False)
    _same(a, b, rows, 'moved')
    if graph:
        a.warm()
        b.warm()
    for ply in range(2):
        rows = a.move(), b.move()
        _same(a, b, rows, ply)
        if ply == 0:   # root_priors is a reader too; nothing is pending behind a move
            assert np.array_equal(a.eng.root_priors()[a.slot_of].view(np.uint8), b.eng.root_priors()[b.slot_of].view(np.uint8))
    a.close()
    b.close()


@pytest.mark.gpu
def test_deep_leaves():
    """Deep, narrow trees from _deep_position: kept records three and more stones below the root, whose planes need the record's own
    last move (a wrong word there changes their priors)."""
    G, n = 6, 200
    env, _ = _deep_position()
    a, b = _pair(_net(), G, n, roots=[env] * G)
    for ply in range(2):
        rows = a.move(), b.move()
        _same(a, b, rows, ply)
        assert (rows[0][:, 3] >= 0).all()
        if ply == 0:   # expanded nodes two stones below the NEW root: leaves three below the searched one, kept by the move
            depth = max(len(p) for p in tfk._expanded_paths(a.eng, int(a.slot_of[0])))
            assert depth >= 2, depth
    got, pending = a.eng.flush_kept_stats()
    assert 0 < got < pending
    a.close()
    b.close()


@pytest.mark.gpu
def test_rows_without_a_base():
    """The bases dropped between the eager search and the move: every listed row takes the four passes without a base."""
    G, n = 6, 200
    a, b = _pair(_net(), G, n)
    for ply in range(2):
        for t in (a, b):
            t.search()
            t.ev.hip.delta_invalidate()
        rows = a.move(search=False), b.move(search=False)
        _same(a, b, rows, ply)
    a.close()
    b.close()


@pytest.mark.gpu
def test_weight_reload_between_moves():
    """New weights between two moves, once with a search pending (the reload's flush is a full flush by rows, with the OLD weights and
    their bases) and once with nothing pending."""
    import torch
    G, n = 6, 120
    net = _net()
    a, b = _pair(net, G, n)
    rows = a.move(), b.move()
    _same(a, b, rows, 'before')
    for step, pending in enumerate((True, False)):
        if pending:
            a.search()
            b.search()
        with torch.no_grad():
            gen = torch.Generator(device='cpu').manual_seed(20 + step)
            for p in net.parameters():
                p.add_((0.05 * torch.randn(p.shape, generator=gen)).to(p.device))
        a.ev.refresh()
        b.ev.refresh()
        if pending:
            rows = a.move(search=False), b.move(search=False)
            _same(a, b, rows, 'searched with the old weights')
        rows = a.move(), b.move()
        _same(a, b, rows, 'new weights %d' % step)
    a.close()
    b.close()


@pytest.mark.gpu
def test_mode_change_with_records_pending():
    """Eager steps that write the store, then on demand -- by sim_chunk (the engine flushes what is pending in the other mode) and by
    the move graph -- and back."""
    G, n = 6, 96
    net = _net()
    a, b = _Twin(True, net, G, n), _Twin(False, net, G, n)
    a.eng.policy_on_demand = False
    a.search(40)            # store mode, pending
    a.eng.policy_on_demand = True
    a.search(56)            # on demand: the 40 are flushed first
    b.search(40)
    b.search(56)
    assert a.eng.search_launches == {True: 1, False: 1}
    rows = a.move(search=False), b.move(search=False)
    _same(a, b, rows, 'store then on demand')
    a.eng.policy_on_demand = False
    a.search(30)            # store mode again, pending when the graph is warmed and replayed
    b.search(30)
    a.eng.policy_on_demand = True
    a.warm()
    b.warm()
    a.search(10)            # on demand, pending when the graph is replayed: play_move_replay flushes it by rows
    b.search(10)
    for ply in range(2):
        rows = a.move(), b.move()
        _same(a, b, rows, 'graph %d' % ply)
    a.eng.search_launches = {True: 1, False: 0}   # (this twin changed modes on purpose: close() checks the others)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [False, True], ids=['play_move', 'move_graph'])
def test_uneven_counts_and_idle_slots(graph):
    """The playout cap (20 or 160 simulations per game and move) on an engine with three idle slots of eight."""
    G = 8
    a, b = _pair(_net(), G, 160, graph=graph, cap=(20, 0.5), queue_games=5)
    budgets = set()
    for ply in range(3):
        counts = a.eng.playouts()[0]
        rows = a.move(), b.move()
        assert len(a.slot_of) == 5
        budgets.update(int(counts[s]) for s in a.slot_of)
        _same(a, b, rows, ply)
    assert budgets == {20, 160}
    a.close()
    b.close()


@pytest.mark.gpu
def test_stalls_and_a_move_without_rows():
    """Every slot stalls and keeps its whole tree: 48 x 200 = 9600 rows, more than the rows kernel's fixed grid of two workgroups per
    CU; then the host's moves are applied by a move whose search finds no running... slot to search and whose list is empty."""
    G, n = 48, 200
    a, b = _pair(_net(), G, n, stall_margin=float(np.nextafter(0.5, 0.0)))
    assert G * n > 2 * a.ev.hip.n_cus
    a.eng.flush_kept_stats(reset=True)
    rows = a.move(), b.move()
    _same(a, b, rows, 'stall')
    assert (rows[0][:, 3] == -1).all()
    assert a.eng.flush_kept_stats(reset=True) == (G * n, G * n)
    visits = rows[0][:, 8:]
    for g in range(G):
        mv = int(np.argmax(visits[g]))
        a.eng.play_resolve(int(a.slot_of[g]), mv)
        b.eng.play_resolve(int(b.slot_of[g]), mv)
    rows = a.move(), b.move()
    assert a.eng.flush_kept_stats() == (0, 0)   # (a stalled slot is not searched: the move's list is empty)
    _same(a, b, rows, 'resolved')
    assert (rows[0][:, 3] >= 0).all()
    a.close()
    b.close()
