"""Network-vs-network matches on the device's move step (rz_play_set_match, rz_play_side; rlzero_amd/match.py): every game of a
match is the game a host-driven loop plays alone with the same kernels -- visit vector for visit vector --, a network against itself
scores exactly one half, each search takes exactly the games whose mover it plays, stalls end in the arbiter's move and leave a fresh
tree, the engines that cannot play a match refuse, match mode off is self-play as before, and slots refill.

The shapes are small on purpose: with fewer playouts than legal moves the reference's rule visits every child once before any twice, so
the visit vectors hold ones and twos, pi is spread over the visited children and nearly every draw lies within stall_margin = 0.05 of an
interval edge (the stall test resolves 209 of 255 moves at 6 x 6 and 440 of 442 at 11 x 11).  The comparisons do not depend on it."""
import ctypes

import numpy as np
import pytest

import sharp_fixture as sf
from oracle.evaluators import sharp_weights

pytestmark = pytest.mark.gpu

SEED = 17
ROUTES = {   # id -> (board, n_in_row, playouts, pairs, openings, opening plies)
    'compact_6x6': (6, 4, 40, 8, 4, 2),
    'receptive_field_11x11': (11, 5, 60, 4, 2, 4),
}


def _net(B, seed):
    """A PolicyValueNet on sharpened weights (tests/sharp_fixture.py: every .weight times the fixture's gain), so that the values of
    two seeds spread over (-1, 1) and the two networks search differently."""
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    net = PolicyValueNet(B)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sharp_weights(B, seed, sf.search(11)['gain']).items()})
    return net.to('cuda:0')


def _match(route, nets, n_slots, stall_margin=0.0):
    from rlzero_amd.match import BatchedMatch
    B, n_row, n_playout = ROUTES[route][:3]
    bm = BatchedMatch.for_networks(nets[0], nets[1], B, n_row, n_games=n_slots, n_playout=n_playout, device='cuda:0', seed=SEED,
                                   stall_margin=stall_margin)
    r = bm.evaluators[0].route(bm.eng)
    assert r.resident and (r.compact_resident if B == 6 else r.resident_delta), r
    return bm


def _openings(route):
    from rlzero_amd.match import paired_openings
    B, n_row, _, _, n_open, plies = ROUTES[route]
    return paired_openings(B, n_row, n_open, plies, seed=SEED)


def _alone(route, nets, results, openings):
    """The games of ``results`` replayed by a host-driven loop on a fresh engine of the same size: set_roots to the opening; per ply a
    fresh tree, simulate with the mover's evaluator, root_visits, numpy's draw on the match's uniform, step.
    -> [(moves, winner, visit vectors)] in the order of ``results``."""
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    from rlzero_amd.match import match_uniform, net_to_move, opening_arrays
    from rlzero_amd.selfplay import batch_pi_and_moves
    B, n_row, n_playout = ROUTES[route][:3]
    G = len(results)
    eng = MCTSEngine(B, n_row, n_games=G, n_playout=n_playout, device='cuda:0', add_noise=False)
    evs = [HipNetEvaluator(net, B, 'cuda:0', max_boards=G) for net in nets]
    gids = np.array([r.game_id for r in results], dtype=np.int64)
    stones, to_move, last = opening_arrays([openings[r.opening] for r in results], B, n_row)
    eng.set_roots(stones, to_move, last, reset_trees=True)
    taken = np.zeros((G, B * B), dtype=bool)
    for g, r in enumerate(results):
        taken[g, openings[r.opening]] = True
    running = np.ones(G, dtype=bool)
    moves_of, visits_of, winner_of, ply = [[] for _ in range(G)], [[] for _ in range(G)], [-1] * G, 0
    while running.any():
        for side in (0, 1):
            turn = running & (net_to_move(gids, ply % 2) == side)
            if turn.any():
                eng.set_active(turn.astype(np.uint8))
                eng.simulate(evs[side], n_playout)
        visits = eng.root_visits()
        rows = np.nonzero(running)[0]
        legal = ~taken[rows]
        _, picked = batch_pi_and_moves(visits[rows], legal, 1e-3, match_uniform(SEED, gids[rows], np.full(len(rows), ply)))
        chosen = np.full(G, -1, dtype=np.int32)
        chosen[rows] = picked
        taken[rows, picked] = True
        for g, leg in zip(rows, legal):
            moves_of[g].append(int(chosen[g]))
            visits_of[g].append(np.where(leg, visits[g], -1).astype(np.int32))
        eng.advance(np.where(running, -1, -2).astype(np.int32))   # a fresh root for the next search
        winner, ended = eng.step(chosen)
        for g in rows:
            if ended[g]:
                winner_of[g], running[g] = int(winner[g]), False
        ply += 1
    eng.check()
    for ev in evs:
        ev.hip.check_flags()
        ev.hip.close()
    eng.close()
    return [(moves_of[g], winner_of[g], visits_of[g]) for g in range(G)]


def _same_games(results, alone):
    assert len(results) == len(alone)
    for r, (moves, winner, visits) in zip(results, alone):
        assert r.moves == moves and r.winner == winner, (r.game_id, r.moves, moves, r.winner, winner)
        assert len(r.visits) == len(visits)
        for ply, (a, b) in enumerate(zip(r.visits, visits)):
            assert np.array_equal(a, b), (r.game_id, ply)


_cache = {}


def _played(route):
    """(networks, openings, the match's results, the same games played alone) of a route: computed once, shared, never changed."""
    if route not in _cache:
        B, _, n_playout, n_pairs = ROUTES[route][:4]
        nets, openings = (_net(B, 3), _net(B, 4)), _openings(route)
        bm = _match(route, nets, 2 * n_pairs)
        results = bm.run(n_pairs, openings)
        stats = (bm.stalls_resolved, bm.moves_done, bm.sims_done)
        bm.close()
        _cache[route] = (nets, openings, results, _alone(route, nets, results, openings), stats)
    return _cache[route]


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_a_match_game_is_the_game_played_alone(route):
    from rlzero_amd.match import score
    n_playout, n_pairs, n_open = ROUTES[route][2], ROUTES[route][3], ROUTES[route][4]
    nets, openings, results, alone, (stalls, moves_done, sims_done) = _played(route)
    assert [r.game_id for r in results] == list(range(2 * n_pairs))
    assert [r.opening for r in results] == [(g >> 1) % n_open for g in range(2 * n_pairs)]
    _same_games(results, alone)
    assert moves_done == sum(len(r.moves) for r in results) and sims_done == n_playout * moves_done
    for r in results:
        assert r.root_n == [n_playout] * len(r.moves)                    # one search from a fresh root per move
        assert all(int(v[v >= 0].sum()) == n_playout - 1 for v in r.visits)   # (the first simulation expands the root)
    # two different networks: the games of a pair are not the same game twice
    assert any(a.moves != b.moves for a, b in zip(results[0::2], results[1::2]))
    s = score(results)
    assert s['games'] == 2 * n_pairs and sum(s['pairs'].values()) == n_pairs and s['a_points'] == sum(r.points_a for r in results)


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_a_network_against_itself_scores_one_half(route):
    from rlzero_amd.match import score
    n_pairs = ROUTES[route][3]
    nets, openings = _played(route)[:2]
    bm = _match(route, (nets[0], nets[0]), 2 * n_pairs)
    results = bm.run(n_pairs, openings)
    bm.close()
    for a, b in zip(results[0::2], results[1::2]):
        assert a.pair == b.pair and a.moves == b.moves and a.winner == b.winner
        assert all(np.array_equal(x, y) for x, y in zip(a.visits, b.visits))
    s = score(results)
    assert s['a_score'] == 0.5 and s['elo_diff'] == 0.0
    assert s['pairs']['1-1'] + s['pairs']['tie-tie'] == n_pairs


def test_each_search_takes_the_games_of_its_mover():
    """An eager, stepped run (4 pairs through 6 slots, so slots refill): the active flags after each play_side against the slots'
    states, game ids and sides to move; every running game is searched by exactly one side per move; the games are the match's."""
    from rlzero_amd._hip import PLAY_RECORD_WORDS, PLAY_RUNNING, PLAY_SEARCHED
    from rlzero_amd.match import NET_A, NET_B, net_to_move
    import torch
    route = 'compact_6x6'
    n_playout = ROUTES[route][2]
    nets, openings, played = _played(route)[:3]
    bm = _match(route, nets, 6)
    eng = bm.eng
    bm.begin(4, openings)
    out, moves = [], 0
    while len(out) < 8:
        moves += 1
        assert moves < 200
        flags = {}
        with torch.cuda.stream(bm.stream):
            gid, _, state, _ = eng.play_state()
            to_move = eng.get_roots()[1]
            for side in (NET_A, NET_B):
                eng.play_side(side)
                flags[side] = eng.active_flags().astype(bool)
                eng.simulate(bm.evaluators[side], n_playout)
            row = eng.play_move()
        bm.stream.synchronize()
        running = state == 1
        for side in (NET_A, NET_B):
            assert np.array_equal(flags[side], running & (net_to_move(gid, to_move) == side)), (moves, side)
        assert not (flags[NET_A] & flags[NET_B]).any() and np.array_equal(flags[NET_A] | flags[NET_B], running)
        rec = bm.log.numpy()[row]
        searched = (rec[:, 4] & PLAY_SEARCHED) != 0
        assert np.array_equal(searched, running) and np.array_equal((rec[:, 4] & PLAY_RUNNING) != 0, state != 0)
        assert (rec[searched, 5] == n_playout).all()
        assert (np.where(rec[searched, PLAY_RECORD_WORDS:] >= 0, rec[searched, PLAY_RECORD_WORDS:], 0).sum(axis=1) == n_playout - 1).all()
        out.extend(bm.read_row(row))
    out.sort(key=lambda r: r.game_id)
    assert [r.game_id for r in out] == list(range(8))
    for r, p in zip(out, played[:8]):
        assert r.moves == p.moves and r.winner == p.winner and all(np.array_equal(x, y) for x, y in zip(r.visits, p.visits))
    eng.check()
    bm.close()


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_stalls_end_in_the_arbiters_move_and_a_fresh_tree(route):
    n_playout, n_pairs = ROUTES[route][2], ROUTES[route][3]
    nets, openings, _, alone = _played(route)[:4]
    bm = _match(route, nets, 2 * n_pairs, stall_margin=0.05)
    results = bm.run(n_pairs, openings)
    stalls, sims_done, moves_done = bm.stalls_resolved, bm.sims_done, bm.moves_done
    bm.close()
    _same_games(results, alone)
    assert stalls > 0
    assert sims_done == n_playout * moves_done          # a stalled slot's search is not repeated
    for r in results:
        assert r.root_n == [n_playout] * len(r.moves)   # after a resolved move too: the next search starts from a fresh root


def _queue(eng, n=4):
    t = eng.torch
    return t.arange(n, dtype=t.int64, device=eng.device), t.tensor([0, n], dtype=t.int32, device=eng.device)


def _set_match_rc(eng, arrays):
    """rz_play_set_match's return code, called directly."""
    t = eng.torch
    dev = [t.from_numpy(np.ascontiguousarray(arrays[0]).view(np.int64)).to(eng.device)] + \
          [t.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(eng.device) for x in arrays[1:]]
    rc = eng.lib.rz_play_set_match(eng.handle, *[ctypes.c_void_p(d.data_ptr()) for d in dev], len(arrays[1]), eng.stream())
    t.cuda.synchronize(eng.device)
    return rc


def test_engines_that_cannot_play_a_match_refuse():
    from rlzero_amd._hip import HipError
    from rlzero_amd.engine import MCTSEngine
    from rlzero_amd.match import opening_arrays, paired_openings
    ERR_ARG = -1
    arrays = opening_arrays(paired_openings(6, 4, 2, 2, seed=1), 6, 4)
    kw = dict(n_games=4, n_playout=16, device='cuda:0')
    for bad in (dict(score_mode='puct'), dict(add_noise=True)):
        eng = MCTSEngine(6, 4, **dict(kw, **bad))
        q = _queue(eng)
        eng.play_attach(1, 1e-3, q[0], q[1])
        assert _set_match_rc(eng, arrays) == ERR_ARG, bad
        with pytest.raises(HipError, match='rz_play_set_match'):
            eng.play_set_match(arrays)
        assert not eng.play_match_on
        eng.close()
    eng = MCTSEngine(6, 4, sims_in_flight=4, **kw)      # (the move step itself is refused there: no attach, no match)
    assert _set_match_rc(eng, arrays) == ERR_ARG
    eng.close()
    for rule in ('resign', 'cap'):
        eng = MCTSEngine(6, 4, **kw)
        q = _queue(eng)
        eng.play_attach(1, 1e-3, q[0], q[1])
        assert eng.lib.rz_play_side(eng.handle, 0, eng.stream()) == ERR_ARG      # no match: no sides
        eng.play_set_resign(-0.9, 0.1) if rule == 'resign' else eng.play_set_cap(4, 0.5)
        assert _set_match_rc(eng, arrays) == ERR_ARG, rule
        eng.play_attach(1, 1e-3, q[0], q[1])            # attached again: neither rule, a match may begin
        eng.play_set_match(arrays)
        assert eng.play_match_on
        assert eng.lib.rz_play_side(eng.handle, 2, eng.stream()) == ERR_ARG
        with pytest.raises(HipError, match='a match is on'):
            eng.play_set_resign(-0.9, 0.1) if rule == 'resign' else eng.play_set_cap(4, 0.5)
        eng.play_set_match(None)                        # off: the rules are accepted again
        eng.play_set_resign(-0.9, 0.1) if rule == 'resign' else eng.play_set_cap(4, 0.5)
        eng.torch.cuda.synchronize()
        eng.check()
        eng.close()


def test_match_mode_off_is_self_play_as_before():
    """play_set_match(openings) then play_set_match(None) on the engine of a self-play object: run_device (eager moves, so that the
    kernels read the flag as it is now) gives the 16 trajectories of a fresh engine."""
    from rlzero_amd.match import opening_arrays, paired_openings
    from rlzero_amd.selfplay import BatchedSelfPlay
    net = _played('compact_6x6')[0][0]
    kw = dict(board=6, n_in_row=4, n_games=8, n_playout=40, lanes=1, device='cuda:0', temperature=1.0, seed=5, add_noise=False)
    fresh = BatchedSelfPlay.for_network(net, **kw)
    fresh.device_attach(queue_capacity=16, move_graphs=False)
    want = fresh.run_device(range(16))
    sp = BatchedSelfPlay.for_network(net, **kw)
    sp.device_attach(queue_capacity=16, move_graphs=False)
    eng = sp.lanes[0].eng
    with sp._on(sp.lanes[0]):
        eng.play_set_match(opening_arrays(paired_openings(6, 4, 3, 2, seed=2), 6, 4))
        eng.play_set_match(None)
    got = sp.run_device(range(16))
    assert [t.game_id for t in got] == list(range(16))
    for a, b in zip(want, got):
        assert (a.game_id, a.moves, a.winner) == (b.game_id, b.moves, b.winner) and np.array_equal(a.pis, b.pis)
    assert any(len(t.moves) > 6 for t in got) and all(t.moves[0] >= 0 for t in got)
    for x in (fresh, sp):
        x.check()
        for lane in x.lanes:
            lane.eng.close()


def test_slots_refill():
    """6 pairs through 4 slots are the games of 6 pairs through 12 slots; every game id finishes once."""
    route = 'compact_6x6'
    nets, openings = _played(route)[:2]
    runs = []
    for n_slots in (4, 12):
        bm = _match(route, nets, n_slots)
        runs.append(bm.run(6, openings))
        bm.close()
    few, many = runs
    assert [r.game_id for r in few] == list(range(12)) == [r.game_id for r in many]
    for a, b in zip(few, many):
        assert a.opening == b.opening and a.moves == b.moves and a.winner == b.winner
        assert all(np.array_equal(x, y) for x, y in zip(a.visits, b.visits))
    # (and the first 16 games of the shared match are these 12, then four more)
    for a, p in zip(many, _played(route)[2]):
        assert a.moves == p.moves and a.winner == p.winner
