"""The per-ply temperature schedule of the device move step (rz_play_set_temperatures; MCTSEngine.play_set_temperatures,
BatchedSelfPlay.set_temperature_schedule): k_play_draw takes 1 / T and the stall margin of a slot from a device table indexed by the
slot's ply, and the host -- the arbiter of every move -- looks T up by the same ply.

Pinned here: the games are the oracle's, called with T[ply] move by move; a table set later reaches a move graph captured earlier;
lanes, chunk graphs and stalls, resignation and the playout cap, Connect4 (42 plies, 7 actions) play the same games in both loops;
schedule off gives the games of an object that never had one; and the calls refuse what they must."""
import numpy as np
import pytest

from oracle import evaluators as ev
from oracle.gomoku_ref import RefGomoku
from oracle.mcts_ref import RefPlayer, inverse_cdf_choice

pytestmark = pytest.mark.gpu

SEED = 5   # (chosen with the oracle alone: every one of its 20 games below differs from its game at the constant T = 1.0)


def _same(a, b):
    assert [t.game_id for t in a] == [t.game_id for t in b]
    for x, y in zip(a, b):
        assert (x.winner, x.moves) == (y.winner, y.moves), x.game_id
        assert np.array_equal(np.asarray(x.pis).view(np.uint64), np.asarray(y.pis).view(np.uint64)), x.game_id


def _net(*shape):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(4)
    return PolicyValueNet(*shape).to('cuda:0')


def _close(*sps):
    for sp in sps:
        for st in sp.check():
            assert st.reuse_dropped == 0
        for lane in sp.lanes:
            lane.eng.close()


def _oracle_game(seed, game_id, temps, n_playout):
    """game.py:96-134 with get_action called at the ply's temperature -> (winner, moves, pis)."""
    from rlzero_amd.selfplay import move_uniform
    us = move_uniform(seed, np.full(64, game_id), np.arange(64))
    player = RefPlayer(ev.vlin, n_playout, 5, is_selfplay=True, choice=inverse_cdf_choice(us))
    env = RefGomoku(6, 4)
    env.reset()
    moves, pis = [], []
    while True:
        T = float(temps[min(len(moves), len(temps) - 1)])
        move, pi = player.get_action(env, temperature=T, return_prob=True)
        env.step(move)
        moves.append(int(move))
        pis.append(pi)
        ended, winner = env.game_end_winner()
        if ended:
            return winner, moves, pis


def test_games_against_the_oracle():
    """6 x 6 / 4 in a row, 8 slots, 20 games, 40 playouts, the synthetic evaluator, T = 1 for four plies and 1e-3 from there."""
    from rlzero_amd.engine import MCTSEngine, SyntheticEvaluator
    from rlzero_amd.selfplay import BatchedSelfPlay, step_schedule
    temps = step_schedule(1.0, 4, 1e-3)
    eng = MCTSEngine(6, 4, n_games=8, n_playout=40, device='cuda:0')
    sp = BatchedSelfPlay(eng, SyntheticEvaluator('vlin'), temperature=1.0, seed=SEED)
    constant = sp.run_device(range(20))
    assert not eng.play_temp_on
    sp.set_temperature_schedule(temps)
    assert eng.play_temp_on
    dev = sp.run_device(range(20))
    assert [t.game_id for t in dev] == list(range(20))
    for t in dev:
        winner, moves, pis = _oracle_game(SEED, t.game_id, temps, 40)
        assert (winner, moves) == (t.winner, t.moves), t.game_id
        assert len(pis) == len(t.pis)
        for p1, p2 in zip(pis, t.pis):
            assert np.max(np.abs(p1 - p2)) <= 1e-12, t.game_id
    _same(dev, sp.run(range(20)))
    assert any(a.moves != b.moves for a, b in zip(dev, constant))
    assert all(a.moves[:4] == b.moves[:4] for a, b in zip(dev, constant))   # (T = 1 for the first four plies in both)
    eng.close()


def _check_rows(rows, temps, stats):
    """Every non-stalled searched record: the device's move is numpy's on the logged visits at the T of the record's ply."""
    from rlzero_amd import playlog
    from rlzero_amd._hip import PLAY_SEARCHED, PLAY_STALLED
    from rlzero_amd.selfplay import batch_pi_and_moves, move_uniform
    from move_step_twin import SEED as TWIN_SEED
    flags = playlog.decode(rows).flags
    d = playlog.decode(rows[((flags & PLAY_SEARCHED) != 0) & ((flags & PLAY_STALLED) == 0)])
    if not len(d.ply):
        return
    us = move_uniform(TWIN_SEED, d.game, d.ply)
    T = temps[np.minimum(d.ply, len(temps) - 1)]
    want = batch_pi_and_moves(d.counts, d.legal, T, us)[1]
    assert want.tolist() == d.move.tolist(), (d.ply.tolist(), T.tolist())
    stats['checked'] += len(d.ply)
    # (what the draw would have been at the attach's T = 1.0: told apart from the table's at least once, below)
    stats['not_constant'] += int((batch_pi_and_moves(d.counts, d.legal, 1.0, us)[1] != d.move).sum())


def _moves_under(rows, temps):
    """How many of the rows' moves numpy draws on the logged visits under ANOTHER table."""
    from rlzero_amd import playlog
    from rlzero_amd.selfplay import batch_pi_and_moves, move_uniform
    from move_step_twin import SEED as TWIN_SEED
    d = playlog.decode(rows)
    T = temps[np.minimum(d.ply, len(temps) - 1)]
    return int((batch_pi_and_moves(d.counts, d.legal, T, move_uniform(TWIN_SEED, d.game, d.ply))[1] == d.move).sum())


def test_table_updates_reach_a_captured_move_graph():
    """11 x 11, a real net on the resident receptive-field route: a table set before the capture is obeyed for six replayed moves, a
    different one set afterwards -- no new capture -- for four more; an eager twin writes the same rows."""
    from move_step_twin import Twin
    from rlzero_amd.selfplay import step_schedule
    net = _net(11)
    first = step_schedule(1.0, 3, 1e-3)                 # plies 0 .. 2 at T = 1, 3 .. 5 all but greedy
    second = np.array([1e-3] * 7 + [0.5, 0.25, 2.0])    # plies 6 .. 9: 1e-3, 0.5, 0.25, 2.0 -- `first` has 1e-3 at all of them
    rows = {}
    for graph in (True, False):
        twin = Twin(True, net, 6, 300)   # (more simulations than cells: the visit counts differ, so T decides the move)
        assert twin.route.resident_delta and not twin.eng.play_temp_on
        twin.eng.play_set_temperatures(first)
        assert twin.eng.play_temp_on
        if graph:
            twin.warm()
        captured = twin.graph
        stats = dict(checked=0, not_constant=0)
        out = []
        for _ in range(6):
            out.append(twin.move())
            _check_rows(out[-1], first, stats)
        assert stats['checked'] == 36 and [int(r[0, 2]) for r in out] == list(range(6))
        assert stats['not_constant'] >= 1
        twin.eng.play_set_temperatures(second)
        assert twin.graph is captured
        stats = dict(checked=0, not_constant=0)
        old = 0
        for _ in range(4):
            out.append(twin.move())
            _check_rows(out[-1], second, stats)
            old += _moves_under(out[-1], first)
        assert stats['checked'] >= 18
        assert old < stats['checked']   # some move is not the one the old table gives: the new table is read
        rows[graph] = out
        twin.close()
    assert len(rows[True]) == len(rows[False]) == 10
    for a, b in zip(rows[True], rows[False]):
        assert np.array_equal(a, b)


def test_lanes_graphs_and_stalls():
    """6 x 6, two lanes with chunk graphs: run_device, run, and run_device with a stall margin of 0.08 -- a stalled slot keeps its ply,
    so the host's move for it is drawn at the same T -- give the same games."""
    from rlzero_amd.selfplay import BatchedSelfPlay, step_schedule
    net = _net(6)
    temps = step_schedule(1.0, 4, 1e-3)
    sp = BatchedSelfPlay.for_network(net, board=6, n_in_row=4, n_games=7, n_playout=40, device='cuda:0', temperature=1.0, seed=21, lanes=2,
                                     use_graph=True, sims_per_graph=8, resident_search=False, temperature_schedule=temps)
    assert len(sp.lanes) == 2
    ids = list(range(20))
    dev = sp.run_device(ids)
    assert all(lane.eng.play_temp_on for lane in sp.lanes) and sp.stalls_resolved == 0
    _same(dev, sp.run(ids, pipelined=True))
    sp.device_attach(queue_capacity=64, stall_margin=0.08)
    assert all(lane.eng.play_temp_on for lane in sp.lanes)
    wide = sp.run_device(ids)
    _same(dev, wide)
    assert sp.stalls_resolved >= 1
    # the schedule is in force: the first four plies apart, pi is shared by the most visited children alone
    assert all(((pi < 1e-6) | (np.abs(pi - pi.max()) < 1e-9)).all() for t in dev for pi in t.pis[4:])
    assert any(max(pi) < 0.9 for t in dev for pi in t.pis[:4])
    _close(sp)


def _threshold(trajs):
    """A threshold between two logged statistics near their median, at least two float32 steps apart: the fp64 rule s < t and
    float32(s) < t then agree for every logged s."""
    s = np.unique(np.concatenate([t.resign_stats for t in trajs]))
    s = s[np.isfinite(s)]
    for i in range(len(s) // 2, len(s) - 1):
        if s[i + 1] > np.nextafter(np.nextafter(s[i], np.float32(2)), np.float32(2)):
            return (float(s[i]) + float(s[i + 1])) / 2
    raise AssertionError('no threshold')


def test_together_with_resignation_and_the_cap():
    from rlzero_amd.selfplay import BatchedSelfPlay, cap_uniform, decay_schedule
    net = _net(11)
    temps = decay_schedule(1.0, 0.05, 6.0, 121)
    cap = (20, 0.4)
    sp = BatchedSelfPlay.for_network(net, 11, 5, n_games=4, n_playout=150, lanes=1, device='cuda:0', temperature=1.0, seed=SEED,
                                     resign=(float('-inf'), 0.0), playout_cap=cap, temperature_schedule=temps)
    eng = sp.lanes[0].eng
    assert eng._ask(sp.lanes[0].evaluator)[0].resident
    ids = list(range(6))
    stats = sp.run_device(ids)
    assert eng.play_temp_on and eng.play_cap_on and eng.play_resign_on
    sp.set_resign(_threshold(stats), 0.25)
    dev = sp.run_device(ids)
    host = sp.run(ids)
    _same(dev, host)
    assert any(t.resigned for t in dev)
    for x, y in zip(dev, host):
        n = len(x.moves) + (1 if x.resigned else 0)   # (a resignation's search has a statistic and a budget, and no move)
        assert len(x.full) == len(x.resign_stats) == n, x.game_id
        assert x.full.tolist() == list(y.full) and x.resign_stats.tobytes() == y.resign_stats.tobytes() and x.resigned == y.resigned
        assert x.full.tolist() == (cap_uniform(SEED, x.game_id, np.arange(n)) < cap[1]).tolist()
    _close(sp)


def test_off_means_the_games_of_today():
    from rlzero_amd.selfplay import BatchedSelfPlay, step_schedule
    net = _net(6)
    kw = dict(board=6, n_in_row=4, n_games=6, n_playout=40, lanes=1, device='cuda:0', temperature=1.0, seed=SEED)
    ids = list(range(14))
    plain = BatchedSelfPlay.for_network(net, **kw)
    want = plain.run_device(ids)
    sp = BatchedSelfPlay.for_network(net, **kw)
    sp.device_attach()
    g0 = sp.lanes[0].move_graph
    assert g0 is not None and not sp.lanes[0].eng.play_temp_on
    sp.set_temperature_schedule(step_schedule(1.0, 2, 1e-3))   # the first schedule of an attached object: captured again
    graph = sp.lanes[0].move_graph
    assert graph is not None and graph is not g0 and sp.lanes[0].eng.play_temp_on
    cooled = sp.run_device(ids)
    assert [t.moves for t in cooled] != [t.moves for t in want]
    _same(cooled, sp.run(ids))
    sp.set_temperature_schedule(None)
    assert sp.lanes[0].move_graph is graph   # off: the same graph, the table holds the attach's 1 / T
    _same(want, sp.run_device(ids))
    _same(want, sp.run(ids))
    sp.set_temperature_schedule(step_schedule(1.0, 2, 1e-3))   # a later table goes straight through
    assert sp.lanes[0].move_graph is graph
    _same(cooled, sp.run_device(ids))
    _close(plain, sp)


def _queue(eng, n=4):
    t = eng.torch
    return t.arange(n, dtype=t.int64, device=eng.device), t.tensor([0, n], dtype=t.int32, device=eng.device)


def test_refusals():
    from rlzero_amd._hip import HipError
    from rlzero_amd.engine import MCTSEngine
    from rlzero_amd.match import opening_arrays, paired_openings
    from rlzero_amd.selfplay import BatchedSelfPlay
    arrays = opening_arrays(paired_openings(6, 4, 2, 2, seed=1), 6, 4)
    bad_tables = ([1.0, 0.0], [-1.0], [1.0, float('nan'), 1.0], [float('inf')], [1.0] * 37)
    # the library
    eng = MCTSEngine(6, 4, n_games=4, n_playout=16, device='cuda:0')
    with pytest.raises(HipError, match='rz_play_attach'):
        eng.play_set_temperatures([1.0])
    q = _queue(eng)
    eng.play_attach(1, 1.0, q[0], q[1])
    for bad in bad_tables:
        with pytest.raises(HipError, match='rz_play_set_temperatures'):
            eng.play_set_temperatures(bad)
        assert not eng.play_temp_on
    eng.play_set_match(arrays)
    with pytest.raises(HipError, match='a match is on'):
        eng.play_set_temperatures([1.0])
    assert not eng.play_temp_on
    eng.play_set_match(None)
    eng.play_set_temperatures([1.0] * 36)   # as many entries as cells: accepted
    assert eng.play_temp_on
    with pytest.raises(HipError, match='temperature schedule'):
        eng.play_set_match(arrays)
    eng.play_set_temperatures(None)         # off again is still "set since attach"
    with pytest.raises(HipError, match='temperature schedule'):
        eng.play_set_match(arrays)
    assert not eng.play_match_on
    eng.play_attach(1, 1.0, q[0], q[1])     # attached again: no schedule, a match may begin
    assert not eng.play_temp_on
    eng.play_set_match(arrays)
    eng.play_set_match(None)
    eng.torch.cuda.synchronize()
    eng.check()
    eng.close()
    # BatchedSelfPlay
    sp = BatchedSelfPlay.for_network(_net(6), board=6, n_in_row=4, n_games=4, n_playout=16, lanes=1, device='cuda:0', temperature=1.0, seed=1,
                                     add_noise=False)
    sp.device_attach(queue_capacity=8)
    lane = sp.lanes[0]
    for bad in bad_tables:
        with pytest.raises(ValueError):
            sp.set_temperature_schedule(bad)
        assert sp.temperature_schedule is None and not lane.eng.play_temp_on
    with sp._on(lane):
        lane.eng.play_set_match(arrays)
    with pytest.raises(ValueError, match='match'):
        sp.set_temperature_schedule([1.0, 0.5])
    assert sp.temperature_schedule is None and not lane.eng.play_temp_on
    with sp._on(lane):
        lane.eng.play_set_match(None)
    sp.set_temperature_schedule([1.0, 0.5])
    assert lane.eng.play_temp_on
    with sp._on(lane), pytest.raises(HipError, match='temperature schedule'):
        lane.eng.play_set_match(arrays)
    assert len(sp.run_device(range(4))) == 4
    _close(sp)


def test_connect4_has_as_many_plies_as_cells():
    """(6, 7): 7 actions, 42 cells -- a schedule of 42 entries is accepted and obeyed to the last ply, 43 are refused."""
    from rlzero_amd.selfplay import BatchedSelfPlay, decay_schedule
    net = _net(6, 7, 7)
    temps = decay_schedule(1.0, 0.02, 8.0, 42)
    assert temps.shape == (42, )
    sp = BatchedSelfPlay.for_network(net, board=(6, 7), n_in_row=4, n_games=6, n_playout=40, game='connect4', net_shape=(6, 7, 7), lanes=1,
                                     device='cuda:0', temperature=1.0, seed=SEED, temperature_schedule=temps)
    ids = list(range(14))
    dev = sp.run_device(ids)
    assert sp.lanes[0].eng.play_temp_on
    _same(dev, sp.run(ids))
    assert max(len(t.moves) for t in dev) > 7   # (plies beyond the action count: the table is indexed by cells)
    with pytest.raises(ValueError):
        sp.set_temperature_schedule(np.ones(43))
    plain = BatchedSelfPlay.for_network(net, board=(6, 7), n_in_row=4, n_games=6, n_playout=40, game='connect4', net_shape=(6, 7, 7), lanes=1,
                                        device='cuda:0', temperature=1.0, seed=SEED)
    assert [t.moves for t in plain.run_device(ids)] != [t.moves for t in dev]
    _close(sp, plain)
