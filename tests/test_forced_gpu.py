"""Forced playouts and policy target pruning on the device (rz_set_forced_playouts, rz_root_pruned_visits, rz_play_set_pruned_visits;
the rules are rlzero_amd/csrc/rz_forced.h, held to tests/forced_twin.py on the CPU by tests/test_forced_host.py).

(a) the three-launch step through HostEvaluator against the twin's search: the whole tree, root visits, W and priors, bit for bit, on
    the cases tests/test_forced_host.py shows the rule to be live on, then one move later with the kept subtree; root_pruned_visits
    against the twin's pruned counts on those trees, entry for entry; k = 0 gives the raw counts and the plain PUCT tree;
(b) the resident PUCT search against the three-launch step of a twin engine: every arena record and the pruned counts, one board per
    tile class, with and without noise, over four moves with tree reuse;
(c) whole games: run against run_device, a forced stall, prune=False;
(d) the refusals, and the trainer end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import forced_twin as ft
from oracle.gomoku_ref import RefGomoku
from oracle.mcts_ref import RefSearch, tree_dump
from test_gpu_parity import _engine as _host_engine, _hex_tree, _make_env, _set_roots, _skewed
from test_resident_puct_gpu import (C_PUCT, CASES, CLASS_BOARDS, DEV, _assert_same, _close, _engine, _evaluator, _net, _snapshot,
                                    _stream_pool_left_as_found)  # noqa: F401  (the fixture: this module draws streams too)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = ft.K


# ------------------------------------------------------------------------------------------------ (a) the twin
def _root_of(eng, acts):
    visits, wsum, pri = eng.root_visits()[0], eng.root_wsum()[0], eng.root_priors()[0]
    return [int(visits[a]) for a in acts], [float(wsum[a]).hex() for a in acts], [float(pri[a]) for a in acts]


def _assert_equals_twin(eng, s, c, tag):
    acts = s.root.acts
    assert _root_of(eng, acts) == ([k.n for k in s.root.kids], [float(k.w).hex() for k in s.root.kids], [float(k.p) for k in s.root.kids]), tag
    assert _hex_tree(eng.tree_dump(0)) == _hex_tree(tree_dump(s.root)), tag
    want = ft.pruned_root(s.root, K, c)
    got = eng.root_pruned_visits()[0]
    assert [int(got[a]) for a in acts] == [want[a] for a in acts], tag
    assert all(int(got[a]) == -1 for a in range(eng.n_actions) if a not in acts), tag
    return want


@pytest.mark.parametrize('case,evaluator', [(c, _skewed) for c in ft.CASES] + [(ft.WIDE_CASE, _skewed), (ft.TIE_CASE, ft.uniform32)],
                         ids=['3x3', '6x6c5', '6x6c1.5', '9x9', '11x11', '12x12wide', '3x3tie'])
def test_three_launch_step_equals_the_twin(case, evaluator):
    from rlzero_amd.engine import HostEvaluator
    B, n, pre, sims, c = case
    env = RefGomoku.from_moves(B, n, pre)
    eng = _host_engine(B, n, n_games=1, n_playout=sims, c_puct=c, score_mode='puct')
    eng.set_forced_playouts(K)
    _set_roots(eng, [env], reset_trees=True)
    host = HostEvaluator(evaluator, lambda s0, s1, tm, last: _make_env(B, n, s0, s1, tm, last))
    eng.simulate(host, sims)
    eng.check()
    s = ft.ForcedSearch(evaluator, sims, c, K)
    s.simulate(env, 1.0)
    assert s.forced_selections > 0
    want = _assert_equals_twin(eng, s, c, (case, 'move 1'))
    raw = dict(zip(s.root.acts, [k.n for k in s.root.kids]))
    if evaluator is _skewed:
        assert any(want[a] < raw[a] for a in raw) and any(want[a] == 0 < raw[a] for a in raw)
    # one move later, with the kept subtree (N and n are whatever the records hold)
    best = s.root.acts[max(range(len(s.root.kids)), key=lambda i: (s.root.kids[i].n, -i))]
    eng.advance([best])
    eng.step([best])
    s.update_with_move(best)
    env.step(best)
    if not env.game_end_winner()[0]:
        eng.simulate(host, sims)
        s.simulate(env, 1.0)
        _assert_equals_twin(eng, s, c, (case, 'move 2'))
    eng.check()
    eng.close()


def test_k_zero_is_plain_puct_and_raw_counts():
    from rlzero_amd.engine import HostEvaluator
    B, n, pre, sims, c = ft.CASES[1]
    env = RefGomoku.from_moves(B, n, pre)
    eng = _host_engine(B, n, n_games=1, n_playout=sims, c_puct=c, score_mode='puct')
    host = HostEvaluator(_skewed, lambda s0, s1, tm, last: _make_env(B, n, s0, s1, tm, last))
    plain = RefSearch(_skewed, sims, c, score_mode='puct')
    plain.simulate(env, 1.0)
    for k in (None, 0.0):   # never set, and set to 0 after having been on
        if k is not None:
            eng.set_forced_playouts(K)
            eng.set_forced_playouts(k)
        _set_roots(eng, [env], reset_trees=True)
        eng.simulate(host, sims)
        assert _hex_tree(eng.tree_dump(0)) == _hex_tree(tree_dump(plain.root))
        visits, pruned = eng.root_visits()[0], eng.root_pruned_visits()[0]
        legal = set(plain.root.acts)
        assert [int(pruned[a]) for a in range(eng.n_actions)] == [int(visits[a]) if a in legal else -1 for a in range(eng.n_actions)]
        assert any(int(visits[a]) == 1 for a in legal)   # (single playouts stay: nothing of the rule applies)
    eng.check()
    eng.close()


# ------------------------------------------------------------------------------------------------ (b) the resident route
ACTIVE = [1, 0, 1, 1, 1, 1, 1, 1]


def _twins8(case, net, **kw):
    """-> [(engine, evaluator)] x 2, eight games each, the second one idle: the resident PUCT route first, the three-launch step second."""
    out = []
    for resident in (True, False):
        ev = _evaluator(case, net, resident)
        eng = _engine(case, 8, **kw)
        eng.set_forced_playouts(K)
        assert ev.resident_ok(eng) is resident and not ev.deferred_ok(eng)
        out.append((eng, ev))
    return out


def _open8(eng):
    eng.reset_games()
    eng.set_noise_keys()
    eng.set_active(ACTIVE)


def _snap8(eng):
    snap = _snapshot(eng)
    snap['pruned'] = eng.root_pruned_visits().copy()
    return snap


def _resident_against_three_launch(case, noise):
    """-> whether the forced rule decided anything in these searches (the same engine with k = 0 builds other trees)."""
    sims = CASES[case][3]
    pairs = _twins8(case, _net(case), add_noise=noise, noise_seed=4)

    def four_moves(eng, ev):
        _open8(eng)
        rec = []
        for move in range(4):
            eng.simulate(ev, sims)
            rec.append(_snap8(eng))
            # game g plays its (g mod 3 + 1)-th most visited move: the kept subtrees differ from game to game
            order = np.argsort(-rec[-1]['visits'], axis=1, kind='stable')
            pick = order[np.arange(8), np.minimum(np.arange(8) % 3, (rec[-1]['visits'] > 0).sum(axis=1).clip(1) - 1)].astype(np.int32)
            eng.advance(np.where(ACTIVE, pick, -2).astype(np.int32))
            _, ended = eng.step(np.where(ACTIVE, pick, -1).astype(np.int32))
            if ended.any():
                break
        return rec
    records = [four_moves(eng, ev) for eng, ev in pairs]
    assert len(records[0]) == len(records[1]) >= 3
    for move, (x, y) in enumerate(zip(*records)):
        _assert_same(x, y, (case, noise, move))
    first = records[0][0]
    assert (first['root_n'][np.array(ACTIVE) == 1] == sims).all() and first['root_n'][1] == 0
    # (whether pruning lowers a count here is the data's affair -- (a) and (c) show it at work; what it may never do is raise one)
    assert all((rec['pruned'] <= rec['visits']).all() for rec in records[0])
    assert (first['pruned'][1] <= 0).all()   # (the idle game: an unsearched root)
    # the same engine with k = 0: its pruned counts are the raw ones, and where the rule was at work it builds other trees
    eng, ev = pairs[0]
    eng.set_forced_playouts(0.0)
    plain = four_moves(eng, ev)
    on = np.array(ACTIVE) == 1
    assert np.array_equal(plain[0]['pruned'][on], plain[0]['visits'][on])   # (the empty board: every action legal)
    live = any(not np.array_equal(x['visits'], y['visits']) for x, y in zip(plain, records[0]))
    _close(pairs)
    return live


@pytest.mark.parametrize('case', CLASS_BOARDS)
def test_resident_search_equals_the_three_launch_step(case):
    """Without and with Dirichlet noise (the noised prior is the p of both rules).  Whether the floor binds is the data's affair -- a
    sharp net at few simulations may visit every child often enough by itself -- so it is asked of the pair, not of each run."""
    live = [_resident_against_three_launch(case, noise) for noise in (False, True)]
    assert any(live), live


# ------------------------------------------------------------------------------------------------ (c) whole games
def _selfplay(case, resident_puct, forced=(K, True), **extra):
    from rlzero_amd.selfplay import BatchedSelfPlay
    game, board, n_in_row = CASES[case][:3]
    kw = dict(game='connect4', net_shape=(board[0], board[1], board[1])) if game == 'connect4' else {}
    kw.update(extra)
    return BatchedSelfPlay.for_network(_net(case), board, n_in_row, n_games=8, n_playout=40, c_puct=C_PUCT, lanes=1, device=DEV,
                                       temperature=1.0, seed=11, score_mode='puct', resident_puct=resident_puct, forced_playouts=forced, **kw)


def _same_games(a, b, tag, pis=True):
    assert [t.game_id for t in a] == [t.game_id for t in b], tag
    for x, y in zip(a, b):
        assert (x.winner, list(x.moves)) == (y.winner, list(y.moves)), (tag, x.game_id)
        assert x.raw_visits is not None and x.raw_visits.dtype == np.int32 and np.array_equal(x.raw_visits, y.raw_visits), (tag, x.game_id)
        if pis:
            assert np.array_equal(np.asarray(x.pis).view(np.uint64), np.asarray(y.pis).view(np.uint64)), (tag, x.game_id)


def _close_sp(*sps):
    for sp in sps:
        sp.check()
        for lane in sp.lanes:
            lane.eng.close()


@pytest.mark.parametrize('case', ['connect4', 'gomoku6'])
def test_run_and_run_device_play_the_same_games(case):
    """12 games in 8 slots on the resident PUCT route, Dirichlet noise on: the host-driven loop (pis from root_pruned_visits) against
    the device move step (pis from the ring's pruned rows; one whole-move hipGraph per move); then with a stall margin that makes slots
    stall; then prune=False: the same trees and moves, the pis from the raw counts."""
    from rlzero_amd.selfplay import batch_pi_and_moves
    ids = list(range(12))

    def raw_pis(t):   # the reference's expression on the raw counts (every legal action has a positive pi: log(0 + 1e-10) is finite)
        return batch_pi_and_moves(t.raw_visits, np.asarray(t.pis) > 0, 1.0, np.zeros(len(t.moves)))[0]

    sp = _selfplay(case, True)
    lane = sp.lanes[0]
    host = sp.run(ids)
    dev = sp.run_device(ids)
    assert lane.move_graph is not None and lane.eng.play_pruned is not None
    _same_games(host, dev, (case, 'loops'))
    # the moves came from the raw counts, the targets did not: somewhere pruning took a visited child out of pi
    raw = np.concatenate([t.raw_visits for t in host], axis=0)
    pis = np.concatenate([t.pis for t in host], axis=0)
    assert raw.shape == pis.shape and (raw.sum(axis=1) == 39).any()   # (a fresh root of 40 visits: 39 child visits)
    assert ((raw > 0) & (pis < 1e-9)).any()
    assert any(not np.array_equal(raw_pis(t), np.asarray(t.pis)) for t in host)
    sp.device_attach(queue_capacity=len(ids), stall_margin=0.2)
    _same_games(sp.run_device(ids), host, (case, 'stalls'))
    assert sp.stalls_resolved > 0 and lane.move_graph is not None
    sp.set_forced_playouts(K, prune=False)
    assert lane.eng.play_pruned is None
    for got in (sp.run_device(ids), sp.run(ids)):
        _same_games(got, host, (case, 'prune=False'), pis=False)
        for t in got:
            assert np.array_equal(np.asarray(t.pis), raw_pis(t))
    # ... and the option off again plays plain PUCT's games: no raw_visits, other moves somewhere
    sp.set_forced_playouts(0)
    off = sp.run_device(ids)
    assert all(t.raw_visits is None for t in off) and [list(t.moves) for t in off] != [list(t.moves) for t in host]
    _close_sp(sp)


def test_three_launch_lanes_play_the_same_games():
    """The three-launch step (no resident search, simulation hipGraphs captured with k in them) plays the resident route's games."""
    ids = list(range(8))
    res, three = _selfplay('gomoku6', True), _selfplay('gomoku6', False)
    assert three.lanes[0].move_graph is None and not three.lanes[0].evaluator.resident_ok(three.lanes[0].eng)
    want = res.run_device(ids)
    _same_games(three.run_device(ids), want, 'three-launch run_device')
    _same_games(three.run(ids), want, 'three-launch run')
    _close_sp(res, three)


# ------------------------------------------------------------------------------------------------ (d) refusals, the trainer
def _lib_refuses(eng, k, words):
    from rlzero_amd._hip import HipError, check
    with pytest.raises(HipError) as err:
        check(eng.lib.rz_set_forced_playouts(eng.handle, k), 'rz_set_forced_playouts')
    assert words in str(err.value), str(err.value)


def test_the_library_refuses():
    import torch
    from rlzero_amd._hip import HipError, check
    from rlzero_amd.engine import WORDS
    ref = _engine('gomoku6', 2, score_mode='uct_ref', c_puct=5.0)
    _lib_refuses(ref, 2.0, 'RZ_SCORE_PUCT')
    with pytest.raises(ValueError, match="'puct'"):
        ref.set_forced_playouts(2.0)
    queue = (torch.zeros(8, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))
    ref.play_attach(1, 1.0, queue[0], queue[1], ring_steps=4)
    ref.play_set_match((np.zeros((1, 2, WORDS), np.uint64), [0], [-1]))
    _lib_refuses(ref, 2.0, 'a match is on')
    ref.close()
    vl = _engine('gomoku6', 2, sims_in_flight=2)
    _lib_refuses(vl, 2.0, 'one simulation in flight')
    with pytest.raises(ValueError, match='one simulation in flight'):
        vl.set_forced_playouts(2.0)
    vl.close()
    eng = _engine('gomoku6', 2)
    for bad in (-1.0, float('nan'), float('inf')):
        _lib_refuses(eng, bad, 'not a finite number')
        with pytest.raises(ValueError, match='finite'):
            eng.set_forced_playouts(bad)
    assert eng.forced_k == 0.0
    # the ring needs the move step and k > 0; k is fixed once a move step holds it
    eng.play_attach(1, 1.0, queue[0], queue[1], ring_steps=4)
    with pytest.raises(HipError, match='forced playouts are off'):
        eng.play_set_pruned_visits(True)
    eng.set_forced_playouts(2.0)
    ring = eng.play_set_pruned_visits(True)
    assert tuple(ring.shape) == (4, 2, 36) and ring.dtype == torch.int32
    _lib_refuses(eng, 1.0, 'attach again')
    eng.play_set_pruned_visits(False)
    eng.set_forced_playouts(1.0)
    eng.play_refill()   # (a move step has been enqueued)
    _lib_refuses(eng, 2.0, 'attach again')
    with pytest.raises(HipError, match='attach again'):
        eng.play_set_pruned_visits(True)
    with pytest.raises(HipError, match='matches need the resident search'):   # (a match stays refused on a PUCT engine, whatever k is)
        check(eng.lib.rz_play_set_match(eng.handle, ring.data_ptr(), ring.data_ptr(), ring.data_ptr(), 1, eng.stream()), 'rz_play_set_match')
    eng.play_attach(1, 1.0, queue[0], queue[1], ring_steps=4)   # attach again: k may change
    eng.set_forced_playouts(2.0)
    eng.check()
    eng.close()


def test_selfplay_refuses():
    from rlzero_amd.engine import MCTSEngine, RolloutEvaluator
    from rlzero_amd.selfplay import BatchedSelfPlay
    with pytest.raises(ValueError, match="'puct'"):
        BatchedSelfPlay.for_network(_net('gomoku6'), 6, 4, n_games=4, n_playout=8, lanes=1, device=DEV, forced_playouts=2.0)
    with pytest.raises(ValueError, match='playout cap|resident search'):
        BatchedSelfPlay.for_network(_net('gomoku6'), 6, 4, n_games=4, n_playout=8, lanes=1, device=DEV, score_mode='puct',
                                    playout_cap=(4, 0.5), forced_playouts=2.0)
    eng = MCTSEngine(6, 4, n_games=2, n_playout=8, score_mode='puct', device=DEV)
    sp = BatchedSelfPlay(eng, RolloutEvaluator(seed=1))
    with pytest.raises(ValueError, match='priors'):
        sp.set_forced_playouts(2.0)
    eng.close()
    sp = _selfplay('gomoku6', True)
    with pytest.raises(ValueError, match='forced playouts'):
        sp.stream_start()
    with pytest.raises(ValueError, match='forced playouts'):
        sp.set_playout_cap(10, 0.5)
    _close_sp(sp)


def test_trainer_two_rounds(tmp_path):
    cmd = [sys.executable, os.path.join(REPO, 'tools', 'train_alphazero.py'), '--board', '6', '--n-in-row', '4', '--playouts', '24',
           '--batches', '2', '--check-freq', '100', '--games-in-flight', '8', '--seed', '3', '--score-mode', 'puct', '--resident-puct',
           '--forced-playouts', '2']
    out = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('forced playouts: k 2')]
    assert len(lines) == 2, out.stdout[-2000:]
    lowered, visited = [int(x) for x in lines[0].split(' plies, ')[1].split(' visited')[0].split(' of ')]
    assert 0 < lowered < visited
