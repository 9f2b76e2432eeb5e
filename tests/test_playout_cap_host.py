"""Playout cap randomization, the host side (no GPU): the budget draw cap_uniform, Trajectory.full / training_samples, the wire
format of the flags, set_playout_cap's refusals and the trainer's option."""
import importlib.util
import os

import numpy as np
import pytest
from conftest import REPO

from rlzero_amd import route as _route
from rlzero_amd.selfplay import (BatchedSelfPlay, Trajectory, cap_uniform, move_uniform, pack_trajectories, payload_of, resign_uniform,
                                 unpack_trajectories, _payload_split)


def test_cap_uniform_is_pinned_and_its_own_stream():
    keys = [(0, 0), (1, 0), (0, 1), (12345, 17), (2 ** 40 + 3, 224)]
    got = [float(cap_uniform(7, g, p)) for g, p in keys]
    assert got == [0.2582724945747593, 0.9116508540339513, 0.5542924802822109, 0.4257490026156062, 0.24861028947720454]
    assert got == [float(cap_uniform(7, g, p)) for g, p in keys]
    g, p = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
    assert cap_uniform(7, g, p).tolist() == got   # (vectorised: the same bits)
    assert not np.any(cap_uniform(7, g, p) == move_uniform(7, g, p))
    assert not np.any(cap_uniform(7, g, 0) == resign_uniform(7, g))
    assert not np.any(cap_uniform(7, g, p) == cap_uniform(8, g, p))


def test_share_of_full_plies():
    g, p = np.meshgrid(np.arange(200), np.arange(100))
    share = float((cap_uniform(11, g.ravel(), p.ravel()) < 0.25).mean())   # 20 000 keys: sigma = 0.0031
    assert 0.235 <= share <= 0.265, share


def _traj(full, resigned=False, n=7, gid=5):
    rs = np.random.RandomState(n)
    moves = rs.permutation(36)[:n].tolist()
    pis = rs.random_sample((n, 36))
    return Trajectory(gid, 6, 4, moves, pis, 1, resigned=resigned, full=full)


def test_training_samples_keep_the_flagged_plies():
    full = [True, False, False, True, True, False, True]
    t = _traj(full)
    every = list(zip(t.states(), list(t.pis), t.z()))
    got = t.training_samples()
    want = [every[i] for i, f in enumerate(full) if f]
    assert len(got) == 4 == len(want)
    for (s1, p1, z1), (s2, p2, z2) in zip(got, want):
        assert (s1 == s2).all() and (p1 == p2).all() and z1 == z2
    # the reference tuple is unchanged by the flags; without a cap every ply is a sample
    assert len(t.as_reference_tuple()[1]) == 7
    plain = _traj(None)
    assert plain.full is None and len(plain.training_samples()) == 7
    # a resigned game: one flag more than moves (the resigning search), which is no sample
    r = _traj(full + [True], resigned=True)
    assert len(r.full) == 8 and len(r.training_samples()) == 4


def test_pack_unpack_round_trips_full():
    trajs = [_traj([True, False, True], n=3, gid=1), _traj(None, n=4, gid=2), _traj([False] * 5 + [True], resigned=True, n=5, gid=3),
             _traj([False, False, True, False, False, False], resigned=True, n=5, gid=4)]
    back = unpack_trajectories(*pack_trajectories(trajs, 36), 6, 4)
    raw, n_games, n_plies = payload_of(trajs, 36, np.float64)
    wire = unpack_trajectories(*_payload_split(raw, n_games, n_plies, 36, np.float64), 6, 4)
    for out in (back, wire):
        for a, b in zip(trajs, out):
            assert (a.game_id, a.moves, a.winner, a.resigned) == (b.game_id, b.moves, b.winner, b.resigned)
            assert (a.full is None) == (b.full is None)
            if a.full is not None:
                assert a.full.tolist() == b.full.tolist() and b.full.dtype == bool
            assert (np.asarray(a.pis) == np.asarray(b.pis)).all()


def test_no_cap_packs_to_the_same_bytes():
    rs = np.random.RandomState(2)
    moves, pis = rs.permutation(36)[:6].tolist(), rs.random_sample((6, 36))
    a = [Trajectory(9, 6, 4, moves, pis, 0, full=None)]
    b = [Trajectory(9, 6, 4, moves, pis, 0)]
    for x, y in zip(pack_trajectories(a, 36), pack_trajectories(b, 36)):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert payload_of(a, 36, np.float32)[0].tobytes() == payload_of(b, 36, np.float32)[0].tobytes()
    # and they are the bytes of the format without the flags: game id, plies, winner, 0 | the moves | pi
    header, words, _ = pack_trajectories(a, 36)
    assert header.tolist() == [[9, 6, 0, 0]] and words.tolist() == moves
    capped = pack_trajectories([Trajectory(9, 6, 4, moves, pis, 0, full=[True] * 6)], 36)
    assert capped[0][0, 3] != 0 and (capped[1] >> 32).tolist() == [1] * 6


class _Eng(object):
    n_playout, sims_in_flight = 40, 1

    def __init__(self, resident):
        self.resident, self.calls = resident, []

    def _ask(self, evaluator):
        return _route.Route(needs_planes=False, deferred=True, delta=False, delta_three_launch=False, resident=self.resident,
                            resident_delta=False, compact_resident=False, resident_per_cu=1), None, None

    def set_playouts(self, counts):
        self.calls.append(counts)


class _Lane(object):
    def __init__(self, eng):
        self.eng, self.evaluator, self.stream = eng, None, None


def _stub(resident=True):
    import contextlib
    sp = BatchedSelfPlay.__new__(BatchedSelfPlay)
    sp.lanes = [_Lane(_Eng(True)), _Lane(_Eng(resident))]
    sp.eng, sp.seed, sp.playout_cap = sp.lanes[0].eng, 3, None
    sp._on = lambda lane: contextlib.nullcontext()
    return sp


def test_set_playout_cap_refuses():
    sp = _stub()
    for n_fast, p_full in ((0, 0.5), (-3, 0.5), (41, 0.5), (5, 0.0), (5, -0.1), (5, 1.0001), (5, float('nan'))):
        with pytest.raises(ValueError):
            sp.set_playout_cap(n_fast, p_full)
        assert sp.playout_cap is None
    sp.set_playout_cap(40, 1.0)
    assert sp.playout_cap == (40, 1.0)
    sp.set_playout_cap(1, 0.25)
    assert sp.playout_cap == (1, 0.25)
    assert sp._full(np.array([0, 1]), np.array([0, 0])).tolist() == (cap_uniform(3, np.array([0, 1]), 0) < 0.25).tolist()
    sp.set_playout_cap(None)
    assert sp.playout_cap is None and sp.lanes[0].eng.calls == [None]
    # a lane without a resident search (two-launch lanes, PUCT, sims_in_flight > 1, host evaluators): refused when the cap is set
    other = _stub(resident=False)
    with pytest.raises(ValueError, match='resident'):
        other.set_playout_cap(5, 0.5)
    assert other.playout_cap is None


def _trainer():
    spec = importlib.util.spec_from_file_location('train_alphazero_tool', os.path.join(REPO, 'tools', 'train_alphazero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trainer_parses_the_option():
    tool = _trainer()
    assert tool.parse_args([]).playout_cap is None
    assert tool.parse_args(['--games-in-flight', '16']).playout_cap is None
    args = tool.parse_args(['--games-in-flight', '16', '--playouts', '200', '--playout-cap', '50:0.25'])
    assert args.playout_cap == (50, 0.25)
    for bad in (['--playout-cap', '50:0.25'],                                            # not batched
                ['--games-in-flight', '16', '--playout-cap', '50'],
                ['--games-in-flight', '16', '--playout-cap', '0:0.5'],
                ['--games-in-flight', '16', '--playout-cap', '50:1.5'],
                ['--games-in-flight', '16', '--playouts', '40', '--playout-cap', '50:0.5']):   # n_fast above the full budget
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
