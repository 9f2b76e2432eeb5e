"""Self-play resignation, host side (no GPU): the calibration of the threshold, the calibration games' uniform, z() of a resigned
game and the resignation fields through the multi-rank gather (header word 3)."""
import os
import socket

import numpy as np
import torch.multiprocessing as mp

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)

_M = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M
    z = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def _traj(gid, margin=np.nan, no_resign=True, resigned=False, plies=3, winner=0, n_cells=9, stats=None):
    from rlzero_amd.selfplay import Trajectory
    rng = np.random.RandomState(gid)
    pis = rng.dirichlet(np.ones(n_cells), size=plies)
    return Trajectory(gid, 3, 3, list(rng.permutation(n_cells)[:plies]), pis, winner, resigned=resigned, no_resign=no_resign,
                      resign_stats=stats, fp_margin=margin)


def test_calibrate_resign_threshold():
    from rlzero_amd.selfplay import calibrate_resign_threshold
    assert calibrate_resign_threshold([]) == float('-inf')
    # games that are not calibration games do not count
    assert calibrate_resign_threshold([_traj(0, -0.5, no_resign=False), _traj(1, -0.9, no_resign=False)]) == float('-inf')
    margins = [-0.9, -0.8, -0.7, -0.6, -0.5, -0.4, -0.3, -0.2, -0.1, 0.0]
    trajs = [_traj(i, m) for i, m in enumerate(margins)]
    # 5 % of 10 games: no false positive allowed -- the lowest margin itself (nobody's margin is below it)
    t = calibrate_resign_threshold(trajs, 0.05)
    assert t == np.float32(-0.9)
    # 20 %: two may fall below
    t = calibrate_resign_threshold(trajs, 0.2)
    assert t == np.float32(-0.7) and sum(np.float32(m) < t for m in margins) == 2
    # the largest such t: a hair above it three games would be false positives
    assert sum(np.float32(m) < np.nextafter(np.float32(t), np.float32(1)) for m in margins) == 3
    # ties: three games share the lowest margin -- none may be below the threshold, all three sit on it
    tied = [_traj(i, m) for i, m in enumerate([-0.8, -0.8, -0.8] + [0.5] * 7)]
    assert calibrate_resign_threshold(tied, 0.1) == np.float32(-0.8)
    assert calibrate_resign_threshold(tied, 0.2) == np.float32(-0.8)
    assert calibrate_resign_threshold(tied, 0.3) == np.float32(0.5)   # three may be below: the whole tie
    # all false positives (every calibration game would have been resigned by a non-loser at the same low value)
    allfp = [_traj(i, -0.99) for i in range(20)]
    assert calibrate_resign_threshold(allfp, 0.05) == np.float32(-0.99)
    # NaN margins (no finite statistic) never fire: they sort last
    assert calibrate_resign_threshold([_traj(0, np.nan), _traj(1, -0.5)], 0.5) == np.inf


def test_fp_margin():
    from rlzero_amd.selfplay import fp_margin
    st = np.array([-0.1, -0.9, -0.3, -0.8, np.nan], dtype=np.float32)
    assert fp_margin(st, 0) == np.float32(-0.3)     # player 0: plies 0, 2, 4
    assert fp_margin(st, 1) == np.float32(-0.9)     # player 1: plies 1, 3
    assert fp_margin(st, -1) == np.float32(-0.9)    # a tie: both players
    assert np.isnan(fp_margin(np.array([np.nan, -1.0], dtype=np.float32), 0))


def test_resign_uniform_is_splitmix64_with_its_own_salt():
    from rlzero_amd.selfplay import move_uniform, resign_uniform
    seed = 0x1234567890ABCDEF
    gids = np.array([0, 1, 2, 77, 1 << 40, (1 << 63) - 1], dtype=np.int64)
    got = resign_uniform(seed, gids)
    for gid, u in zip(gids, got):
        x = _splitmix64(_splitmix64(seed ^ 0x72657369676E0000) ^ int(gid))
        assert u == (x >> 11) * (1.0 / 9007199254740992.0)
    assert resign_uniform(seed, 5) != move_uniform(seed, 5, 0)
    u = resign_uniform(3, np.arange(20000))
    assert abs((u < 0.1).mean() - 0.1) < 0.01 and (u >= 0).all() and (u < 1).all()


def test_z_of_a_resigned_game():
    # player 1 resigns at ply 3 (three plies played: 0 and 2 by player 0, 1 by player 1): winner player 0
    t = _traj(1, resigned=True, no_resign=False, plies=3, winner=1 - 3 % 2, stats=np.zeros(4, np.float32))
    assert t.winner == 0 and list(t.z()) == [1.0, -1.0, 1.0]
    # player 0 resigns at ply 4: winner player 1
    t = _traj(2, resigned=True, no_resign=False, plies=4, winner=1 - 4 % 2, stats=np.zeros(5, np.float32))
    assert t.winner == 1 and list(t.z()) == [-1.0, 1.0, -1.0, 1.0]
    # the reference tuple: one sample per played ply
    w, data = t.as_reference_tuple()
    assert w == 1 and len(data) == 4


def _mixed(n_cells=9):
    return [_traj(0, np.float32(-0.25), no_resign=True, winner=1),
            _traj(1, resigned=True, no_resign=False, winner=0),
            _traj(2, no_resign=False, winner=-1, plies=9),
            _traj(3, np.float32(np.nan), no_resign=True, winner=0, plies=5),
            _traj(4, np.float32(-1.0), no_resign=True, plies=1, winner=-1)]


def _fields(t):
    return (t.game_id, t.moves, t.winner, t.resigned, t.no_resign, np.float32(t.fp_margin).tobytes())


def test_pack_payload_split_unpack_round_trip():
    from rlzero_amd.selfplay import (_payload_bytes, _payload_split, pack_trajectories, payload_of, unpack_trajectories)
    trajs = _mixed()
    for dtype in (np.float64, np.float32):
        header, moves, pis = pack_trajectories(trajs, 9)
        assert header[1, 3] == 1 << 32 and header[2, 3] == 0 and header[0, 3] >> 33 == 1
        raw, n, p = payload_of(trajs, 9, dtype)
        assert np.array_equal(raw, _payload_bytes(header, moves, pis, dtype))
        back = unpack_trajectories(*_payload_split(raw, n, p, 9, dtype), 3, 3)
        assert [_fields(a) for a in trajs] == [_fields(b) for b in back]
        for a, b in zip(trajs, back):
            assert np.array_equal(a.pis.astype(dtype), b.pis)
    # without resignation the format is what it was: header word 3 is 0, the bytes are those of plain trajectories
    from rlzero_amd.selfplay import Trajectory
    plain = [Trajectory(t.game_id, 3, 3, t.moves, t.pis, t.winner) for t in trajs]
    off = [Trajectory(t.game_id, 3, 3, t.moves, t.pis, t.winner, resigned=False, no_resign=False, resign_stats=None) for t in trajs]
    raw_plain, _, _ = payload_of(plain, 9, np.float64)
    header, moves, pis = pack_trajectories(off, 9)
    assert (header[:, 3] == 0).all()
    want = np.concatenate([np.array([[t.game_id, len(t.moves), t.winner, 0] for t in plain], np.int64).reshape(-1).view(np.uint8),
                           np.array([m for t in plain for m in t.moves], np.int64).view(np.uint8),
                           np.concatenate([t.pis for t in plain]).astype(np.float64).reshape(-1).view(np.uint8)])
    assert np.array_equal(raw_plain, want) and np.array_equal(payload_of(off, 9, np.float64)[0], want)
    back = unpack_trajectories(*_payload_split(want, len(plain), sum(len(t.moves) for t in plain), 9, np.float64), 3, 3)
    assert not any(t.resigned or t.no_resign for t in back) and all(np.isnan(t.fp_margin) for t in back)


def _gather_worker(rank, world, port, result_path):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from rlzero_amd import selfplay
    trajs = _mixed()
    local = [t for t in trajs if t.game_id % world == rank]
    merged = selfplay.gather_trajectories(local, 3, 3, dst=0, pi_dtype=np.float32)
    if rank == 0:
        assert [_fields(a) for a in trajs] == [_fields(b) for b in merged]
        # rank 0 calibrates on every rank's games
        assert selfplay.calibrate_resign_threshold(merged, 0.0) == np.float32(-1.0)
        assert selfplay.calibrate_resign_threshold(merged, 0.34) == np.float32(-0.25)
    else:
        assert merged is None
    dist.barrier()
    open(result_path + '.%d' % rank, 'w').write('ok')
    dist.destroy_process_group()


def test_two_rank_gather_carries_resign_fields(tmp_path):
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    result = str(tmp_path / 'resign')
    mp.spawn(_gather_worker, args=(2, port, result), nprocs=2, join=True)
    assert os.path.exists(result + '.0') and os.path.exists(result + '.1')
