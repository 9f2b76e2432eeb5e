"""The device replay buffer (rz_replay_*, rlzero_amd.replay.DeviceReplay) against the trainer's host ReplayBuffer: after the same games
DeviceReplay(B, C) holds the entries of ReplayBuffer(8 C, B) fed training_samples() -- every entry index, bit for bit as float32 --
through ring wrap-around, several add calls, playout-cap gaps and float32 pi; the device draw is replay_indices; the raw records are
pack_positions; misuse raises; the learner takes the gathered tensors; the trainer's options run."""
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import REPO

import replay_cases as rc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _replay(board, capacity, **kw):
    from rlzero_amd.replay import DeviceReplay
    return DeviceReplay(board, capacity, device=DEV, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_as_host(dr, buf, what=''):
    """Every entry of the device buffer against the host buffer's, bit for bit."""
    assert len(dr) == len(buf), what
    if len(buf) == 0:
        return
    got = [x.cpu().numpy() for x in dr.gather(np.arange(len(buf)))]
    for g, w, name in zip(got, rc.host_entries(buf), ('states', 'pis', 'zs')):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, name)
        assert np.array_equal(_bits(g), _bits(w)), (what, name)


@pytest.mark.parametrize('board', [3, 4, 15, 16])
def test_every_entry_of_games_of_every_length(board):
    """1 ply, 2 plies, 65 plies (crosses a wave; the boards that have them), the full board (225: no multiple of 64; 256: every mask
    word and all four waves), winners 0, 1 and tie."""
    A = board * board
    lengths = [(1, 0), (2, 1), (min(65, A), -1), (A, 0), (A, 1), (min(A, 7), -1)]
    games = [rc.random_game(board, plies, winner, seed=100 * board + i, game_id=i) for i, (plies, winner) in enumerate(lengths)]
    capacity = sum(len(t.moves) for t in games) + 3
    dr = _replay(board, capacity)
    assert len(dr) == 0
    assert dr.add(games) == capacity - 3
    _same_as_host(dr, rc.host_buffer(games, capacity, board), board)
    dr.close()


@pytest.mark.parametrize('capacity', [100, 20, 5])
def test_ring(capacity):
    """A capacity larger than all games, one a game straddles the end of, one smaller than a game (its last plies remain); several
    add calls of several games against one add of all, compared with the host buffer after every call."""
    board = 4
    games = [rc.random_game(board, plies, winner, seed=7 + i, game_id=i)
             for i, (plies, winner) in enumerate([(10, 0), (12, 1), (9, -1), (16, 0), (1, 1), (7, 0)])]
    calls = [games[:2], games[2:3], games[3:6]]
    split, whole = _replay(board, capacity), _replay(board, capacity)
    done = []
    for call in calls:
        split.add(call)
        done += call
        _same_as_host(split, rc.host_buffer(done, capacity, board), (capacity, len(done)))
    whole.add(games)
    _same_as_host(whole, rc.host_buffer(games, capacity, board), capacity)
    assert len(split) == len(whole) == 8 * min(capacity, 55)
    # (the two rings may differ in where they start: what they hold is the same, position for position)
    for a, b in zip(split.read(), whole.read()):
        assert np.array_equal(a, b)
    split.close()
    whole.close()


def test_playout_cap_gaps():
    """A `full` mask with gaps, ply 0 and the last ply dropped: the held entries are training_samples(), and the stones of dropped
    plies are on the later boards."""
    board = 15
    full = np.ones(70, dtype=bool)
    full[[0, 3, 4, 63, 64, 69]] = False
    capped = rc.random_game(board, 70, 1, seed=5, game_id=0, full=full)
    resigned = rc.random_game(board, 6, 0, seed=6, game_id=1, full=[True, False, True, True, False, True, True])   # (one flag more than plies)
    games = [capped, resigned]
    dr = _replay(board, 200)
    assert dr.add(games) == 64 + 4 == sum(len(t.training_samples()) for t in games)
    _same_as_host(dr, rc.host_buffer(games, 200, board))
    states, _, _ = dr.gather([8 * 0 + 6])   # the first kept ply (ply 1), un-transformed planes (four quarter turns)
    planes = states[0].cpu().numpy().reshape(4, -1)
    assert planes[1].sum() == 1 and planes[1][capped.moves[0]] == 1 and planes[0].sum() == 0   # the dropped ply 0's stone: the opponent's
    assert planes[2][capped.moves[0]] == 1 and planes[3].sum() == 0
    dr.close()


def test_float32_pi_is_the_same_bits():
    board = 4
    games64 = [rc.random_game(board, 9, 0, seed=21, game_id=0), rc.random_game(board, 16, -1, seed=22, game_id=1)]
    games32 = [rc.random_game(board, 9, 0, seed=21, game_id=0, pi_dtype=np.float32), rc.random_game(board, 16, -1, seed=22, game_id=1, pi_dtype=np.float32)]
    assert games32[0].pis.dtype == np.float32 and games64[0].pis.dtype == np.float64
    a, b = _replay(board, 30), _replay(board, 30)
    a.add(games64)
    b.add(games32)
    idx = np.arange(len(a))
    for x, y in zip(a.gather(idx), b.gather(idx)):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
    _same_as_host(a, rc.host_buffer(games64, 30, board))
    a.close()
    b.close()


def test_sample_is_the_host_draw():
    import torch
    from rlzero_amd.replay import replay_indices
    board, seed = 15, 11
    games = [rc.random_game(board, 40 + i, i % 2, seed=30 + i, game_id=i) for i in range(3)]
    dr = _replay(board, 100, seed=seed)   # (the ring has wrapped: 123 positions)
    dr.add(games)
    assert len(dr) == 800
    n = 300

    def same(got, want):
        return all(torch.equal(g, w) for g, w in zip(got, want))
    step3 = dr.sample(n, step=3)
    assert same(step3, dr.gather(replay_indices(seed, 3, n, len(dr))))
    assert same(step3, dr.sample(n, step=3))                    # the same step repeats
    assert not same(step3, dr.sample(n, step=4))                # two steps differ
    first, second = dr.sample(n), dr.sample(n)                  # the internal counter: steps 0, 1
    assert same(first, dr.gather(replay_indices(seed, 0, n, len(dr)))) and same(second, dr.sample(n, step=1)) and dr.step == 2
    # indices from a device tensor: the same launch
    idx = replay_indices(seed, 3, n, len(dr))
    assert same(step3, dr.gather(torch.from_numpy(idx).to(DEV)))
    assert [tuple(x.shape) for x in step3] == [(n, 4, board, board), (n, board * board), (n, )]
    dr.close()


def test_raw_records():
    from rlzero_amd.replay import pack_positions
    board = 16
    full = np.ones(256, dtype=bool)
    full[[0, 100, 255]] = False
    games = [rc.random_game(board, 256, 1, seed=40, game_id=0, full=full), rc.random_game(board, 3, -1, seed=41, game_id=1)]
    dr = _replay(board, 300)
    dr.add(games)
    want = pack_positions(games, board)
    got = dr.read()
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert int(got[0][-4, 1, 3]) != 0     # (the fourth mask word is in use)
    part = dr.read(250, 6)
    assert all(np.array_equal(p, w[250:256]) for p, w in zip(part, want))
    dr.close()


def test_misuse_raises():
    import torch
    from rlzero_amd._hip import HipError
    from rlzero_amd.selfplay import Trajectory
    for board in (2, 17):
        with pytest.raises(HipError):
            _replay(board, 10)
    with pytest.raises(HipError):
        _replay(4, 0)
    dr = _replay(4, 10)
    with pytest.raises(HipError):
        dr.sample(4)                                            # empty
    with pytest.raises(HipError):
        dr.gather([0])
    with pytest.raises(ValueError):
        dr.add([Trajectory(0, (6, 7), 4, [3, 3], np.full((2, 7), 1 / 7), 0, game='connect4')])
    with pytest.raises(ValueError):
        dr.add([rc.random_game(5, 3, 0, seed=1)])               # another board
    with pytest.raises(HipError):
        dr.add([Trajectory(0, 4, 4, list(range(16)) + [0], np.full((17, 16), 1 / 16), 0)])   # longer than the board has cells
    with pytest.raises(HipError):
        dr.add([Trajectory(0, 4, 4, [16], np.full((1, 16), 1 / 16), 0)])                    # a move outside the board
    assert len(dr) == 0
    dr.add([rc.random_game(4, 5, 0, seed=2)])
    assert len(dr) == 40
    for bad in ([40], [-1], [0, 39, 40]):
        with pytest.raises(HipError):
            dr.gather(bad)
        with pytest.raises(HipError):
            dr.gather(torch.tensor(bad, dtype=torch.int64, device=DEV))
    states, pis, zs = dr.gather(torch.tensor([39, 0], dtype=torch.int64, device=DEV))   # (the flag does not linger)
    assert states.shape == (2, 4, 4, 4) and float(pis.sum()) == pytest.approx(2.0, abs=1e-5)
    dr.close()


def test_learner_takes_the_gathered_tensors():
    import torch
    from rlzero_amd.games.gomoku.alphazero_agent import AlphaZeroAgent
    board = 6
    games = [rc.random_game(board, 20 + i, i % 2, seed=50 + i, game_id=i) for i in range(3)]
    dr = _replay(board, 100)
    dr.add(games)
    buf = rc.host_buffer(games, 100, board)
    idx = np.random.RandomState(0).permutation(len(buf))[:64]
    rows = [buf[int(i)] for i in idx]
    host = [list(col) for col in zip(*rows)]
    gathered = dr.gather(idx)
    agents = []
    for _ in range(2):
        torch.manual_seed(9)
        agents.append(AlphaZeroAgent(board, device=DEV))
    for h, g in zip(host, gathered):
        assert torch.equal(agents[0]._tensor(h), g) and agents[1]._tensor(g) is g
    probs_h, v_h = agents[0].policy_value(host[0])
    probs_d, v_d = agents[1].policy_value(gathered[0])
    assert np.allclose(probs_h, probs_d, atol=1e-6) and np.allclose(v_h, v_d, atol=1e-6)
    loss_h, ent_h = agents[0].learn(*host)
    loss_d, ent_d = agents[1].learn(*gathered)
    assert np.isfinite([loss_h, ent_h]).all()
    assert abs(loss_h - loss_d) <= 1e-6 and abs(ent_h - ent_d) <= 1e-6
    dr.close()


@pytest.mark.parametrize('device_replay', [True, False])
def test_trainer_options(tmp_path, device_replay):
    cmd = [sys.executable, os.path.join(REPO, 'tools', 'train_alphazero.py'), '--board', '6', '--n-in-row', '4', '--playouts', '24',
           '--games-in-flight', '16', '--batches', '2', '--batch-size', '64', '--updates-per-round', '4', '--seed', '1'] + (['--device-replay'] if device_replay else [])
    env = dict(os.environ, PYTHONPATH=REPO)
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(('batch i:', 'kl:'))]
    assert [ln.split(':')[0] for ln in lines] == (['batch i'] + ['kl'] * 4) * 2, out.stdout[-2000:]
    for ln in lines:
        if ln.startswith('kl:'):
            fields = dict(f.split(':') for f in ln.split(','))
            assert list(fields) == ['kl', 'lr_multiplier', 'loss', 'entropy', 'explained_var_old', 'explained_var_new']
            assert np.isfinite([float(v) for v in fields.values()]).all(), ln
