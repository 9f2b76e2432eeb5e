"""The device replay buffer for Connect4 (rz_replay_create_game, rz_replay_set_tables_game; DeviceReplay(game='connect4')) against the
trainer's host ReplayBuffer(game='connect4'): after the same games DeviceReplay((rows, cols), C) holds the entries of
ReplayBuffer(2 C, (rows, cols)) fed training_samples() -- entry 2 j + k, every index, bit for bit as float32 -- through ring
wrap-around, several add calls and playout-cap gaps; the raw records are pack_positions (stones dropped in plain Python); the
device draw is replay_indices over 2 x positions; misuse raises.  Reanalyse: the refreshed rows are reanalysed_pi of the visit counts
of an INDEPENDENT MCTSEngine(game='connect4') given the same roots through the host set_roots.  The learner takes the gathered
tensors, and the trainer runs end to end with either buffer and with Reanalyse."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import REPO

import replay_cases as rc
import replay_connect4_cases as c4

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SLOTS, SEED, PLAYOUTS = 8, 11, 32


def _replay(board, capacity, **kw):
    from rlzero_amd.replay import DeviceReplay
    return DeviceReplay(board, capacity, device=DEV, game='connect4', **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_as_host(dr, buf, what=''):
    """Every entry of the device buffer against the host buffer's, bit for bit."""
    assert len(dr) == len(buf) == 2 * dr.positions, what
    if len(buf) == 0:
        return
    got = [x.cpu().numpy() for x in dr.gather(np.arange(len(buf)))]
    rows, cols = dr.board_size
    assert got[0].shape == (len(buf), 4, rows, cols) and got[1].shape == (len(buf), cols) and got[2].shape == (len(buf), )
    for g, w, name in zip(got, rc.host_entries(buf), ('states', 'pis', 'zs')):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, name)
        assert np.array_equal(_bits(g), _bits(w)), (what, name)


@pytest.mark.parametrize('rows, cols, n_in_row', c4.BOARDS)
def test_every_entry_of_games_of_every_length(rows, cols, n_in_row):
    """Games of 0, 1, 2, ... rows * cols plies (random legal drops, random pi rows), winners 0 / 1 / tie in turn, and one that fills a
    column to the top first: every entry is the host buffer's, every record pack_positions'.  (9, 8): 72 cells, two waves of
    threads and two mask words; (4, 16): the widest pi row; (4, 5): 20 cells, a partial wave."""
    from rlzero_amd.replay import pack_positions
    board, cells = (rows, cols), rows * cols
    games = [c4.random_game(board, plies, (0, 1, -1)[plies % 3], seed=1000 * rows + plies, game_id=plies, n_in_row=n_in_row) for plies in range(cells + 1)]
    games.append(c4.column_filler(board, seed=rows, game_id=cells + 1, n_in_row=n_in_row))
    capacity = sum(len(t.moves) for t in games) + 3
    dr = _replay(board, capacity)
    assert len(dr) == 0 and (dr.n_cells, dr.n_actions, dr.n_symmetries) == (cells, cols, 2)
    assert dr.src_state.shape == (2, cells) and dr.src_pi.shape == (2, cols)
    assert dr.add(games) == capacity - 3
    _same_as_host(dr, c4.host_buffer(games, capacity, board), board)
    for g, w in zip(dr.read(), pack_positions(games, board, game='connect4')):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    dr.close()


@pytest.mark.parametrize('capacity', [100, 20, 12, 7, 5])
def test_ring(capacity):
    """A capacity larger than all games, one equal to the longest game, one a game straddles the end of, a prime one, one smaller
    than most games (more kept plies than slots in ONE add: the last plies remain); several add calls of several games against one
    add of all, compared with the host buffer after every call."""
    board = (4, 5)
    games = [c4.random_game(board, plies, winner, seed=7 + i, game_id=i, n_in_row=3)
             for i, (plies, winner) in enumerate([(10, 0), (12, 1), (9, -1), (20, 0), (1, 1), (7, 0)])]
    calls = [games[:2], games[2:3], games[3:6]]
    split, whole = _replay(board, capacity), _replay(board, capacity)
    done = []
    for call in calls:
        split.add(call)
        done += call
        _same_as_host(split, c4.host_buffer(done, capacity, board), (capacity, len(done)))
    whole.add(games)
    _same_as_host(whole, c4.host_buffer(games, capacity, board), capacity)
    assert len(split) == len(whole) == 2 * min(capacity, 59)
    for a, b in zip(split.read(), whole.read()):
        assert np.array_equal(a, b)
    split.close()
    whole.close()


def test_playout_cap_gaps():
    """A `full` mask with gaps, ply 0 and the last ply dropped: the held entries are training_samples(), and the stones of dropped
    plies are on the later boards."""
    board = (9, 8)
    full = np.ones(70, dtype=bool)
    full[[0, 3, 4, 63, 64, 69]] = False
    capped = c4.random_game(board, 70, 1, seed=5, game_id=0, full=full)
    resigned = c4.random_game(board, 6, 0, seed=6, game_id=1, full=[True, False, True, True, False, True, True])   # (one flag more than plies)
    games = [capped, resigned]
    dr = _replay(board, 200)
    assert dr.add(games) == 64 + 4 == sum(len(t.training_samples()) for t in games)
    _same_as_host(dr, c4.host_buffer(games, 200, board))
    states, _, _ = dr.gather([2 * 0 + 0])   # the first kept ply (ply 1) as played
    planes = states[0].cpu().numpy().reshape(4, -1)
    cell = capped.moves[0]                  # (the first stone lies in row 0: its cell is its column)
    assert planes[1].sum() == 1 and planes[1][cell] == 1 and planes[0].sum() == 0   # the dropped ply 0's stone: the opponent's
    assert planes[2][cell] == 1 and planes[3].sum() == 0
    mirrored, _, _ = dr.gather([2 * 0 + 1])
    assert mirrored[0].cpu().numpy().reshape(4, -1)[1][board[1] - 1 - cell] == 1
    dr.close()


def test_sample_is_the_host_draw():
    import torch
    from rlzero_amd.replay import replay_indices
    board, seed = (6, 7), 11
    games = [c4.random_game(board, 30 + i, i % 2, seed=30 + i, game_id=i) for i in range(3)]
    dr = _replay(board, 50, seed=seed)   # (the ring has wrapped: 93 positions)
    dr.add(games)
    assert dr.positions == 50 and len(dr) == 100
    n = 300

    def same(got, want):
        return all(torch.equal(g, w) for g, w in zip(got, want))
    step3 = dr.sample(n, step=3)
    assert same(step3, dr.gather(replay_indices(seed, 3, n, 2 * dr.positions)))
    assert same(step3, dr.sample(n, step=3))                    # the same step repeats
    assert not same(step3, dr.sample(n, step=4))                # two steps differ
    first, second = dr.sample(n), dr.sample(n)                  # the internal counter: steps 0, 1
    assert same(first, dr.gather(replay_indices(seed, 0, n, len(dr)))) and same(second, dr.sample(n, step=1)) and dr.step == 2
    idx = replay_indices(seed, 3, n, len(dr))
    assert idx.max() >= 90 and (idx % 2).min() == 0 and (idx % 2).max() == 1   # (both symmetries, up to the newest positions)
    assert same(step3, dr.gather(torch.from_numpy(idx).to(DEV)))
    assert [tuple(x.shape) for x in step3] == [(n, 4, 6, 7), (n, 7), (n, )]
    dr.close()


def test_misuse_raises():
    import torch
    from rlzero_amd import _hip
    from rlzero_amd._hip import HipError
    from rlzero_amd.selfplay import Trajectory
    for board in ((0, 7), (6, 17), (17, 7)):
        with pytest.raises(HipError):
            _replay(board, 10)
    with pytest.raises(HipError):
        _replay((6, 7), 0)
    dr = _replay((4, 5), 10)
    with pytest.raises(HipError):
        dr.sample(4)                                            # empty
    with pytest.raises(HipError):
        dr.gather([0])
    with pytest.raises(ValueError):
        dr.add([rc.random_game(4, 3, 0, seed=1)])               # a Gomoku game
    with pytest.raises(ValueError):
        dr.add([c4.random_game((6, 7), 3, 0, seed=1)])          # another board
    with pytest.raises(ValueError):
        dr.add([c4.random_game((5, 4), 3, 0, seed=1)])          # ... with the same number of cells
    with pytest.raises(HipError):
        dr.add([Trajectory(0, (4, 5), 3, [5], np.full((1, 5), 0.2), 0, game='connect4')])                 # a column >= cols
    with pytest.raises(HipError):
        dr.add([Trajectory(0, (4, 5), 3, [0, 2, -1], np.full((3, 5), 0.2), 0, game='connect4')])
    with pytest.raises(HipError):
        dr.add([Trajectory(0, (4, 5), 3, [2, 2, 2, 2, 2], np.full((5, 5), 0.2), 0, game='connect4')])     # a column played more than `rows` times
    with pytest.raises(HipError):
        dr.add([c4.random_game((4, 5), 3, 0, seed=1, game_id=0), Trajectory(1, (4, 5), 3, [1, 3, 3, 3, 3, 3], np.full((6, 5), 0.2), 0, game='connect4')])
    assert len(dr) == 0 and dr.ticket == 0                      # (a refused add stores nothing, its legal games included)
    with pytest.raises(HipError):                               # Gomoku's [8][A] upload is not this buffer's
        _hip.check(dr.lib.rz_replay_set_tables(dr.handle, ctypes.c_void_p(dr.src_state.ctypes.data), ctypes.c_void_p(dr.src_pi.ctypes.data), dr._stream()), 'rz_replay_set_tables')
    with pytest.raises(HipError):                               # ... nor are tables of other sizes
        _hip.check(dr.lib.rz_replay_set_tables_game(dr.handle, 2, 20, 4, ctypes.c_void_p(dr.src_state.ctypes.data), ctypes.c_void_p(dr.src_pi.ctypes.data),
                                                    dr._stream()), 'rz_replay_set_tables_game')
    dr.add([c4.random_game((4, 5), 5, 0, seed=2, n_in_row=3)])
    assert len(dr) == 10
    for bad in ([10], [-1], [0, 9, 10]):
        with pytest.raises(HipError):
            dr.gather(bad)
        with pytest.raises(HipError):
            dr.gather(torch.tensor(bad, dtype=torch.int64, device=DEV))
    states, pis, zs = dr.gather(torch.tensor([9, 0], dtype=torch.int64, device=DEV))   # (the flag does not linger)
    assert states.shape == (2, 4, 4, 5) and float(pis.sum()) == pytest.approx(2.0, abs=1e-5)
    # a bad device index: the flag, and nothing written for that entry while its neighbours are
    idx = torch.tensor([3, 10, 4, -7], dtype=torch.int64, device=DEV)
    outs = [torch.full((4, 4, 4, 5), -5.0, device=DEV), torch.full((4, 5), -5.0, device=DEV), torch.full((4, ), -5.0, device=DEV)]
    _hip.check(dr.lib.rz_replay_gather(dr.handle, None, idx.data_ptr(), 4, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), dr._stream()), 'rz_replay_gather')
    assert dr.poll_errors() == _hip.REPLAY_BAD_INDEX and dr.poll_errors() == 0
    good = dr.gather([3, 4])
    for out, want in zip(outs, good):
        assert (out[[1, 3]] == -5.0).all().item() and torch.equal(out[[0, 2]], want)
    dr.close()


# ----------------------------------------------------------------------------------------------- Reanalyse
def _net(board, seed):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(seed)
    return PolicyValueNet(board[0], board[1], board[1])


def _roots_of_records(stones, meta):
    """The record-to-root rule in numpy: stones by player, side to move, last CELL."""
    parity = (meta >> 9) & 1
    by_player = np.where(parity[:, None, None] == 0, stones, stones[:, ::-1, :])
    return np.ascontiguousarray(by_player), parity.astype(np.int32), ((meta & 511) - 1).astype(np.int32)


def _oracle_pi(net, board, n_in_row, records):
    """reanalysed_pi of the visit counts an independent Connect4 engine finds for every position of ``records`` (pack_positions'),
    eight at a time through the host ``set_roots`` -> float32 [n, cols]."""
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    from rlzero_amd.replay import reanalysed_pi
    stones, to_move, last = _roots_of_records(records[0], records[1])
    n = len(to_move)
    eng = MCTSEngine(board, n_in_row, n_games=SLOTS, n_playout=PLAYOUTS, device=DEV, add_noise=False, game='connect4')
    ev = HipNetEvaluator(net, (board[0], board[1], board[1]), DEV, max_boards=SLOTS)
    out = []
    for a in range(0, n, SLOTS):
        m = min(SLOTS, n - a)
        s, t, l = np.zeros((SLOTS, 2, stones.shape[2]), np.uint64), np.zeros(SLOTS, np.int32), np.full(SLOTS, -1, np.int32)
        s[:m], t[:m], l[:m] = stones[a:a + m], to_move[a:a + m], last[a:a + m]
        eng.set_roots(s, t, l, reset_trees=True)
        eng.set_active((np.arange(SLOTS) < m).astype(np.uint8))
        eng.simulate(ev, PLAYOUTS)
        out.append(eng.root_visits()[:m].copy())
    eng.check()
    eng.close()
    ev.hip.close()
    visits = np.concatenate(out)
    assert visits.shape == (n, board[1])
    pi, written = reanalysed_pi(visits)
    assert written.all()
    return pi


def _holds(dr, records, expected_pi, what):
    """The buffer holds ``records``' stones and meta words bit for bit, and ``expected_pi``."""
    stones, meta, pi = dr.read()
    assert np.array_equal(stones, records[0]) and np.array_equal(meta, records[1]), what
    differ = np.nonzero((_bits(pi) != _bits(expected_pi)).any(axis=1))[0]
    assert differ.size == 0, (what, differ.tolist())


@pytest.mark.parametrize('rows, cols, n_in_row', [(6, 7, 4), (4, 5, 3)])
def test_reanalyse_is_a_fresh_search_of_the_stored_position(rows, cols, n_in_row):
    """A wrapped ring, duplicate indices, a padded last chunk, device indices, a stale ticket, and new weights: the refreshed rows
    are the independent engine's, everything else stays bit-identical.  The games complete no line (a stored position is never
    terminal) and their pi rows are random, so a refreshed row cannot equal a stored one by accident."""
    import torch
    from rlzero_amd._hip import HipError
    from rlzero_amd.replay import ReplayReanalyser, pack_positions
    board = (rows, cols)
    games = [c4.random_game(board, rows * cols, -1, seed=100 * rows + g, game_id=g, n_in_row=n_in_row, avoid_lines=True) for g in range(3)]
    kept = sum(len(t.moves) for t in games)
    capacity = kept - 5
    assert capacity >= 2 * SLOTS + 4 and min(len(t.moves) for t in games) > 5
    dr = _replay(board, capacity, seed=SEED)
    for t in games:
        dr.add([t])
    count, cursor, cap = dr._state()
    assert (count, cap) == (capacity, capacity) and cursor % cap != 0 and dr.ticket == kept   # wrapped: position 0 is not in slot 0
    records = tuple(x[-capacity:] for x in pack_positions(games, board, game='connect4'))
    for g, w in zip(dr.read(), records):
        assert np.array_equal(g, w)
    net = _net(board, seed=rows)
    want = _oracle_pi(net, board, n_in_row, records)
    choice = (records[2] > 0).sum(axis=1) > 1                    # (one open column: the stored and the searched row are both its one-hot)
    assert choice.sum() >= capacity - 3 and not (_bits(want) == _bits(records[2])).all(axis=1)[choice].any()
    expected = records[2].copy()
    ra = ReplayReanalyser(net, dr, n_in_row, PLAYOUTS, slots=SLOTS, seed=SEED)
    assert ra.engine.game == 'connect4' and ra.engine.n_actions == cols

    # 13 host indices: one full chunk and a padded one, position 5 once in each; the newest and the oldest position
    idx = np.array([capacity - 1, 3, 17, 5, 14, 0, 10, 9, 12, 5, 15, 1, 16])
    assert ra.reanalyse(idx) == 13 and ra.positions_done == 13 and ra.sims_done == 13 * PLAYOUTS
    expected[idx] = want[idx]
    _holds(dr, records, expected, 'host indices')
    ra.check()

    # both symmetries of a refreshed position share the new row
    _, pis, _ = dr.gather(2 * 5 + np.arange(2))
    pis = pis.cpu().numpy()
    assert np.array_equal(_bits(pis[0]), _bits(want[5])) and np.array_equal(_bits(pis[1]), _bits(want[5][::-1]))

    # indices in a device tensor: the same result; one out of range raises and nothing is refreshed
    on_device = np.array([2, 7, capacity - 2, 5])
    assert ra.reanalyse(torch.from_numpy(on_device).to(DEV)) == 4
    expected[on_device] = want[on_device]
    _holds(dr, records, expected, 'device indices')
    with pytest.raises(HipError):
        ra.reanalyse(torch.tensor([4, capacity, 6], dtype=torch.int64, device=DEV))
    _holds(dr, records, expected, 'a bad device index')

    # other weights loaded into the module: after refresh_weights() the rows follow them
    late = np.arange(capacity - 8, capacity)
    net.load_state_dict(_net(board, seed=rows + 50).state_dict())
    ra.refresh_weights()
    assert ra.reanalyse(late) == 8
    want2 = _oracle_pi(net, board, n_in_row, records)
    expected[late] = want2[late]
    _holds(dr, records, expected, 'changed weights')
    assert (_bits(want2) != _bits(want)).any()

    # the ticket: an add between positions and update_pi, and the result has no home
    where, _, _, last_move, ticket = dr.position_roots([1, 2], pad_to=SLOTS)
    assert ticket == dr.ticket and (where[2:] == -1).all().item() and (where[:2] >= 0).all().item()
    assert last_move[:2].cpu().tolist() == [int((m & 511) - 1) for m in records[1][1:3]]   # (the last CELL)
    visits = torch.ones((SLOTS, cols), dtype=torch.int32, device=DEV)
    dr.add([c4.random_game(board, 3, 0, seed=5, game_id=9, n_in_row=n_in_row)])
    snap = dr.read()
    with pytest.raises(HipError, match='stale ticket'):
        dr.update_pi(where, visits, ticket)
    for a, b in zip(dr.read(), snap):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # ... and with the current ticket only the named rows change (one wave of threads sums a row of `cols` counts)
    where, _, _, _, ticket = dr.position_roots([1, 4], pad_to=SLOTS)
    visits[1, :3] = torch.tensor([-7, 3, 1], dtype=torch.int32)
    dr.update_pi(where, visits, ticket)
    now = dr.read()
    assert np.array_equal(now[0], snap[0]) and np.array_equal(now[1], snap[1])
    uniform = np.full(cols, np.float32(1.0 / cols))
    spiked = np.full(cols, np.float32(1.0 / (cols + 1)))
    spiked[:2] = [0.0, np.float32(3.0 / (cols + 1))]
    assert np.array_equal(_bits(now[2][1]), _bits(uniform)) and np.array_equal(_bits(now[2][4]), _bits(spiked))
    others = np.setdiff1d(np.arange(capacity), [1, 4])
    assert np.array_equal(_bits(now[2][others]), _bits(snap[2][others]))
    with pytest.raises(ValueError):
        dr.update_pi(where, torch.ones((SLOTS, rows * cols), dtype=torch.int32, device=DEV), ticket)   # (a row per CELL is Gomoku's)
    ra.check()
    ra.close()
    dr.close()


def test_learner_takes_the_gathered_tensors():
    from rlzero_amd.games.gomoku.alphazero_agent import AlphaZeroAgent
    board = (6, 7)
    dr = _replay(board, 100)
    dr.add([c4.random_game(board, 20 + i, i % 2, seed=50 + i, game_id=i) for i in range(3)])
    agent = AlphaZeroAgent(6, device=DEV, board_width=7, n_actions=7)
    batch = dr.sample(32)
    assert agent._tensor(batch[0]) is batch[0]
    loss, entropy = agent.learn(*batch)
    assert np.isfinite([loss, entropy]).all()
    dr.close()


@pytest.mark.parametrize('extra', [[], ['--device-replay'], ['--device-replay', '--reanalyse', '16', '--reanalyse-slots', '8']],
                         ids=['host-buffer', 'device-replay', 'reanalyse'])
def test_trainer_end_to_end(tmp_path, extra):
    cmd = [sys.executable, os.path.join(REPO, 'tools', 'train_alphazero.py'), '--game', 'connect4', '--board', '4', '--board-width', '5', '--n-in-row', '3',
           '--games-in-flight', '8', '--playouts', '16', '--batches', '2', '--check-freq', '2', '--seed', '1'] + extra
    env = dict(os.environ, PYTHONPATH=REPO)
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(('batch i:', 'kl:', 'current self-play batch:', 'num_playouts:'))]
    assert [ln.split(':')[0] for ln in lines] == ['batch i', 'kl', 'batch i', 'kl', 'current self-play batch', 'num_playouts'], out.stdout[-2000:]
    for ln in lines:
        if ln.startswith('kl:'):
            fields = dict(f.split(':') for f in ln.split(','))
            assert list(fields) == ['kl', 'lr_multiplier', 'loss', 'entropy', 'explained_var_old', 'explained_var_new']
            assert np.isfinite([float(v) for v in fields.values()]).all(), ln
