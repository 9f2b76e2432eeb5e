"""The host side of the device replay buffer (rlzero_amd/replay.py; no GPU): the two symmetry tables against the reference's own
augmented output (g5_equi.npz) and against ReplayBuffer._entry, the sampler's counter-based draw, the trainer's new arguments."""
import numpy as np
import pytest

import replay_cases as rc
from rlzero_amd.replay import pack_positions, replay_index, replay_indices, symmetry_tables


def test_tables_reproduce_the_reference_fixture(g5):
    src_state, src_pi = symmetry_tables(4)
    assert src_state.shape == src_pi.shape == (8, 16) and src_state.dtype == src_pi.dtype == np.int16
    planes, pi = g5['state'].reshape(4, 16), g5['pi']
    for k in range(8):
        assert np.array_equal(planes[:, src_state[k]].reshape(4, 4, 4), g5['equi_states'][k]), k
        assert np.array_equal(pi[src_pi[k]], g5['equi_pis'][k]), k


@pytest.mark.parametrize('board', [3, 4, 15, 16])
def test_tables_are_two_different_permutations(board):
    A = board * board
    src_state, src_pi = symmetry_tables(board)
    for table in (src_state, src_pi):
        assert all(sorted(row.tolist()) == list(range(A)) for row in table)
        assert len({row.tobytes() for row in table}) == 8   # pairwise distinct
    assert not np.array_equal(src_state, src_pi)
    assert np.array_equal(src_state[6], np.arange(A))   # (four quarter turns)
    assert all(not np.array_equal(src_state[k], src_pi[k]) for k in (0, 1, 4, 5))   # (the reference's quirk: odd quarter turns)
    # both agree with the host buffer's entries on a random reachable position
    game = rc.random_game(board, min(A, 7), 0, seed=board)
    buf = rc.host_buffer([game], A, board)
    j = len(game.moves) - 1
    state, pi = np.asarray(game.states()[j]), np.asarray(game.pis[j])
    for k in range(8):
        want_state, want_pi, _ = buf[8 * j + k]
        assert np.array_equal(state.reshape(4, A)[:, src_state[k]].reshape(4, board, board), want_state), k
        assert np.array_equal(pi[src_pi[k]], want_pi), k


def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) % 2 ** 64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    return x ^ (x >> 31)


KNOWN = [((0, 0, 0, 8), 1), ((0, 0, 1, 8), 2), ((1, 2, 3, 1000), 169), ((123456789, 7, 4095, 296), 152),
         ((2 ** 63 + 5, 2 ** 40, 2 ** 33, 2 ** 31 - 1), 544110692), ((5, 1, 0, 1), 0)]


def test_replay_index_known_answers():
    for args, want in KNOWN:
        assert replay_index(*args) == want, args
        seed, step, i, n = args
        x = _splitmix(_splitmix(_splitmix(seed ^ int.from_bytes(b'replay\0\0', 'big')) ^ step) ^ i)   # the definition, in plain integers
        assert (x * n) >> 64 == want, args
    assert replay_indices(1, 2, 4, 1000).tolist() == [917, 680, 243, 169]


def test_replay_index_range_determinism_coverage():
    n = 8 * 37
    draws = replay_indices(3, 0, 65536, n)
    assert draws.dtype == np.int64 and draws.min() >= 0 and draws.max() < n
    assert len(set(draws.tolist())) == n                      # every entry is hit
    assert np.array_equal(draws, replay_indices(3, 0, 65536, n))
    assert not np.array_equal(draws[:64], replay_indices(3, 1, 64, n)) and not np.array_equal(draws[:64], replay_indices(4, 0, 64, n))
    for step in (0, 1, 5):
        vec = replay_indices(9, step, 1001, 777)
        assert [replay_index(9, step, i, 777) for i in (0, 1, 63, 1000)] == vec[[0, 1, 63, 1000]].tolist()
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError):
            replay_indices(0, 0, 1, bad)


def test_pack_positions_is_the_states_of_the_trajectory():
    """The raw record (two bitboards, meta word) holds what Trajectory.states() / z() define, dropped plies' stones included."""
    full = np.array([0, 1, 1, 0, 1, 1, 0], dtype=bool)
    game = rc.random_game(4, 7, 1, seed=2, full=full)
    stones, meta, pi = pack_positions([game], 4)
    kept = np.nonzero(full)[0]
    assert len(stones) == len(kept) and np.array_equal(pi, game.pis[kept].astype(np.float32))
    for rec, word, p in zip(stones, meta, kept):
        planes = game.states()[p]
        for side in range(2):
            cells = [c for c in range(16) if (int(rec[side][c >> 6]) >> (c & 63)) & 1]
            assert cells == np.nonzero(planes[side].reshape(-1))[0].tolist()
        assert (word & 511) == game.moves[p - 1] + 1 and ((word >> 9) & 1) == p % 2 and ((word >> 10) & 3) - 1 == game.z()[p]


def test_trainer_arguments():
    tr = rc.trainer()
    args = tr.parse_args([])
    assert (args.batch_size, args.updates_per_round, args.device_replay) == (32, 1, False)
    args = tr.parse_args(['--batch-size', '64', '--updates-per-round', '4'])
    assert (args.batch_size, args.updates_per_round) == (64, 4)
    with pytest.raises(SystemExit):
        tr.parse_args(['--device-replay'])
    for bad in (['--batch-size', '0'], ['--updates-per-round', '0']):
        with pytest.raises(SystemExit):
            tr.parse_args(bad)
    with pytest.raises(ValueError):
        tr.TrainPipeline(device_replay=True)   # (the reference flow: no games in flight)
    pipe = tr.TrainPipeline(board_size=3, n_in_row=3)
    assert pipe.batch_size == 32 and pipe.updates_per_round == 1 and not pipe.device_replay


def test_agent_takes_tensors():
    import torch
    from rlzero_amd.games.gomoku.alphazero_agent import AlphaZeroAgent
    agent = AlphaZeroAgent(3)
    states = np.random.RandomState(0).rand(5, 4, 3, 3)
    as_list = agent._tensor(list(states))
    as_tensor = agent._tensor(torch.from_numpy(states))
    assert as_tensor.dtype == torch.float32 and torch.equal(as_list, as_tensor)
    same = torch.zeros(2, 4, 3, 3)
    assert agent._tensor(same) is same   # (already float32 on the device: no copy)


def _entry_from_record(stones, word, pi, k, src_state, src_pi):
    """What k_replay_gather writes for symmetry k of one raw record, restated in numpy."""
    A = len(pi)
    bits = [np.array([(int(stones[side][c >> 6]) >> (c & 63)) & 1 for c in range(A)], dtype=np.float32) for side in range(2)]
    last = np.zeros(A, dtype=np.float32)
    if word & 511:
        last[(word & 511) - 1] = 1.0
    even = np.full(A, 0.0 if (word >> 9) & 1 else 1.0, dtype=np.float32)
    planes = np.stack([bits[0], bits[1], last, even])[:, src_state[k]]
    return planes, pi[src_pi[k]], np.float32(((word >> 10) & 3) - 1)


@pytest.mark.parametrize('board', [3, 15])
def test_records_and_tables_give_the_host_entries(board):
    """The record layout and the two tables carry everything: every entry of the host buffer follows from pack_positions + look-ups."""
    A = board * board
    full = np.ones(min(A, 30), dtype=bool)
    full[[0, 4]] = False
    games = [rc.random_game(board, min(A, 30), 1, seed=1, full=full), rc.random_game(board, 2, -1, seed=2), rc.random_game(board, A, 0, seed=3)]
    buf = rc.host_buffer(games, 10 ** 4, board)
    stones, meta, pis = pack_positions(games, board)
    src_state, src_pi = symmetry_tables(board)
    assert len(buf) == 8 * len(meta)
    for e in list(range(0, len(buf), 37)) + [len(buf) - 1]:
        j, k = divmod(e, 8)
        planes, pi, z = _entry_from_record(stones[j], int(meta[j]), pis[j], k, src_state, src_pi)
        want = buf[e]
        assert np.array_equal(planes.reshape(4, board, board), np.asarray(want[0], dtype=np.float32)), e
        assert np.array_equal(pi, np.asarray(want[1], dtype=np.float32)) and z == np.float32(want[2]), e
