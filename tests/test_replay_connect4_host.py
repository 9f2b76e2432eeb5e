"""The Connect4 device replay on the CPU: the two rules of rlzero_amd/csrc/rz_replay_rules.h that are Connect4's -- ``cell_of_ply``
(the cell a dropped stone comes to rest in: what k_replay_add<true> runs over the move list) and ``first_illegal_drop`` (what
rz_replay_add refuses before a launch) -- against ``Connect4Env.step``; the stored record as a root of the search engine against
``Connect4Env.from_bitboards`` for every ply (the last CELL lands in plane 2); ``symmetry_tables(..., game='connect4')`` against the
numpy expressions it stands for; the trainer's host ``ReplayBuffer`` and ``get_equi_data`` entry for entry; the trainer's options.
A driver with its own main is compiled against the header with ROCm's clang++, by
tests/host_driver.py, and once more with -fsanitize=address,undefined (a stand-alone program); every call runs both and holds their outputs
equal.  Nothing here touches a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import host_driver
import replay_cases as rc
import replay_connect4_cases as c4
from rlzero_amd import _hip
from rlzero_amd.games.connect4.connect4_env import Connect4Env
from rlzero_amd.replay import pack_positions, symmetry_tables
from rlzero_amd.selfplay import Trajectory

WORDS = _hip.BOARD_WORDS

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rz_replay_rules.h"

namespace rr = rzrr;

template <typename T>
static std::vector<T> load(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (bytes && fread(v.data(), 1, (size_t)bytes, f) != (size_t)bytes) exit(2);
    fclose(f);
    return v;
}
template <typename T>
static void store(const char *path, const std::vector<T> &v) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror(path); exit(2); }
    fclose(f);
}

constexpr int kRec = 2 * RZ_BOARD_WORDS;

// cells rows cols moves.i32 [plies of all games] offsets.i32 [G + 1] -> cells.i32 [plies] illegal.i32 [G]: every game's move list
// as a heap row of exactly its plies (a read past ply q or before ply 0 is the sanitizer's), cell_of_ply of every ply, and the
// first ply first_illegal_drop refuses (-1: none)
static int cells(char **a) {
    const int rows = atoi(a[0]), cols = atoi(a[1]);
    const std::vector<int32_t> moves = load<int32_t>(a[2]), offsets = load<int32_t>(a[3]);
    std::vector<int32_t> out(moves.size(), -1), illegal(offsets.size() - 1);
    for (size_t g = 0; g + 1 < offsets.size(); ++g) {
        const std::vector<int32_t> game(moves.begin() + offsets[g], moves.begin() + offsets[g + 1]);
        illegal[g] = rr::first_illegal_drop(game.data(), (int)game.size(), rows, cols);
        const int legal = illegal[g] < 0 ? (int)game.size() : illegal[g];
        for (int q = 0; q < legal; ++q) {
            const std::vector<int32_t> upto(game.begin(), game.begin() + q + 1);   // (plies 0 .. q and no more)
            out[offsets[g] + q] = rr::cell_of_ply(upto.data(), q, cols);
        }
    }
    store(a[4], out);
    store(a[5], illegal);
    return 0;
}

// roots records.u64 [R][2][W] meta.i32 [R] -> stones.u64 [R][2][W] to_move.i32 [R] last.i32 [R]
static int roots(char **a) {
    const std::vector<uint64_t> rec = load<uint64_t>(a[0]);
    const std::vector<int32_t> meta = load<int32_t>(a[1]);
    const size_t R = meta.size();
    if (rec.size() != R * kRec) return 4;
    std::vector<uint64_t> out(R * kRec, ~0ull);
    std::vector<int32_t> to_move(R), last(R);
    for (size_t r = 0; r < R; ++r) {
        const std::vector<uint64_t> one(rec.begin() + r * kRec, rec.begin() + (r + 1) * kRec);
        std::vector<uint64_t> root(kRec, ~0ull);
        rr::root_of_record(one.data(), meta[r], root.data(), &to_move[r], &last[r]);
        for (int j = 0; j < kRec; ++j) out[r * kRec + j] = root[j];
    }
    store(a[2], out);
    store(a[3], to_move);
    store(a[4], last);
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "cells" && argc == 8) return cells(argv + 2);
    if (what == "roots" && argc == 7) return roots(argv + 2);
    return 4;
}
'''


drv = host_driver.fixture('replay_connect4', DRIVER)


def _games(rows, cols, n_in_row):
    """A full board of random drops, one that fills column 0 to the top first, a short game, one ply, no ply."""
    board, cells = (rows, cols), rows * cols
    return [c4.random_game(board, cells, 0, seed=10 * rows + cols, game_id=0, n_in_row=n_in_row),
            c4.column_filler(board, seed=rows + cols, game_id=1, n_in_row=n_in_row),
            c4.random_game(board, min(cells, 7), 1, seed=3, game_id=2, n_in_row=n_in_row),
            c4.random_game(board, 1, -1, seed=4, game_id=3, n_in_row=n_in_row),
            c4.random_game(board, 0, -1, seed=5, game_id=4, n_in_row=n_in_row)]


def _flat(games):
    offsets = np.cumsum([0] + [len(t.moves) for t in games]).astype(np.int32)
    return np.array([m for t in games for m in t.moves], dtype=np.int32), offsets


# ----------------------------------------------------------------------------------------------- columns to cells
@pytest.mark.parametrize('rows, cols, n_in_row', c4.BOARDS)
def test_cell_of_ply_is_the_environment(drv, rows, cols, n_in_row):
    """Every ply of every game: the header's cell is the cell ``Connect4Env.step`` puts the stone in, and none of these legal games
    is refused.  (9, 8): the cells cross a 64-bit word; (4, 16): the widest board, 16 columns."""
    games = _games(rows, cols, n_in_row)
    moves, offsets = _flat(games)
    got, illegal = drv.run('cells', [rows, cols], [moves, offsets], [np.int32, np.int32])
    want = []
    for t in games:
        env = Connect4Env(rows, cols, n_in_row)
        for column in t.moves:
            env.step(column)
            want.append(env.last_cell)
    assert (illegal == -1).all()
    assert got.tolist() == want
    filler = got[offsets[1]:offsets[2]]
    assert filler[:rows].tolist() == [r * cols for r in range(rows)]                            # column 0 from the bottom to the top
    assert sorted(got[offsets[0]:offsets[1]].tolist()) == list(range(rows * cols))              # a full board: every cell once
    assert int(got.max()) == rows * cols - 1


def test_illegal_drops_are_named(drv):
    """A column outside the board, a negative one, a column played once more than the board has rows: the first such ply; the plies
    before it still have their cells."""
    rows, cols = 4, 5
    lists = [[0, 1, 5], [-1], [2, 2, 2, 2, 2], [0, 0, 0, 0, 1, 1, 1, 1, 0], [4, 4, 4, 4], [3, 16]]
    moves = np.array([m for ms in lists for m in ms], dtype=np.int32)
    offsets = np.cumsum([0] + [len(ms) for ms in lists]).astype(np.int32)
    got, illegal = drv.run('cells', [rows, cols], [moves, offsets], [np.int32, np.int32])
    assert illegal.tolist() == [2, 0, 4, 8, -1, 1]
    assert got[offsets[2]:offsets[3]].tolist() == [2, 7, 12, 17, -1] and got[offsets[4]:offsets[5]].tolist() == [4, 9, 14, 19]


# ----------------------------------------------------------------------------------------------- record to root
def _words(bits):
    return [(bits >> (64 * w)) & (2 ** 64 - 1) for w in range(WORDS)]


def _int(words):
    return sum(int(w) << (64 * i) for i, w in enumerate(words))


@pytest.mark.parametrize('rows, cols, n_in_row', c4.BOARDS)
def test_record_to_root_is_the_environment(drv, rows, cols, n_in_row):
    """Every ply of every game: the record ``pack_positions`` forms from the COLUMNS (dropping the stones in plain Python), pushed
    through the header, gives ``Connect4Env.from_bitboards`` the board of an environment stepped through the same moves -- the same
    ``current_state()``, whose plane 2 marks the last CELL --, the same side to move and the same legal columns."""
    games = _games(rows, cols, n_in_row)
    stones, meta, pis = pack_positions(games, (rows, cols), game='connect4')
    assert pis.shape == (sum(len(t.moves) for t in games), cols)
    got_stones, got_to_move, got_last = drv.run('roots', [], [stones, meta], [np.uint64, np.int32, np.int32])
    got_stones = got_stones.reshape(-1, 2, WORDS)
    i = 0
    for t in games:
        env = Connect4Env(rows, cols, n_in_row)
        for p, column in enumerate(t.moves):
            root = Connect4Env.from_bitboards(rows, cols, n_in_row, _int(got_stones[i, 0]), _int(got_stones[i, 1]), int(got_to_move[i]), int(got_last[i]))
            want = env.current_state()
            assert np.array_equal(root.current_state(), want), (t.game_id, p)
            assert got_to_move[i] == env.current_player() == p % 2 and got_last[i] == env.last_cell
            assert root.bitboards() == env.bitboards() and root.leagel_actions() == env.leagel_actions()
            if p:
                assert want[2].sum() == 1 and want[2].reshape(-1)[env.last_cell] == 1 and env.last_cell % cols == t.moves[p - 1]
            assert np.array_equal(pis[i], np.asarray(t.pis[p], dtype=np.float32))
            env.step(column)
            i += 1
    assert i == len(meta)
    used = [w for w in range(WORDS) if got_stones[:, :, w].any()]
    assert used == list(range((rows * cols + 63) // 64))                                        # every mask word the board has
    assert got_last[0] == -1 and got_to_move[:3].tolist() == [0, 1, 0]


def test_pack_positions_refuses_an_illegal_drop_and_keeps_gomoku():
    bad = Trajectory(0, (4, 5), 3, [1, 1, 1, 1, 1], np.full((5, 5), 0.2), -1, game='connect4')
    with pytest.raises(ValueError):
        pack_positions([bad], (4, 5), game='connect4')
    game = rc.random_game(6, 20, 0, seed=2)
    for a, b in zip(pack_positions([game], 6), pack_positions([game], 6, game='gomoku')):
        assert np.array_equal(a, b)
    assert pack_positions([game], 6)[2].shape == (20, 36)


# ----------------------------------------------------------------------------------------------- the symmetry tables
def _gomoku_tables_as_before(board_size):
    """``symmetry_tables`` of a square board as the code before the Connect4 buffer stated it."""
    size = int(board_size)
    cells = np.arange(size * size, dtype=np.int16)
    states, grids = cells.reshape(1, 1, size, size), cells.reshape(1, size, size)
    src_state, src_pi = [], []
    for k in range(8):
        quarter_turns, mirrored = k // 2 + 1, k % 2 == 1
        turned = np.rot90(states, quarter_turns, axes=(2, 3))
        pi_turned = np.rot90(grids[:, ::-1, :], quarter_turns, axes=(1, 2))
        if mirrored:
            src_state.append(np.ascontiguousarray(turned[:, :, :, ::-1]).reshape(-1))
            src_pi.append(np.ascontiguousarray(pi_turned[:, :, ::-1][:, ::-1, :]).reshape(-1))
        else:
            src_state.append(np.ascontiguousarray(turned).reshape(-1))
            src_pi.append(np.ascontiguousarray(pi_turned[:, ::-1, :]).reshape(-1))
    return np.stack(src_state).astype(np.int16), np.stack(src_pi).astype(np.int16)


@pytest.mark.parametrize('rows, cols, n_in_row', c4.BOARDS)
def test_symmetry_tables_are_the_mirror(rows, cols, n_in_row):
    src_state, src_pi = symmetry_tables((rows, cols), game='connect4')
    assert src_state.dtype == src_pi.dtype == np.int16 and src_state.shape == (2, rows * cols) and src_pi.shape == (2, cols)
    assert src_state[0].tolist() == list(range(rows * cols)) and src_pi[0].tolist() == list(range(cols))   # k = 0: as played
    assert np.array_equal(src_state[1][src_state[1]], src_state[0]) and np.array_equal(src_pi[1][src_pi[1]], src_pi[0])   # an involution
    rs = np.random.RandomState(rows * cols)
    planes, pi = rs.rand(4, rows, cols), rs.rand(cols)
    for k, (want_planes, want_pi) in enumerate(((planes, pi), (planes[:, :, ::-1], pi[::-1]))):
        assert np.array_equal(planes.reshape(4, -1)[:, src_state[k]].reshape(4, rows, cols), want_planes)
        assert np.array_equal(pi[src_pi[k]], want_pi)
    assert sorted(src_state[1].tolist()) == list(range(rows * cols))
    assert (src_state[1] // cols == src_state[0] // cols).all()                                   # a mirror keeps every stone's row


def test_gomoku_tables_are_unchanged():
    for board in (3, 6, 15):
        for got, want in zip(symmetry_tables(board), _gomoku_tables_as_before(board)):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        for got, want in zip(symmetry_tables(board, game='gomoku'), symmetry_tables(board)):
            assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        symmetry_tables(6, game='chess')


# ----------------------------------------------------------------------------------------------- the trainer's host buffer
def test_host_buffer_holds_the_samples_and_their_mirrors():
    """Entry 2 j + k of the trainer's ReplayBuffer: sample j of the games in order as played (k = 0) and mirrored (k = 1), through
    a maxlen that cuts the oldest entries off (an odd number of them); ``get_equi_data`` gives the same list."""
    tr = rc.trainer()
    board = (6, 7)
    full = np.ones(12, dtype=bool)
    full[[0, 5]] = False
    games = [c4.random_game(board, 9, 0, seed=1, game_id=0), c4.random_game(board, 12, 1, seed=2, game_id=1, full=full),
             c4.random_game(board, 42, -1, seed=3, game_id=2), c4.random_game(board, 1, 1, seed=4, game_id=3)]
    samples = [sm for t in games for sm in t.training_samples()]
    assert len(samples) == 9 + 10 + 42 + 1
    want = []
    for state, pi, z in samples:
        want.append((np.asarray(state), np.asarray(pi), z))
        want.append((np.asarray(state)[:, :, ::-1], np.asarray(pi)[::-1], z))
    assert sum(not np.array_equal(want[2 * j][0], want[2 * j + 1][0]) for j in range(len(samples))) > len(samples) // 2   # (the mirror moves stones)

    def same(got, expected):
        assert len(got) == len(expected)
        for (gs, gp, gz), (ws, wp, wz) in zip(got, expected):
            assert gs.shape == (4, 6, 7) and gp.shape == (7, )
            assert np.array_equal(gs, ws) and np.array_equal(gp, wp) and gz == wz
    buf = c4.host_buffer(games, 100, board)
    assert len(buf) == 2 * len(samples) and buf.n_symmetries == 2 and buf.maxlen == 200
    same(list(buf), want)
    same([buf[i] for i in range(len(buf))], want)
    same(buf[-3:], want[-3:])
    small = c4.host_buffer(games, 30, board)
    same(list(small), want[-60:])
    odd = tr.ReplayBuffer(61, board, game='connect4')                                           # (the first entry held is a mirror)
    for t in games:
        odd.extend_samples(t.training_samples())
    same(list(odd), want[-61:])
    pipe = tr.TrainPipeline(board_size=6, board_width=7, n_in_row=4, game='connect4', selfplay_games_in_flight=4, seed=0)
    same(pipe.get_equi_data(samples), want)
    assert pipe.get_equi_data([]) == []
    assert isinstance(pipe.data_buffer, tr.ReplayBuffer) and pipe.data_buffer.game == 'connect4'
    assert pipe.buffer_size == max(1000, 4 * 42 * 2) and (pipe.rows, pipe.cols, pipe.n_symmetries) == (6, 7, 2)
    assert pipe.alphazero_agent.policy_value_net(pipe.alphazero_agent._tensor([want[0][0]]))[0].shape == (1, 7)
    pipe.data_buffer.extend_samples(samples)
    same(list(pipe.data_buffer), want)
    # a Gomoku buffer is what it was: eight entries a sample
    gomoku = rc.host_buffer([rc.random_game(4, 5, 0, seed=1)], 10, 4)
    assert len(gomoku) == 40 and gomoku[0][0].shape == (4, 4, 4)


# ----------------------------------------------------------------------------------------------- the trainer's options
def test_the_trainer_refuses_connect4_outside_the_batched_mode_and_with_a_gate():
    script = os.path.join(REPO, 'tools', 'train_alphazero.py')
    for extra, message in (([], b'--game connect4 needs --games-in-flight > 0 (batched mode)'),
                           (['--games-in-flight', '8', '--gate-against', 'some.model'], b'--gate-against is a Gomoku option'),
                           (['--games-in-flight', '8', '--gpus', '2'], b'--game connect4 runs on one GPU')):
        run = subprocess.run([sys.executable, script, '--game', 'connect4'] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             env=dict(os.environ, PYTHONPATH=REPO))
        assert run.returncode == 2 and message in run.stderr and b'usage:' in run.stderr, run.stderr[-600:]
    run = subprocess.run([sys.executable, script, '--board-width', '7'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, PYTHONPATH=REPO))
    assert run.returncode == 2 and b'--board-width is a Connect4 option' in run.stderr
    tr = rc.trainer()
    with pytest.raises(ValueError, match='selfplay_games_in_flight must be > 0'):
        tr.TrainPipeline(board_size=6, n_in_row=4, game='connect4')
    with pytest.raises(ValueError, match='gate match'):
        tr.TrainPipeline(board_size=6, n_in_row=4, game='connect4', selfplay_games_in_flight=8, gate_against='some.model')
    with pytest.raises(ValueError):
        tr.TrainPipeline(board_size=6, n_in_row=4, game='chess')
    args = tr.parse_args(['--game', 'connect4', '--games-in-flight', '8'])
    assert (args.game, args.board, args.board_width, args.n_in_row) == ('connect4', 6, 7, 4)
    args = tr.parse_args(['--game', 'connect4', '--board', '4', '--board-width', '5', '--n-in-row', '3', '--games-in-flight', '8',
                          '--temperature-schedule', 'step:1.0:19:0.1'])
    assert (args.board, args.board_width, args.n_in_row) == (4, 5, 3)
    with pytest.raises(SystemExit):
        tr.parse_args(['--game', 'connect4', '--board', '4', '--board-width', '5', '--games-in-flight', '8', '--temperature-schedule', 'step:1.0:20:0.1'])


def test_gomoku_arguments_parse_as_before():
    """Without --game, and with --game gomoku, every option has the value it had: the defaults of the reference script's run."""
    tr = rc.trainer()
    base = vars(tr.parse_args([]))
    assert base.pop('game') == 'gomoku' and base.pop('board_width') is None
    assert base == dict(gpus=1, board=6, n_in_row=4, playouts=400, batches=64, check_freq=50, games_in_flight=0, seed=None,
                        resign_threshold='off', resign_disabled_frac=0.1, resign_fp_target=0.05, playout_cap=None, temperature_schedule=None,
                        pi_temperature=None, gate_against=None, batch_size=32, updates_per_round=1, device_replay=False, reanalyse=0,
                        reanalyse_slots=512, reanalyse_playouts=None)
    line = ['--board', '9', '--n-in-row', '5', '--games-in-flight', '16', '--playout-cap', '10:0.5', '--playouts', '50', '--gate-against', 'x.model',
            '--temperature-schedule', 'step:1.0:80:0.1']
    assert vars(tr.parse_args(line)) == vars(tr.parse_args(['--game', 'gomoku'] + line))
    pipe = tr.TrainPipeline(board_size=3, n_in_row=3)
    assert pipe.game_kind == 'gomoku' and pipe.board_size == 3 and pipe.buffer_size == 1000 and pipe.data_buffer.n_symmetries == 8
    with pytest.raises(ValueError):
        tr.TrainPipeline(board_size=3, n_in_row=3, board_width=4)
