"""Reanalyse for the AlphaZero device replay on the CPU: the rules of rlzero_amd/csrc/rz_replay_rules.h that k_replay_positions and
k_replay_update_pi call -- a stored record as a root of the search engine, the pi row of fresh visit counts, the draws of a refresh,
the slot of a position and the ticket -- against their Python statements: ``pack_positions`` plus ``GomokuEnv`` stepped through the
same moves, ``reanalysed_pi`` (bit for bit), ``replay_reanalyse_draws`` (Python integers), and, for the documented deviation, the
reference's pi expression at T = 1 (``batch_pi_and_moves``) within a bound derived below.  A driver with its own main is compiled
against the header with ROCm's clang++, by
tests/host_driver.py, and once more with
-fsanitize=address,undefined (a stand-alone program); every call runs both and holds their outputs equal.  The trainer's options
are refused by the parser where they make no sense; nothing here touches a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import host_driver
from host_driver import CSRC
from rlzero_amd import _hip
from rlzero_amd.games.gomoku.gomoku_env import GomokuEnv
from rlzero_amd.replay import pack_positions, reanalysed_pi, replay_index, replay_reanalyse_draws
from rlzero_amd.selfplay import Trajectory, batch_pi_and_moves
from test_mz_replay_host import same_bits

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

// roots records.u64 [R][2][W] meta.i32 [R] -> stones.u64 [R][2][W] to_move.i32 [R] last.i32 [R]; the whole record, and once more
// word by word as the kernel's threads place it
static int roots(char **a) {
    const std::vector<uint64_t> rec = load<uint64_t>(a[0]);
    const std::vector<int32_t> meta = load<int32_t>(a[1]);
    const size_t R = meta.size();
    if (rec.size() != R * kRec) return 4;
    std::vector<uint64_t> out(R * kRec, ~0ull), by_word(R * kRec, ~0ull);
    std::vector<int32_t> to_move(R), last(R);
    for (size_t r = 0; r < R; ++r) {
        const std::vector<uint64_t> one(rec.begin() + r * kRec, rec.begin() + (r + 1) * kRec);   // (a heap row of exactly one record)
        std::vector<uint64_t> root(kRec, ~0ull);
        rr::root_of_record(one.data(), meta[r], root.data(), &to_move[r], &last[r]);
        for (int j = 0; j < kRec; ++j) {
            out[r * kRec + j] = root[j];
            by_word.at(r * kRec + rr::root_word(meta[r], j)) = one[j];
        }
    }
    if (out != by_word) return 5;
    store(a[2], out);
    store(a[3], to_move);
    store(a[4], last);
    return 0;
}

// pi A visits.i32 [R][A] -> pi.f32 [R][A] (rows that are not written keep -1) written.i32 [R] sum.i64 [R]
static int pi(char **a) {
    const int A = atoi(a[0]);
    const std::vector<int32_t> in = load<int32_t>(a[1]);
    const size_t R = in.size() / A;
    std::vector<float> out(R * A, -1.0f);
    std::vector<int32_t> written(R);
    std::vector<int64_t> sums(R);
    for (size_t r = 0; r < R; ++r) {
        const std::vector<int32_t> row(in.begin() + r * A, in.begin() + (r + 1) * A);   // (a heap row of exactly A counts)
        const int64_t sum = rr::visit_sum(row.data(), A);
        sums[r] = sum;
        written[r] = sum != 0;
        if (sum == 0) continue;
        for (int c = 0; c < A; ++c) out[r * A + c] = rr::pi_of_visits(row[c], sum);
    }
    store(a[2], out);
    store(a[3], written);
    store(a[4], sums);
    return 0;
}

// draws seed step n positions -> i64 [n]
static int draws(char **a) {
    const uint64_t seed = strtoull(a[0], nullptr, 10), step = strtoull(a[1], nullptr, 10);
    const int n = atoi(a[2]);
    const uint64_t positions = strtoull(a[3], nullptr, 10);
    std::vector<int64_t> out((size_t)n);
    for (int i = 0; i < n; ++i) out[i] = rr::reanalyse_position(seed, step, (uint64_t)i, positions);
    store(a[4], out);
    return 0;
}

// slots oldest count capacity index.i64 [R] -> slot.i64 [R]
static int slots(char **a) {
    const int64_t oldest = atoll(a[0]), count = atoll(a[1]), capacity = atoll(a[2]);
    const std::vector<int64_t> index = load<int64_t>(a[3]);
    std::vector<int64_t> out(index.size());
    for (size_t r = 0; r < index.size(); ++r) out[r] = rr::slot_of_position(index[r], oldest, count, capacity);
    store(a[4], out);
    return 0;
}

// tickets pairs.i64 [R][2] (ticket, stored) -> current.i32 [R]
static int tickets(char **a) {
    const std::vector<int64_t> in = load<int64_t>(a[0]);
    std::vector<int32_t> out(in.size() / 2);
    for (size_t r = 0; r < out.size(); ++r) out[r] = rr::ticket_current(in[2 * r], in[2 * r + 1]) ? 1 : 0;
    store(a[1], out);
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "roots" && argc == 7) return roots(argv + 2);
    if (what == "pi" && argc == 7) return pi(argv + 2);
    if (what == "draws" && argc == 7) return draws(argv + 2);
    if (what == "slots" && argc == 7) return slots(argv + 2);
    if (what == "tickets" && argc == 4) return tickets(argv + 2);
    return 4;
}
'''


drv = host_driver.fixture('replay_reanalyse', DRIVER)


def test_the_header_has_no_hip_include():
    with open(os.path.join(CSRC, 'rz_replay_rules.h')) as f:
        text = f.read()
    assert 'hip/' not in text and '#include "rz_host.h"' not in text
    # (the header as the main file of a plain C++ compiler: it parses alone)
    subprocess.run(host_driver.compile_command('-fsyntax-only', '-Wno-pragma-once-outside-header', '-x', 'c++', os.path.join(CSRC, 'rz_replay_rules.h')),
                   check=True)
    with open(os.path.join(CSRC, 'rz_replay.hip')) as f:
        assert '#include "rz_replay_rules.h"' in f.read()


# ----------------------------------------------------------------------------------------------- record to root
def _words(bits):
    return [(bits >> (64 * w)) & (2 ** 64 - 1) for w in range(WORDS)]


def _move_lists(board, rs):
    """A few legal games: one of every cell in ascending order (the last move reaches the last cell), one in descending order, a
    seeded shuffle of the whole board, a short one."""
    A = board * board
    return [list(range(A)), list(range(A - 1, -1, -1)), rs.permutation(A).tolist(), rs.permutation(A)[:7].tolist()]


@pytest.mark.parametrize('board, n_in_row', [(6, 4), (11, 5), (16, 5)])
def test_record_to_root_is_the_environment(drv, board, n_in_row):
    """Every ply of every game: the record ``pack_positions`` forms, pushed through the header, is the board of a GomokuEnv stepped
    through the same moves -- stones by PLAYER, side to move, last move.  (Lines are not judged here: an environment past a win
    still places stones, and the record holds no more than stones.)  6 x 6: one mask word; 11 x 11: two; 16 x 16: four, with
    the last move up to cell 255."""
    A = board * board
    rs = np.random.RandomState(board)
    games = [Trajectory(g, board, n_in_row, moves, np.full((len(moves), A), 1.0 / A), -1) for g, moves in enumerate(_move_lists(board, rs))]
    stones, meta, _ = pack_positions(games, board)
    got_stones, got_to_move, got_last = drv.run('roots', [], [stones, meta], [np.uint64, np.int32, np.int32])
    got_stones = got_stones.reshape(-1, 2, WORDS)
    want_stones, want_to_move, want_last = [], [], []
    for t in games:
        env = GomokuEnv(board, n_in_row)
        env.reset()
        for p, move in enumerate(t.moves):
            by_player = [0, 0]
            for cell, player in env.states.items():
                by_player[player] |= 1 << cell
            want_stones.append([_words(by_player[0]), _words(by_player[1])])
            want_to_move.append(env.current_player())
            want_last.append(env.last_move)
            env.step(move)
    want_stones = np.array(want_stones, dtype=np.uint64)
    assert got_stones.shape == want_stones.shape == (sum(len(t.moves) for t in games), 2, WORDS)
    assert np.array_equal(got_stones, want_stones)
    assert np.array_equal(got_to_move, np.array(want_to_move, dtype=np.int32))
    assert np.array_equal(got_last, np.array(want_last, dtype=np.int32))
    assert got_last[0] == -1 and got_to_move[:3].tolist() == [0, 1, 0]
    assert int(got_last.max()) == A - 1                                                         # (16 x 16: cell 255, nine bits of meta)
    used = [w for w in range(WORDS) if got_stones[:, :, w].any()]
    assert used == list(range((A + 63) // 64))                                                  # every mask word the board has


# ----------------------------------------------------------------------------------------------- pi of visits
PI_CASES = {
    4: [[0, 7, 0, 0], [3, 3, 3, 3], [-5, 2, -1, 2], [0, 0, 0, 0], [-1, -2, -3, 0], [2 ** 31 - 1, 1, 0, 0], [2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1],
        [2 ** 30, 2 ** 30, 0, 1], [1, 2, 3, 4], [-2 ** 31, 1, 0, 0]],
    36: None, 225: None, 256: None,
}


@pytest.mark.parametrize('A', sorted(PI_CASES))
def test_pi_of_visits_is_reanalysed_pi(drv, A):
    """One visited child (exactly 1.0), all children equal, negative entries (count as 0), a zero sum (no write), sums near and
    past 2^31 (int64, exact) -- and random rows: the header's bits are ``reanalysed_pi``'s."""
    rs = np.random.RandomState(A)
    rows = PI_CASES[A]
    if rows is None:
        one = [0] * A
        one[A // 2] = 800
        rows = [one, [3] * A, [0] * A, [2 ** 31 - 1] * A, [(-1) ** a * (a + 1) for a in range(A)]]
    vis = np.concatenate((np.array(rows, dtype=np.int64).astype(np.int32), rs.randint(-3, 60, size=(64, A)).astype(np.int32)))
    got, written, sums = drv.run('pi', [A], [vis], [np.float32, np.int32, np.int64])
    got = got.reshape(-1, A)
    want, want_written = reanalysed_pi(vis)
    assert np.array_equal(written != 0, want_written)
    assert same_bits(got[want_written], want[want_written])
    assert (got[~want_written] == -1.0).all() and (~want_written).sum() >= 1                    # a zero sum: nothing is written
    assert np.array_equal(sums, np.maximum(vis.astype(np.int64), 0).sum(axis=1))               # the exact integer
    assert got[0].max() == 1.0 and np.count_nonzero(got[0]) == 1                                # one visited child
    assert (got[1] == np.float32(1.0 / A)).all()                                                # all equal
    if A == 4:
        assert got[2].tolist() == [0.0, 0.5, 0.0, 0.5] and written[4] == 0 and sums[6] == 4 * (2 ** 31 - 1) > 2 ** 31
        assert got[5].tolist() == [np.float32((2 ** 31 - 1) / 2 ** 31), np.float32(1 / 2 ** 31), 0.0, 0.0]
        assert got[9].tolist() == [0.0, 1.0, 0.0, 0.0]
    # every written row is a distribution up to the casts
    assert np.abs(got[want_written].astype(np.float64).sum(axis=1) - 1.0).max() <= A * 2.0 ** -25


def test_distance_from_the_reference_pi():
    """The documented deviation: the header's pi (``reanalysed_pi``: its bits, by the test above) against the reference's
    softmax(log(N + 1e-10) / T) at T = 1 over the legal cells (``batch_pi_and_moves``).  Per entry at most

        2^-25 + (A + 1) * 1e-10 / sum(N) + 1e-12

    -- the float32 cast of a value <= 1 (half an ulp), the reference's + 1e-10 inside the logarithm (it adds 1e-10 to the entry and
    up to A * 1e-10 to the normaliser, each relative to sum(N)), the float64 log / exp round trip.  1200 random rows, A = 36 .. 256,
    sum(N) = 1 .. 799."""
    rs = np.random.RandomState(7)
    worst = 0.0
    for A in (36, 121, 225, 256):
        rows, legal = [], []
        for _ in range(300):
            k = rs.randint(1, A + 1)                                    # legal cells
            mask = np.zeros(A, dtype=bool)
            mask[rs.permutation(A)[:k]] = True
            total = rs.randint(1, 800)
            counts = np.zeros(A, dtype=np.int32)
            counts[np.nonzero(mask)[0]] = rs.multinomial(total, rs.dirichlet(np.full(k, 0.3)))
            rows.append(counts)
            legal.append(mask)
        vis, legal = np.array(rows), np.array(legal)
        ours, written = reanalysed_pi(vis)
        assert written.all()
        ref, _ = batch_pi_and_moves(vis, legal, 1.0, np.zeros(len(vis)))
        bound = 2.0 ** -25 + (A + 1) * 1e-10 / vis.sum(axis=1, keepdims=True) + 1e-12
        ratio = np.abs(ours.astype(np.float64) - ref) / bound
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (A, float(ratio.max()))
    print('worst use of the bound: %.3f' % worst)


# ----------------------------------------------------------------------------------------------- draws, slots, the ticket
def test_draws_equal_the_restatement(drv):
    seen = []
    for seed, step, positions in ((0, 0, 40), (13, 1, 40), (2 ** 64 - 1, 2 ** 40 + 3, 1), (5, 7, 2 ** 24)):
        got, = drv.run('draws', [seed, step, 96, positions], [], [np.int64])
        want = replay_reanalyse_draws(seed, step, 96, positions)
        assert want.dtype == np.int64 and np.array_equal(got, want)
        assert (got >= 0).all() and (got < positions).all()
        seen.append(got)
        # the sampler's stream ("replay") of the same (seed, step) is another one
        other = np.array([replay_index(seed, step, i, positions) for i in range(96)])
        assert positions == 1 or not np.array_equal(other, got)
    assert len(set(seen[0].tolist())) > 30 and not np.array_equal(seen[0], seen[1])             # spread over the positions; keyed by step
    assert not np.array_equal(replay_reanalyse_draws(5, 0, 64, 40), replay_reanalyse_draws(5, 1, 64, 40))
    assert not np.array_equal(replay_reanalyse_draws(5, 0, 64, 40), replay_reanalyse_draws(6, 0, 64, 40))
    with pytest.raises(ValueError):
        replay_reanalyse_draws(0, 0, 4, 0)


def test_slots_and_the_ticket(drv):
    index = np.array([0, 1, 38, 39, 40, -1, 2 ** 40, -2 ** 40], dtype=np.int64)
    got, = drv.run('slots', [17, 40, 40], [index], [np.int64])                                  # a full ring that has wrapped: oldest at slot 17
    assert got.tolist() == [17, 18, 15, 16, -1, -1, -1, -1]
    got, = drv.run('slots', [0, 5, 40], [index], [np.int64])                                    # five positions held of forty slots
    assert got.tolist() == [0, 1, -1, -1, -1, -1, -1, -1]
    pairs = np.array([[0, 0], [55, 55], [55, 56], [56, 55], [2 ** 40, 2 ** 40], [0, 40]], dtype=np.int64)
    got, = drv.run('tickets', [], [pairs], [np.int32])
    assert got.tolist() == [1, 1, 0, 0, 1, 0]                                                   # (a count: a full turn of the ring is not "the same")


# ----------------------------------------------------------------------------------------------- the trainer's options
def test_the_trainer_refuses_reanalyse_without_device_replay_or_batched_mode():
    """--reanalyse needs --device-replay and batched mode: the parser says so and exits non-zero before anything touches the GPU."""
    script = os.path.join(REPO, 'tools', 'train_alphazero.py')
    for extra, message in (([], b'--reanalyse needs --device-replay'), (['--games-in-flight', '16'], b'--reanalyse needs --device-replay'),
                           (['--device-replay'], b'--reanalyse needs --games-in-flight > 0 (batched mode)')):
        for value in ('32', 'all'):
            run = subprocess.run([sys.executable, script, '--reanalyse', value] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                 env=dict(os.environ, PYTHONPATH=REPO))
            assert run.returncode == 2 and message in run.stderr and b'usage:' in run.stderr, run.stderr[-600:]
    import replay_cases as rc
    tr = rc.trainer()
    assert tr.reanalyse_arg('all') == 'all' and tr.reanalyse_arg('2048') == 2048 and tr.reanalyse_arg('0') == 0
    args = tr.parse_args([])
    assert (args.reanalyse, args.reanalyse_slots, args.reanalyse_playouts) == (0, 512, None)   # off by default
    for value in (32, 'all'):
        with pytest.raises(ValueError, match='needs --device-replay'):
            tr.TrainPipeline(board_size=3, n_in_row=3, reanalyse=value)
    pipe = tr.TrainPipeline(board_size=3, n_in_row=3)
    assert pipe.reanalyse is None and pipe._reanalyser is None and pipe.reanalyse_round() == 0   # off: nothing is allocated
