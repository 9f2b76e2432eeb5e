// rz_replay_rules.h -- Reanalyse for the AlphaZero device replay (rz_replay.hip: k_replay_positions, k_replay_update_pi;
// include/rlzero_hip.h: rz_replay_positions, rz_replay_update_pi; rlzero_amd/replay.py: ReplayReanalyser): everything about it that
// is neither a kernel launch nor a memory access.  Plain C++, no HIP include, so that the CPU can test it against
// rlzero_amd/replay.py (pack_positions, reanalysed_pi, replay_reanalyse_draws) and the Gomoku environment
// (tests/test_replay_reanalyse_host.py); the kernels call these functions.  Three rules: a stored record as a root of the search
// engine, the pi row of fresh visit counts, the draws of a refresh -- and the ticket that ties a result to the store it was drawn from.
// Beside the refresh's draws stand the mini-batch's own (replay_index: k_replay_sample; tests/test_rng_host.py).
// For Connect4 (at the end; tests/test_replay_connect4_host.py against Connect4Env): the cell a dropped stone comes to rest in.
#pragma once
#include <stdint.h>

#include "rlzero_hip.h"
#include "rz_ring.h"
#include "rz_rng.h"

#if defined(__HIPCC__)
#define RZR_FN __host__ __device__ __forceinline__
#else
#define RZR_FN inline
#endif

namespace rzrr {

constexpr int kMetaLastMask = 511, kMetaParityBit = 9;   // the meta word: bits 0..8 last move + 1 (0: none), bit 9 ply parity

// ---- record to root.  A record holds stones[2][RZ_BOARD_WORDS] -- [0] the mover's, [1] the opponent's -- and the meta word; the
// engine (rz_set_roots) takes stones[player][word] with player 0 = the first player, the side to move and the last move (-1: none).
// The ply's parity IS the mover's player id: the first player moves at the even plies.
RZR_FN int32_t root_to_move(int32_t meta) { return (meta >> kMetaParityBit) & 1; }
RZR_FN int32_t root_last_move(int32_t meta) { return (meta & kMetaLastMask) - 1; }
// the player whose stones the record's `side` (0 the mover's, 1 the opponent's) holds
RZR_FN int root_player(int32_t meta, int side) { return side == 0 ? root_to_move(meta) : 1 - root_to_move(meta); }
// word j = side * RZ_BOARD_WORDS + w of a record -> its place among the 2 * RZ_BOARD_WORDS words of the root
RZR_FN int root_word(int32_t meta, int j) { return root_player(meta, j / RZ_BOARD_WORDS) * RZ_BOARD_WORDS + j % RZ_BOARD_WORDS; }
// the whole record at once (the CPU's use; the kernel places a word per thread through root_word)
RZR_FN void root_of_record(const uint64_t *rec, int32_t meta, uint64_t *stones, int32_t *to_move, int32_t *last_move) {
    for (int j = 0; j < 2 * RZ_BOARD_WORDS; ++j) stones[root_word(meta, j)] = rec[j];
    *to_move = root_to_move(meta);
    *last_move = root_last_move(meta);
}

// ---- pi of visits: the visit distribution N / sum N, i.e. softmax(log(N + 1e-10)) of the reference at T = 1 up to rounding (the
// numpy expression itself is not reproducible on the device: a documented deviation, bounded in the host test).  Counts below 0
// count as 0; the sum is an integer, exact in any order; one fp64 division, cast to float32 once.  A sum of 0: no row is written.
RZR_FN int64_t visit_count(int32_t n) { return n > 0 ? (int64_t)n : 0; }
RZR_FN int64_t visit_sum(const int32_t *visits, int A) {
    int64_t sum = 0;
    for (int a = 0; a < A; ++a) sum += visit_count(visits[a]);
    return sum;
}
// (sum > 0)
RZR_FN float pi_of_visits(int32_t n, int64_t sum) { return (float)((double)visit_count(n) / (double)sum); }

// ---- the draws of reanalyse_sample (rlzero_amd/replay.py: replay_reanalyse_draws, the same bits): position i of refresh `step` is
// the high half of x * positions_held for the 64-bit x of a splitmix64 chain over (seed ^ salt, step, i) -- uniform over POSITIONS
// (the eight symmetries of a position share one pi row), within 2^-64.  The salt keeps a refresh and a mini-batch
// (rz_replay_sample: "replay") of one update number apart.
using rzrng::mix64;     // (rz_rng.h)
using rzrng::mulhi64;

constexpr uint64_t kReanalyseSalt = 0x617A7265616E616Cull;   // "azreanal"

RZR_FN int64_t reanalyse_position(uint64_t seed, uint64_t step, uint64_t i, uint64_t positions_held) {
    uint64_t x = mix64(seed ^ kReanalyseSalt);
    x = mix64(x ^ step);
    x = mix64(x ^ i);
    return (int64_t)mulhi64(x, positions_held);
}

// ---- the draws of a mini-batch (k_replay_sample; rlzero_amd/replay.py: replay_index, replay_indices, the same bits): entry i of
// update `step` is the high half of x * n_entries (integer only; a value's probability is floor or ceil of 2^64 / n over 2^64, i.e.
// within 2^-64 of 1 / n) -- uniform over ENTRIES, a position under one of its symmetries.
constexpr uint64_t kReplaySalt = 0x7265706C61790000ull;   // "replay": the sampler's own stream

RZR_FN int64_t replay_index(uint64_t seed, uint64_t step, uint64_t i, uint64_t n_entries) {
    uint64_t x = mix64(seed ^ kReplaySalt);
    x = mix64(x ^ step);
    x = mix64(x ^ i);
    return (int64_t)mulhi64(x, n_entries);
}

// ---- a position index (0 = the oldest held) to its ring slot, or -1 for an index outside 0 .. count - 1
RZR_FN int64_t slot_of_position(int64_t index, int64_t oldest, int64_t count, int64_t capacity) {
    if (index < 0 || index >= count) return -1;
    return (oldest + index) % capacity;
}

// ---- the ticket: the number of positions EVER stored in the handle when rz_replay_positions resolved a request.  A count, not the
// write cursor: the cursor returns to the same slot after `capacity` positions, the count never does.  A result may be written
// only while nothing was stored in between -- a slot may hold another position by then.  (The store's own check is its ring's,
// rz_ring.h; this forwarder is the host test's way in.)
inline bool ticket_current(int64_t ticket, int64_t stored) {
    rz_ring ring;
    ring.stored = stored;
    return ring.ticket_current(ticket);
}

// ---- the value target (rz_replay_set_value_mix; rlzero_amd/replay.py: mixed_value_targets, the same bits): z of the game mixed
// with the search's root value q of the position, (1 - lam) z + lam q.  In fp64, each product ROUNDED before the sum -- this file is
// compiled with -ffp-contract=off on both sides; a fused multiply-add gives other bits (tests/test_value_targets_host.py shows
// that it would be caught) -- and cast to float32 once.  A NaN q (a position stored without a value) leaves z as it is.
RZR_FN float value_target(float z, float q, double lam) {
    if (q != q) return z;
    const double keep = (1.0 - lam) * (double)z, take = lam * (double)q;
    return (float)(keep + take);
}
// ---- a refreshed q (k_replay_update_q): float32 of the fresh search's fp64 root value; a NaN (an unvisited root) writes nothing
RZR_FN bool value_written(int64_t slot, int64_t capacity, double v) { return slot >= 0 && slot < capacity && v == v; }

// ---- Connect4 (RZ_GAME_CONNECT4; k_replay_add<true>, rz_replay_add): a move is a COLUMN and the stone drops, a record holds CELLS
// (cell = row * cols + column, row 0 at the bottom: Connect4Env.step).  The cell of ply q of a move list: as many rows up as the
// earlier plies put stones into its column.  The kernel runs it over the move list in LDS, a thread per ply; everything behind it
// (the stones of a position, the last move of the meta word, the root of a search) works on cells, as for Gomoku.
RZR_FN int cell_of_ply(const int32_t *moves, int q, int cols) {
    const int32_t column = moves[q];
    int below = 0;
    for (int j = 0; j < q; ++j) below += moves[j] == column ? 1 : 0;
    return below * cols + column;
}
// the first ply of a move list that is no legal drop on a board of rows x cols (cols <= RZ_MAX_BOARD_SIZE) -- a column outside
// 0 .. cols - 1, or one that holds `rows` stones already --, or -1: what the host refuses before a launch
RZR_FN int first_illegal_drop(const int32_t *moves, int n, int rows, int cols) {
    int height[RZ_MAX_BOARD_SIZE] = {0};
    for (int p = 0; p < n; ++p) {
        const int32_t column = moves[p];
        if (column < 0 || column >= cols || height[column] >= rows) return p;
        ++height[column];
    }
    return -1;
}

}  // namespace rzrr
