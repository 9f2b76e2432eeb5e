// rz_replay.hip -- the device replay buffer (include/rlzero_hip.h: rz_replay_*, ABI 31; Reanalyse, ABI 38; Connect4, ABI 39).
//
// The learner's samples live in device memory as a ring of self-contained positions (two bitboards, one meta word, a pi row) and
// a mini-batch is ONE launch: k_replay_gather / k_replay_sample write the observation planes, the symmetry-transformed pi and z
// of every entry straight into the learner's tensors.  The eight symmetries are two tables of source cells the host obtained
// from the reference's own numpy expressions (tools/train_alphazero.py:59-79) -- the planes and pi are permuted DIFFERENTLY there,
// and nothing here re-derives either permutation.  k_replay_add forms the positions of finished games from their move lists.
//
// Two games share the store.  Gomoku: C = A = B * B, S = 8 symmetries.  Connect4: C = rows * cols cells, a pi row of A = cols floats,
// S = 2 (the position and its left-right mirror); its moves are columns, which k_replay_add<true> turns into cells
// (rz_replay_rules.h: cell_of_ply) before the Gomoku code runs on them.  k_replay_add, k_replay_gather and k_replay_sample are
// templates on the game so that the Gomoku instantiations keep the code they had (entry >> 3, entry & 7, one table width).
//
// Value targets from the search (ABI 44, opt-in: rz_replay_enable_values): a float32 array q [capacity] beside the meta words holds the
// root value the mover's search saw (NaN: none), written by k_replay_add<.., true> and refreshed by k_replay_update_q; with
// rz_replay_set_value_mix(lam > 0) k_replay_gather<.., true> / k_replay_sample<.., true> write zs = (1 - lam) z + lam q
// (rz_replay_rules.h: value_target).  Without the option no array exists and the <.., false> instantiations -- the code of ABI 43 -- run.
//
// Bounds: every slot is reduced modulo the capacity, every table entry is checked at upload (< C for the planes, < A for pi), an
// entry index from the device is checked by the kernel before anything is read, moves are checked on the host (Gomoku: < A;
// Connect4: a column < cols that is not full) and index registers or LDS arrays of kMaxCells entries under a mask, not memory.
//
// This file is the host side of ONE translation unit: the kernels lie in headers beside it, one per family, each of which compiles
// alone (tests/test_csrc_headers.py) and describes its kernels where they are defined.
//   rz_replay_dev.h      no kernel: ReplayDev, the constants of a record, replay_emit (an entry as a row of a mini-batch)
//   rz_replay_add.h      the way in: k_replay_add
//   rz_replay_batch.h    the mini-batch: k_replay_gather, k_replay_sample
//   rz_replay_refresh.h  Reanalyse: k_replay_positions, k_replay_update_pi, k_replay_update_q
// The rules the kernels and the host share are plain C++ in rz_replay_rules.h, the ring of positions is rz_ring.h's; both are tested
// on the CPU.  Below: struct rz_replay, the argument checks and every extern "C" entry point.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "rlzero_hip.h"
#include "rz_host.h"
#include "rz_replay_rules.h"
#include "rz_ring.h"

// (this order is the order of the kernels in the code object; the template instantiations follow in the order the code below names them)
#include "rz_replay_dev.h"
#include "rz_replay_add.h"
#include "rz_replay_batch.h"
#include "rz_replay_refresh.h"

struct rz_replay {
    ReplayDev dev = {};
    int game = RZ_GAME_GOMOKU, rows = 0, device = 0;
    rz_ring ring;   // of positions; ring.stored is the ticket of rz_replay_positions / rz_replay_update_pi
    int16_t *d_tables = nullptr;
    bool tables = false;
    float *q = nullptr;   // [capacity] the search's root value of every position (rz_replay_enable_values; NaN: none), else no array
    double mix = 0.0;     // rz_replay_set_value_mix: lam of the value target; 0: zs is z, the kernels without q
    DevPool pool;    // the store
    Staging stage;   // what the host hands to a launch
};

namespace {

int rp_ready(rz_replay *r) {
    if (r == nullptr) return rz_fail(RZ_ERR_ARG, "replay handle is NULL");
    return rz_on_device(r->device);
}

int rp_outputs(rz_replay *r, int64_t n, const float *d_states, const float *d_pis, const float *d_zs) {
    if (!r->tables) return rz_fail(RZ_ERR_ARG, "rz_replay_set_tables has not been called");
    if (n < 0 || n > 0x7fffffffLL) return rz_fail(RZ_ERR_ARG, "n out of range");
    return n > 0 ? rz_outputs(d_states, d_pis, d_zs) : RZ_OK;
}

inline unsigned rp_block(const rz_replay *r) { return (unsigned)((r->dev.C + 63) / 64 * 64); }       // a thread per cell
inline unsigned rp_pi_block(const rz_replay *r) { return (unsigned)((r->dev.A + 63) / 64 * 64); }   // a thread per action
inline bool rp_connect4(const rz_replay *r) { return r->game == RZ_GAME_CONNECT4; }

// the store of `capacity` positions of a rows x cols board (the caller has checked the board)
int rp_create(int game, int rows, int cols, int64_t capacity, int32_t device, rz_replay **out) {
    if (capacity < 1 || capacity > (1LL << 24)) return rz_fail(RZ_ERR_ARG, "capacity outside 1 .. 2^24 positions");
    RZ_TRY(rz_claim_device(device));
    rz_replay *r = new (std::nothrow) rz_replay();
    if (!r) return rz_fail(RZ_ERR_OOM, "host allocation failed");
    r->game = game;
    r->rows = rows;
    r->device = device;
    ReplayDev &D = r->dev;
    D.C = rows * cols;
    D.A = game == RZ_GAME_CONNECT4 ? cols : D.C;
    D.S = game == RZ_GAME_CONNECT4 ? 2 : 8;
    D.cols = cols;
    D.capacity = r->ring.capacity = capacity;
    const size_t cap = (size_t)capacity, A = (size_t)D.A;
    bool ok = r->pool.alloc(&D.stones, capacity * kRecWords) == RZ_OK && r->pool.alloc(&D.meta, capacity) == RZ_OK && r->pool.alloc(&D.pi, capacity * D.A) == RZ_OK &&
              r->pool.alloc(&r->d_tables, D.S * (D.C + D.A)) == RZ_OK && r->pool.alloc(&D.err, 1) == RZ_OK;
    if (!ok) {
        rz_replay_destroy(r);
        return rz_fail(RZ_ERR_OOM, "hipMalloc failed (replay store)");
    }
    D.src_state = r->d_tables;
    D.src_pi = r->d_tables + (size_t)D.S * D.C;
    ok = hipMemset(D.err, 0, sizeof(int32_t)) == hipSuccess && hipMemset(D.stones, 0, cap * kRecWords * sizeof(unsigned long long)) == hipSuccess &&
         hipMemset(D.meta, 0, cap * sizeof(int32_t)) == hipSuccess && hipMemset(D.pi, 0, cap * A * sizeof(float)) == hipSuccess &&
         r->stage.create("replay") == RZ_OK && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        rz_replay_destroy(r);
        return rz_fail(RZ_ERR_HIP, "initialisation of the replay store failed");
    }
    *out = r;
    return RZ_OK;
}

// rz_replay_add / rz_replay_add_values: h_q float [kept] the root value of every kept ply, or NULL (a buffer with values stores NaN)
int rp_add(rz_replay *r, int32_t n_games, const int32_t *h_offsets, const int32_t *h_moves, const uint8_t *h_keep, const int32_t *h_winner,
           const float *h_pi, const float *h_q, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (h_q != nullptr && r->q == nullptr) return rz_fail(RZ_ERR_ARG, "values for a buffer without them: rz_replay_enable_values");
    if (n_games < 0) return rz_fail(RZ_ERR_ARG, "n_games < 0");
    if (n_games == 0) return RZ_OK;
    if (h_offsets == nullptr || h_winner == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    const int A = r->dev.A, C = r->dev.C;
    if (h_offsets[0] != 0) return rz_fail(RZ_ERR_ARG, "h_offsets[0] must be 0");
    std::vector<int32_t> base((size_t)n_games);
    long long kept = 0;
    for (int g = 0; g < n_games; ++g) {
        const long long P = (long long)h_offsets[g + 1] - h_offsets[g];
        if (P < 0) return rz_fail(RZ_ERR_ARG, "h_offsets must not decrease");
        if (P > C) return rz_fail(RZ_ERR_ARG, "a game is longer than the board has cells");
        if (h_winner[g] < -1 || h_winner[g] > 1) return rz_fail(RZ_ERR_ARG, "winner must be 0, 1 or -1");
        if (P > 0 && (h_moves == nullptr || h_keep == nullptr)) return rz_fail(RZ_ERR_ARG, "NULL argument");
        base[(size_t)g] = (int32_t)kept;
        if (rp_connect4(r) && P > 0) {   // columns: each inside the board and not played more often than the board has rows
            const int bad = rzrr::first_illegal_drop(h_moves + h_offsets[g], (int)P, r->rows, r->dev.cols);
            if (bad >= 0) {
                const int32_t column = h_moves[h_offsets[g] + bad];
                return rz_fail(RZ_ERR_ARG, column < 0 || column >= r->dev.cols ? "a move is outside the board" : "a column is played more often than the board has rows");
            }
        }
        for (int p = h_offsets[g]; p < h_offsets[g + 1]; ++p) {
            if (h_moves[p] < 0 || h_moves[p] >= A) return rz_fail(RZ_ERR_ARG, "a move is outside the board");
            kept += h_keep[p] != 0;
        }
    }
    const long long total = h_offsets[n_games];
    if (kept == 0) return RZ_OK;
    if (h_pi == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    const bool with_q = r->q != nullptr;
    // staging: offsets | base | winner | moves | keep | pi rows | (a buffer with values) q rows
    const size_t o_off = 0, o_base = o_off + align16(((size_t)n_games + 1) * 4), o_win = o_base + align16((size_t)n_games * 4),
                 o_moves = o_win + align16((size_t)n_games * 4), o_keep = o_moves + align16((size_t)total * 4),
                 o_pi = o_keep + align16((size_t)total), o_q = o_pi + align16((size_t)kept * A * sizeof(float)),
                 bytes = with_q ? o_q + (size_t)kept * sizeof(float) : o_pi + (size_t)kept * A * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    RZ_TRY(r->stage.reserve(bytes, s));
    char *h = (char *)r->stage.h, *d = (char *)r->stage.d;
    memcpy(h + o_off, h_offsets, ((size_t)n_games + 1) * 4);
    memcpy(h + o_base, base.data(), (size_t)n_games * 4);
    memcpy(h + o_win, h_winner, (size_t)n_games * 4);
    memcpy(h + o_moves, h_moves, (size_t)total * 4);
    memcpy(h + o_keep, h_keep, (size_t)total);
    memcpy(h + o_pi, h_pi, (size_t)kept * A * sizeof(float));
    if (with_q) {
        float *hq = (float *)(h + o_q);
        for (long long t = 0; t < kept; ++t) hq[t] = h_q != nullptr ? h_q[t] : NAN;
    }
    RZ_TRY(r->stage.upload(bytes, s));
    auto kernel = with_q ? (rp_connect4(r) ? k_replay_add<true, true> : k_replay_add<false, true>)
                         : (rp_connect4(r) ? k_replay_add<true, false> : k_replay_add<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_games), dim3(kMaxCells), 0, s, r->dev, (const int32_t *)(d + o_off), (const int32_t *)(d + o_base),
                       (const int32_t *)(d + o_win), (const int32_t *)(d + o_moves), (const uint8_t *)(d + o_keep), (const float *)(d + o_pi),
                       r->ring.cursor, r->ring.skip(kept), with_q ? (const float *)(d + o_q) : (const float *)nullptr, r->q);
    RZ_TRY(r->stage.launched(s, "k_replay_add"));
    r->ring.commit(kept);
    return RZ_OK;
}

inline bool rp_mixing(const rz_replay *r) { return r->q != nullptr && r->mix > 0.0; }

}  // namespace

extern "C" {

int rz_replay_create(int32_t board_size, int64_t capacity, int32_t device, rz_replay **out) {
    if (out == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (board_size < 3 || board_size > RZ_MAX_BOARD_SIZE) return rz_fail(RZ_ERR_ARG, "board_size outside 3 .. 16");
    return rp_create(RZ_GAME_GOMOKU, board_size, board_size, capacity, device, out);
}

int rz_replay_create_game(int32_t game_kind, int32_t rows, int32_t cols, int64_t capacity, int32_t device, rz_replay **out) {
    if (out == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (game_kind == RZ_GAME_GOMOKU) {
        if (rows != cols) return rz_fail(RZ_ERR_ARG, "a Gomoku board is square");
        return rz_replay_create(rows, capacity, device, out);
    }
    if (game_kind != RZ_GAME_CONNECT4) return rz_fail(RZ_ERR_ARG, "unknown game_kind");
    if (rows < 1 || rows > RZ_MAX_BOARD_SIZE || cols < 1 || cols > RZ_MAX_BOARD_SIZE) return rz_fail(RZ_ERR_ARG, "rows or cols outside 1 .. 16");
    return rp_create(RZ_GAME_CONNECT4, rows, cols, capacity, device, out);
}

int rz_replay_geometry(rz_replay *r, int32_t *game_kind, int32_t *rows, int32_t *cols, int32_t *n_cells, int32_t *n_actions,
                       int32_t *n_symmetries) {
    if (r == nullptr) return rz_fail(RZ_ERR_ARG, "replay handle is NULL");
    if (game_kind) *game_kind = r->game;
    if (rows) *rows = r->rows;
    if (cols) *cols = r->dev.cols;
    if (n_cells) *n_cells = r->dev.C;
    if (n_actions) *n_actions = r->dev.A;
    if (n_symmetries) *n_symmetries = r->dev.S;
    return RZ_OK;
}

int rz_replay_destroy(rz_replay *r) {
    if (r == nullptr) return RZ_OK;
    (void)hipSetDevice(r->device);
    (void)hipDeviceSynchronize();
    r->stage.destroy();
    delete r;   // (the pool frees the store)
    return RZ_OK;
}

int rz_replay_set_tables_game(rz_replay *r, int32_t n_symmetries, int32_t n_cells, int32_t n_actions, const int16_t *h_src_state,
                              const int16_t *h_src_pi, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (h_src_state == nullptr || h_src_pi == nullptr) return rz_fail(RZ_ERR_ARG, "NULL table");
    const int S = r->dev.S, C = r->dev.C, A = r->dev.A;
    if (n_symmetries != S || n_cells != C || n_actions != A) return rz_fail(RZ_ERR_ARG, "the tables are not of this buffer's symmetries, cells and actions");
    for (int i = 0; i < S * C; ++i)
        if (h_src_state[i] < 0 || h_src_state[i] >= C) return rz_fail(RZ_ERR_ARG, "table entry outside 0 .. C-1");
    for (int i = 0; i < S * A; ++i)
        if (h_src_pi[i] < 0 || h_src_pi[i] >= A) return rz_fail(RZ_ERR_ARG, "table entry outside 0 .. A-1");
    hipStream_t s = (hipStream_t)stream;
    const size_t planes = (size_t)S * C * sizeof(int16_t), pis = (size_t)S * A * sizeof(int16_t);   // (d_tables: src_state, then src_pi)
    RZ_TRY(r->stage.reserve(planes + pis, s));
    memcpy(r->stage.h, h_src_state, planes);
    memcpy((char *)r->stage.h + planes, h_src_pi, pis);
    RZ_TRY(r->stage.upload(planes + pis, s));
    RZ_HIP(hipMemcpyAsync(r->d_tables, r->stage.d, planes + pis, hipMemcpyDeviceToDevice, s));
    RZ_TRY(r->stage.launched(s, "the table copy (replay)"));
    r->tables = true;
    return RZ_OK;
}

int rz_replay_set_tables(rz_replay *r, const int16_t *h_src_state, const int16_t *h_src_pi, void *stream) {
    if (r != nullptr && rp_connect4(r)) return rz_fail(RZ_ERR_ARG, "rz_replay_set_tables takes Gomoku's [8][A] tables: rz_replay_set_tables_game");
    return rz_replay_set_tables_game(r, 8, r != nullptr ? r->dev.A : 0, r != nullptr ? r->dev.A : 0, h_src_state, h_src_pi, stream);
}

int rz_replay_state(rz_replay *r, int64_t *count, int64_t *cursor, int64_t *capacity) {
    if (r == nullptr) return rz_fail(RZ_ERR_ARG, "replay handle is NULL");
    if (count) *count = r->ring.count;
    if (cursor) *cursor = r->ring.cursor;
    if (capacity) *capacity = r->ring.capacity;
    return RZ_OK;
}

int rz_replay_add(rz_replay *r, int32_t n_games, const int32_t *h_offsets, const int32_t *h_moves, const uint8_t *h_keep,
                  const int32_t *h_winner, const float *h_pi, void *stream) {
    return rp_add(r, n_games, h_offsets, h_moves, h_keep, h_winner, h_pi, nullptr, stream);
}

int rz_replay_add_values(rz_replay *r, int32_t n_games, const int32_t *h_offsets, const int32_t *h_moves, const uint8_t *h_keep,
                         const int32_t *h_winner, const float *h_pi, const float *h_q, void *stream) {
    return rp_add(r, n_games, h_offsets, h_moves, h_keep, h_winner, h_pi, h_q, stream);
}

int rz_replay_enable_values(rz_replay *r, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (r->q != nullptr) return RZ_OK;
    if (r->ring.stored != 0) return rz_fail(RZ_ERR_ARG, "rz_replay_enable_values: the buffer holds positions stored without a value");
    float *q = nullptr;
    if (r->pool.alloc(&q, r->dev.capacity) != RZ_OK) return rz_fail(RZ_ERR_OOM, "hipMalloc failed (replay values)");
    // every slot NaN (0x7FC00000): a position that never got a value keeps z as its target
    if (hipMemsetD32Async((hipDeviceptr_t)q, 0x7FC00000, (size_t)r->dev.capacity, (hipStream_t)stream) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "initialisation of the replay values failed");
    r->q = q;
    return RZ_OK;
}

int rz_replay_set_value_mix(rz_replay *r, double lam) {
    if (r == nullptr) return rz_fail(RZ_ERR_ARG, "replay handle is NULL");
    if (!(lam >= 0.0 && lam <= 1.0)) return rz_fail(RZ_ERR_ARG, "rz_replay_set_value_mix: lam %g not in [0, 1]", lam);
    if (lam > 0.0 && r->q == nullptr) return rz_fail(RZ_ERR_ARG, "rz_replay_set_value_mix: lam > 0 needs the search values (rz_replay_enable_values)");
    r->mix = lam;
    return RZ_OK;
}

int rz_replay_update_values(rz_replay *r, const int32_t *d_where, int64_t n, const double *d_root_values, int64_t ticket, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (r->q == nullptr) return rz_fail(RZ_ERR_ARG, "rz_replay_update_values: the buffer keeps no search values (rz_replay_enable_values)");
    if (n < 0 || n > (1LL << 24)) return rz_fail(RZ_ERR_ARG, "n outside 0 .. 2^24");
    if (!r->ring.ticket_current(ticket)) return rz_fail(RZ_ERR_ARG, "stale ticket: positions were stored since rz_replay_positions");
    if (n == 0) return RZ_OK;
    if (d_where == nullptr || d_root_values == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    const unsigned blocks = (unsigned)((n + kMaxCells - 1) / kMaxCells);
    hipLaunchKernelGGL(k_replay_update_q, dim3(blocks), dim3(kMaxCells), 0, (hipStream_t)stream, r->q, r->dev.capacity, d_where, d_root_values, (long long)n);
    return rz_launched("k_replay_update_q");
}

int rz_replay_read_values(rz_replay *r, int64_t first, int64_t n, float *h_q, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (r->q == nullptr) return rz_fail(RZ_ERR_ARG, "rz_replay_read_values: the buffer keeps no search values (rz_replay_enable_values)");
    if (first < 0 || n < 0 || first + n > r->ring.count) return rz_fail(RZ_ERR_ARG, "positions outside 0 .. count - 1");
    if (n == 0) return RZ_OK;
    if (h_q == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    const long long cap = r->ring.capacity, start = r->ring.window_start(first);
    const long long n1 = n < cap - start ? n : cap - start;   // up to the ring's end, then from its start
    bool ok = hipMemcpyAsync(h_q, r->q + start, (size_t)n1 * 4, hipMemcpyDeviceToHost, s) == hipSuccess;
    if (n > n1) ok = ok && hipMemcpyAsync(h_q + n1, r->q, (size_t)(n - n1) * 4, hipMemcpyDeviceToHost, s) == hipSuccess;
    if (!ok || hipStreamSynchronize(s) != hipSuccess) return rz_fail(RZ_ERR_HIP, "read-back failed (replay values)");
    return RZ_OK;
}

int rz_replay_gather(rz_replay *r, const int64_t *h_indices, const int64_t *d_indices, int64_t n, float *d_states, float *d_pis,
                     float *d_zs, void *stream) {
    RZ_ENTER(rp_ready, r);
    RZ_TRY(rp_outputs(r, n, d_states, d_pis, d_zs));
    RZ_ONE_OF(h_indices, d_indices);
    if (n == 0) return RZ_OK;
    const long long n_entries = r->dev.S * r->ring.count;
    if (n_entries == 0) return rz_fail(RZ_ERR_ARG, "the replay buffer is empty");
    hipStream_t s = (hipStream_t)stream;
    const long long *idx = (const long long *)d_indices;
    if (h_indices != nullptr) {
        for (int64_t i = 0; i < n; ++i)
            if (h_indices[i] < 0 || h_indices[i] >= n_entries) return rz_fail(RZ_ERR_ARG, "entry index outside 0 .. S * count - 1");
        RZ_TRY(r->stage.reserve((size_t)n * 8, s));
        memcpy(r->stage.h, h_indices, (size_t)n * 8);
        RZ_TRY(r->stage.upload((size_t)n * 8, s));
        idx = (const long long *)r->stage.d;
    }
    // (rz_replay_set_value_mix: at lam = 0 the kernels without q, whose zs is z)
    auto kernel = rp_mixing(r) ? (rp_connect4(r) ? k_replay_gather<true, true> : k_replay_gather<false, true>)
                               : (rp_connect4(r) ? k_replay_gather<true, false> : k_replay_gather<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(rp_block(r)), 0, s, r->dev, idx, r->ring.oldest(), n_entries, d_states, d_pis, d_zs,
                       rp_mixing(r) ? (const float *)r->q : (const float *)nullptr, r->mix);
    return h_indices != nullptr ? r->stage.launched(s, "k_replay_gather") : rz_launched("k_replay_gather");
}

int rz_replay_sample(rz_replay *r, uint64_t seed, uint64_t step, int64_t n, float *d_states, float *d_pis, float *d_zs, void *stream) {
    RZ_ENTER(rp_ready, r);
    RZ_TRY(rp_outputs(r, n, d_states, d_pis, d_zs));
    const long long n_entries = r->dev.S * r->ring.count;
    if (n_entries == 0) return rz_fail(RZ_ERR_ARG, "the replay buffer is empty");
    if (n == 0) return RZ_OK;
    auto kernel = rp_mixing(r) ? (rp_connect4(r) ? k_replay_sample<true, true> : k_replay_sample<false, true>)
                               : (rp_connect4(r) ? k_replay_sample<true, false> : k_replay_sample<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(rp_block(r)), 0, (hipStream_t)stream, r->dev, (unsigned long long)seed,
                       (unsigned long long)step, r->ring.oldest(), n_entries, d_states, d_pis, d_zs,
                       rp_mixing(r) ? (const float *)r->q : (const float *)nullptr, r->mix);
    return rz_launched("k_replay_sample");
}

int rz_replay_ticket(rz_replay *r, int64_t *ticket) {
    if (r == nullptr) return rz_fail(RZ_ERR_ARG, "replay handle is NULL");
    if (ticket == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    *ticket = r->ring.ticket();
    return RZ_OK;
}

int rz_replay_positions(rz_replay *r, const int64_t *h_indices, const int64_t *d_indices, uint64_t seed, uint64_t step, int64_t n,
                        int32_t *d_where, uint64_t *d_stones, int32_t *d_to_move, int32_t *d_last_move, int64_t *ticket, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (n < 0 || n > (1LL << 24)) return rz_fail(RZ_ERR_ARG, "n outside 0 .. 2^24");
    if (ticket == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    if (h_indices != nullptr && d_indices != nullptr) return rz_fail(RZ_ERR_ARG, "at most one of h_indices / d_indices");
    *ticket = r->ring.ticket();
    if (n == 0) return RZ_OK;
    RZ_TRY(rz_outputs(d_where, d_stones, d_to_move, d_last_move));
    if (r->ring.count == 0) return rz_fail(RZ_ERR_ARG, "the replay buffer is empty");
    hipStream_t s = (hipStream_t)stream;
    const long long *idx = (const long long *)d_indices;
    if (h_indices != nullptr) {
        for (int64_t i = 0; i < n; ++i)
            if (h_indices[i] < 0 || h_indices[i] >= r->ring.count) return rz_fail(RZ_ERR_ARG, "position index outside 0 .. count - 1");
        RZ_TRY(r->stage.reserve((size_t)n * 8, s));
        memcpy(r->stage.h, h_indices, (size_t)n * 8);
        RZ_TRY(r->stage.upload((size_t)n * 8, s));
        idx = (const long long *)r->stage.d;
    }
    const unsigned blocks = (unsigned)((n * kRecWords + kMaxCells - 1) / kMaxCells);
    hipLaunchKernelGGL(k_replay_positions, dim3(blocks), dim3(kMaxCells), 0, s, r->dev, idx, (unsigned long long)seed, (unsigned long long)step,
                       r->ring.oldest(), r->ring.count, (long long)n, d_where, (unsigned long long *)d_stones, d_to_move, d_last_move);
    return h_indices != nullptr ? r->stage.launched(s, "k_replay_positions") : rz_launched("k_replay_positions");
}

int rz_replay_update_pi(rz_replay *r, const int32_t *d_where, int64_t n, const int32_t *d_visits, int64_t ticket, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (n < 0 || n > (1LL << 24)) return rz_fail(RZ_ERR_ARG, "n outside 0 .. 2^24");
    // an add since rz_replay_positions may have given a slot to another position: the search's result has no home
    if (!r->ring.ticket_current(ticket)) return rz_fail(RZ_ERR_ARG, "stale ticket: positions were stored since rz_replay_positions");
    if (n == 0) return RZ_OK;
    if (d_where == nullptr || d_visits == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    hipLaunchKernelGGL(k_replay_update_pi, dim3((unsigned)n), dim3(rp_pi_block(r)), 0, (hipStream_t)stream, r->dev, d_where, d_visits);
    return rz_launched("k_replay_update_pi");
}

int rz_replay_read(rz_replay *r, int64_t first, int64_t n, uint64_t *h_stones, int32_t *h_meta, float *h_pi, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (first < 0 || n < 0 || first + n > r->ring.count) return rz_fail(RZ_ERR_ARG, "positions outside 0 .. count - 1");
    hipStream_t s = (hipStream_t)stream;
    const long long cap = r->ring.capacity, start = r->ring.window_start(first);
    const long long n1 = n < cap - start ? n : cap - start;   // up to the ring's end, then from its start
    const size_t A = (size_t)r->dev.A;
    bool ok = true;
    for (int part = 0; part < 2; ++part) {
        const long long from = part == 0 ? start : 0, cnt = part == 0 ? n1 : n - n1, at = part == 0 ? 0 : n1;
        if (cnt <= 0) continue;
        if (h_stones) ok = ok && hipMemcpyAsync(h_stones + at * kRecWords, r->dev.stones + from * kRecWords, (size_t)cnt * kRecWords * 8, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (h_meta) ok = ok && hipMemcpyAsync(h_meta + at, r->dev.meta + from, (size_t)cnt * 4, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (h_pi) ok = ok && hipMemcpyAsync(h_pi + at * A, r->dev.pi + from * A, (size_t)cnt * A * 4, hipMemcpyDeviceToHost, s) == hipSuccess;
    }
    if (!ok || hipStreamSynchronize(s) != hipSuccess) return rz_fail(RZ_ERR_HIP, "read-back failed (replay)");
    return RZ_OK;
}

int rz_replay_poll_errors(rz_replay *r, int32_t *flags, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (flags == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(flags, r->dev.err, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemsetAsync(r->dev.err, 0, sizeof(int32_t), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "reading the replay flags failed");
    return RZ_OK;
}

}  // extern "C"
