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
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "rlzero_hip.h"
#include "rz_host.h"
#include "rz_replay_rules.h"

namespace {

constexpr int kMaxCells = RZ_MAX_BOARD_SIZE * RZ_MAX_BOARD_SIZE;   // 256: plies of a game = threads of k_replay_add
constexpr int kRecWords = 2 * RZ_BOARD_WORDS;                      // uint64 words of a position's stones
constexpr unsigned long long kReplaySalt = 0x7265706C61790000ull;  // "replay": the sampler's own stream
constexpr int kMetaParityBit = 9, kMetaZShift = 10;
constexpr int kFlagBadIndex = 1;

struct ReplayDev {
    unsigned long long *stones;   // [capacity][2][RZ_BOARD_WORDS]
    int32_t *meta;                // [capacity]
    float *pi;                    // [capacity][A]
    const int16_t *src_state;     // [S][C]
    const int16_t *src_pi;        // [S][A]
    int32_t *err;
    long long capacity;
    int A;                        // width of a pi row (Gomoku: C; Connect4: cols)
    int C, S, cols;               // cells; symmetries (8 or 2); columns of the board
};

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// entry i of update `step`: the high half of x * n_entries (integer only; a value's probability is floor or ceil of 2^64 / n over
// 2^64, i.e. within 2^-64 of 1 / n)
__device__ __forceinline__ long long replay_index(unsigned long long seed, unsigned long long step, unsigned long long i,
                                                  unsigned long long n_entries) {
    unsigned long long x = splitmix64(seed ^ kReplaySalt);
    x = splitmix64(x ^ step);
    x = splitmix64(x ^ i);
    return (long long)__umul64hi(x, n_entries);
}

// One workgroup per game, thread p = ply p (blockDim.x == 256 >= plies).  `base[g]`: kept plies of the games before g; a kept ply of
// global rank t goes to slot (cursor + t) % capacity unless t < skip (more kept plies than slots: only the last `capacity` are
// written, so no two threads of the launch share a slot).
// kC4: the moves are Connect4 columns.  Thread p turns column p into its cell over the move list in LDS, behind the first barrier;
// one more barrier, and everything below reads cells.
// kQ (rz_replay_enable_values): the search's root value of every kept ply, q_rows[t], goes to q_of[slot] beside the meta word; the
// instantiations without it never read either pointer and are the code they were.
template <bool kC4, bool kQ>
__global__ __launch_bounds__(kMaxCells) void k_replay_add(ReplayDev R, const int32_t *__restrict__ offsets, const int32_t *__restrict__ base,
                                                           const int32_t *__restrict__ winner, const int32_t *__restrict__ moves,
                                                           const uint8_t *__restrict__ keep, const float *__restrict__ pi_rows,
                                                           long long cursor, long long skip, const float *__restrict__ q_rows,
                                                           float *__restrict__ q_of) {
    __shared__ int32_t s_moves[kMaxCells];
    __shared__ int32_t s_slot[kMaxCells];
    __shared__ int32_t s_row[kMaxCells];
    __shared__ int32_t s_kept[kMaxCells / 64];
    const int g = blockIdx.x, p = threadIdx.x, lane = p & 63, wave = p >> 6;
    const int off = offsets[g];
    const int P = min(offsets[g + 1] - off, kMaxCells);
    const bool in = p < P;
    s_moves[p] = in ? (moves[off + p] & (kMaxCells - 1)) : 0;
    const bool kept = in && keep[off + p] != 0;
    const unsigned long long ballot = __ballot(kept);
    if (lane == 0) s_kept[wave] = __popcll(ballot);
    __syncthreads();
    const int32_t *s_cells = s_moves;   // the cell of every ply (Gomoku: the move itself)
    if (kC4) {
        __shared__ int32_t s_dropped[kMaxCells];
        s_dropped[p] = in ? (rzrr::cell_of_ply(s_moves, p, R.cols) & (kMaxCells - 1)) : 0;
        __syncthreads();
        s_cells = s_dropped;
    }
    int rank = __popcll(ballot & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += s_kept[w];
    const long long t = (long long)base[g] + rank;
    int slot = -1;
    if (kept && t >= skip) {
        slot = (int)((cursor + t) % R.capacity);
        unsigned long long own[RZ_BOARD_WORDS] = {0, 0, 0, 0}, opp[RZ_BOARD_WORDS] = {0, 0, 0, 0};
        for (int q = 0; q < p; ++q) {
            const int m = s_cells[q];
            const unsigned long long bit = 1ull << (m & 63);
            const bool mine = ((q ^ p) & 1) == 0;   // ply q was the mover's when q and p have the same parity
#pragma unroll
            for (int w = 0; w < RZ_BOARD_WORDS; ++w) {
                own[w] |= (mine && (m >> 6) == w) ? bit : 0ull;
                opp[w] |= (!mine && (m >> 6) == w) ? bit : 0ull;
            }
        }
        unsigned long long *rec = R.stones + (long long)slot * kRecWords;
#pragma unroll
        for (int w = 0; w < RZ_BOARD_WORDS; ++w) {
            rec[w] = own[w];
            rec[RZ_BOARD_WORDS + w] = opp[w];
        }
        const int win = winner[g];
        const int z = win < 0 ? 0 : ((p & 1) == win ? 1 : -1);
        const int last = p > 0 ? s_cells[p - 1] + 1 : 0;
        R.meta[slot] = last | ((p & 1) << kMetaParityBit) | ((z + 1) << kMetaZShift);
        if (kQ) q_of[slot] = q_rows[t];
    }
    s_slot[p] = slot;
    s_row[p] = (int32_t)t;
    __syncthreads();
    // the pi rows: a wave per kept ply, coalesced
    for (int q = wave; q < P; q += kMaxCells / 64) {
        const int sl = s_slot[q];
        if (sl < 0) continue;
        const float *src = pi_rows + (long long)s_row[q] * R.A;
        float *dst = R.pi + (long long)sl * R.A;
        for (int o = lane; o < R.A; o += 64) dst[o] = src[o];
    }
}

// entry e -> output row i: a thread per output cell (blockDim.x >= C >= A).  Gomoku: entry 8 j + k, one width for both tables;
// Connect4: entry 2 j + k, the planes over the C cells and pi over the A columns, written by the first A threads.
// kMix (rz_replay_set_value_mix, lam > 0): zs[i] = rzrr::value_target(z, q[slot], lam) -- the eight symmetries of a position share its
// q --; without it neither q nor lam is read and zs[i] is z, the code it was.
template <bool kC4, bool kMix>
__device__ __forceinline__ void replay_emit(const ReplayDev &R, long long e, long long oldest, long long i, float *__restrict__ states,
                                            float *__restrict__ pis, float *__restrict__ zs, const float *__restrict__ q, double lam) {
    const int o = threadIdx.x, A = R.A, C = kC4 ? R.C : R.A, k = (int)(e & (kC4 ? 1 : 7));
    const long long slot = (oldest + (e >> (kC4 ? 1 : 3))) % R.capacity;
    const unsigned long long *rec = R.stones + slot * kRecWords;   // (uniform across the workgroup)
    const unsigned long long a0 = rec[0], a1 = rec[1], a2 = rec[2], a3 = rec[3], b0 = rec[4], b1 = rec[5], b2 = rec[6], b3 = rec[7];
    const int meta = R.meta[slot];
    if (o == 0) {
        const float z = (float)(((meta >> kMetaZShift) & 3) - 1);
        zs[i] = kMix ? rzrr::value_target(z, q[slot], lam) : z;
    }
    if (o >= C) return;
    const int s = R.src_state[k * C + o];
    const int w = s >> 6;
    const unsigned long long own = w == 0 ? a0 : w == 1 ? a1 : w == 2 ? a2 : a3;
    const unsigned long long opp = w == 0 ? b0 : w == 1 ? b1 : w == 2 ? b2 : b3;
    float *out = states + i * 4 * C;
    out[o] = (float)((own >> (s & 63)) & 1ull);
    out[C + o] = (float)((opp >> (s & 63)) & 1ull);
    out[2 * C + o] = (s + 1 == (meta & 511)) ? 1.0f : 0.0f;
    out[3 * C + o] = ((meta >> kMetaParityBit) & 1) ? 0.0f : 1.0f;
    if (kC4 && o >= A) return;
    pis[i * A + o] = R.pi[slot * A + R.src_pi[k * A + o]];
}

template <bool kC4, bool kMix>
__global__ __launch_bounds__(kMaxCells) void k_replay_gather(ReplayDev R, const long long *__restrict__ indices, long long oldest,
                                                              long long n_entries, float *__restrict__ states, float *__restrict__ pis,
                                                              float *__restrict__ zs, const float *__restrict__ q, double lam) {
    const long long i = blockIdx.x;
    const long long e = indices[i];
    if (e < 0 || e >= n_entries) {   // an index from the device: nothing is read or written for it
        if (threadIdx.x == 0) atomicOr(R.err, kFlagBadIndex);
        return;
    }
    replay_emit<kC4, kMix>(R, e, oldest, i, states, pis, zs, q, lam);
}

template <bool kC4, bool kMix>
__global__ __launch_bounds__(kMaxCells) void k_replay_sample(ReplayDev R, unsigned long long seed, unsigned long long step, long long oldest,
                                                              long long n_entries, float *__restrict__ states, float *__restrict__ pis,
                                                              float *__restrict__ zs, const float *__restrict__ q, double lam) {
    const long long i = blockIdx.x;
    replay_emit<kC4, kMix>(R, replay_index(seed, step, (unsigned long long)i, (unsigned long long)n_entries), oldest, i, states, pis, zs, q, lam);
}

// Reanalyse, the way out: position index -> ring slot (`where`, -1 for an index outside 0 .. count - 1) and the stored record as a
// root of the search engine.  A thread per (row, record word): word j of the record goes to rzrr::root_word of row i; thread 0 of a
// row also writes the slot, the side to move and the last move.  indices NULL: the draws of refresh `step` made here.  A bad index
// sets the flag and writes only where[i] = -1: nothing of the store is read for it and its root is left as it was.
__global__ __launch_bounds__(kMaxCells) void k_replay_positions(ReplayDev R, const long long *__restrict__ indices, unsigned long long seed,
                                                                 unsigned long long step, long long oldest, long long count, long long n,
                                                                 int32_t *__restrict__ where, unsigned long long *__restrict__ stones,
                                                                 int32_t *__restrict__ to_move, int32_t *__restrict__ last_move) {
    const long long tid = (long long)blockIdx.x * kMaxCells + threadIdx.x;
    const long long i = tid / kRecWords;
    const int j = (int)(tid % kRecWords);
    if (i >= n) return;
    const long long index = indices != nullptr ? indices[i] : rzrr::reanalyse_position(seed, step, (uint64_t)i, (uint64_t)count);
    const long long slot = rzrr::slot_of_position(index, oldest, count, R.capacity);
    if (slot < 0) {
        if (j == 0) {
            atomicOr(R.err, kFlagBadIndex);
            where[i] = -1;
        }
        return;
    }
    const int32_t meta = R.meta[slot];
    stones[i * kRecWords + rzrr::root_word(meta, j)] = R.stones[slot * kRecWords + j];
    if (j == 0) {
        where[i] = (int32_t)slot;
        to_move[i] = rzrr::root_to_move(meta);
        last_move[i] = rzrr::root_last_move(meta);
    }
}

// Reanalyse, the way back: pi[where[i]][a] = N[i][a] / sum N[i] (rzrr::pi_of_visits).  A workgroup per row, a thread per action
// (blockDim.x = A rounded up to whole waves: one wave for Connect4's A = cols <= 16, up to four for Gomoku).  The sum is an INTEGER reduction -- across the lanes of a wave, then across the waves
// through LDS -- so it is exact whatever the order.  where < 0 (a refused or a padding row), a slot outside the capacity or a sum of
// 0 writes nothing; stones and meta are never written.  Every branch before the barrier is uniform across the workgroup.
__global__ __launch_bounds__(kMaxCells) void k_replay_update_pi(ReplayDev R, const int32_t *__restrict__ where, const int32_t *__restrict__ visits) {
    __shared__ long long s_part[kMaxCells / 64];
    const long long i = blockIdx.x;
    const int a = threadIdx.x, A = R.A, lane = a & 63, wave = a >> 6;
    const long long slot = where[i];
    if (slot < 0 || slot >= R.capacity) return;
    const int32_t mine = a < A ? visits[i * A + a] : 0;
    long long part = rzrr::visit_count(mine);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
    if (lane == 0) s_part[wave] = part;
    __syncthreads();
    long long sum = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) sum += s_part[w];
    if (sum == 0 || a >= A) return;
    R.pi[slot * A + a] = rzrr::pi_of_visits(mine, sum);
}

// Reanalyse, the way back for the value target: q[where[i]] = float32(values[i][0]) -- values: the engine's rz_root_values,
// float64 [n][2], of which [0] is the root value for the player to move.  A thread per row.  where < 0 (a refused or a padding row), a
// slot outside the capacity or a NaN value (an unvisited root) writes nothing (rzrr::value_written); stones, meta and pi are never
// written.  Two rows that name one slot write the same bits: the search is deterministic.
__global__ __launch_bounds__(kMaxCells) void k_replay_update_q(float *__restrict__ q, long long capacity, const int32_t *__restrict__ where,
                                                                const double *__restrict__ values, long long n) {
    const long long i = (long long)blockIdx.x * kMaxCells + threadIdx.x;
    if (i >= n) return;
    const long long slot = where[i];
    const double v = values[2 * i];
    if (rzrr::value_written(slot, capacity, v)) q[slot] = (float)v;
}

}  // namespace

struct rz_replay {
    ReplayDev dev = {};
    int game = RZ_GAME_GOMOKU, rows = 0, device = 0;
    long long cursor = 0, count = 0;   // next slot written; positions held
    long long stored = 0;              // positions ever stored: the ticket of rz_replay_positions / rz_replay_update_pi
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
    if (n > 0 && (d_states == nullptr || d_pis == nullptr || d_zs == nullptr)) return rz_fail(RZ_ERR_ARG, "NULL output buffer");
    return RZ_OK;
}

inline unsigned rp_block(const rz_replay *r) { return (unsigned)((r->dev.C + 63) / 64 * 64); }       // a thread per cell
inline unsigned rp_pi_block(const rz_replay *r) { return (unsigned)((r->dev.A + 63) / 64 * 64); }   // a thread per action
inline bool rp_connect4(const rz_replay *r) { return r->game == RZ_GAME_CONNECT4; }
inline long long rp_oldest(const rz_replay *r) { return ((r->cursor - r->count) % r->dev.capacity + r->dev.capacity) % r->dev.capacity; }

// the store of `capacity` positions of a rows x cols board (the caller has checked the board)
int rp_create(int game, int rows, int cols, int64_t capacity, int32_t device, rz_replay **out) {
    if (capacity < 1 || capacity > (1LL << 24)) return rz_fail(RZ_ERR_ARG, "capacity outside 1 .. 2^24 positions");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return rz_fail(RZ_ERR_ARG, "bad device ordinal");
    if (hipSetDevice(device) != hipSuccess) return rz_fail(RZ_ERR_HIP, "hipSetDevice failed");
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
    D.capacity = capacity;
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
    const long long cap = r->dev.capacity, skip = kept > cap ? kept - cap : 0;
    auto kernel = with_q ? (rp_connect4(r) ? k_replay_add<true, true> : k_replay_add<false, true>)
                         : (rp_connect4(r) ? k_replay_add<true, false> : k_replay_add<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_games), dim3(kMaxCells), 0, s, r->dev, (const int32_t *)(d + o_off), (const int32_t *)(d + o_base),
                       (const int32_t *)(d + o_win), (const int32_t *)(d + o_moves), (const uint8_t *)(d + o_keep), (const float *)(d + o_pi),
                       r->cursor, skip, with_q ? (const float *)(d + o_q) : (const float *)nullptr, r->q);
    RZ_TRY(r->stage.launched(s, "k_replay_add"));
    r->cursor = (r->cursor + kept) % cap;
    r->count = r->count + kept > cap ? cap : r->count + kept;
    r->stored += kept;
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
    if (count) *count = r->count;
    if (cursor) *cursor = r->cursor;
    if (capacity) *capacity = r->dev.capacity;
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
    if (r->stored != 0) return rz_fail(RZ_ERR_ARG, "rz_replay_enable_values: the buffer holds positions stored without a value");
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
    if (!rzrr::ticket_current(ticket, r->stored)) return rz_fail(RZ_ERR_ARG, "stale ticket: positions were stored since rz_replay_positions");
    if (n == 0) return RZ_OK;
    if (d_where == nullptr || d_root_values == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    const unsigned blocks = (unsigned)((n + kMaxCells - 1) / kMaxCells);
    hipLaunchKernelGGL(k_replay_update_q, dim3(blocks), dim3(kMaxCells), 0, (hipStream_t)stream, r->q, r->dev.capacity, d_where, d_root_values, (long long)n);
    return rz_launched("k_replay_update_q");
}

int rz_replay_read_values(rz_replay *r, int64_t first, int64_t n, float *h_q, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (r->q == nullptr) return rz_fail(RZ_ERR_ARG, "rz_replay_read_values: the buffer keeps no search values (rz_replay_enable_values)");
    if (first < 0 || n < 0 || first + n > r->count) return rz_fail(RZ_ERR_ARG, "positions outside 0 .. count - 1");
    if (n == 0) return RZ_OK;
    if (h_q == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    const long long cap = r->dev.capacity, start = (rp_oldest(r) + first) % cap;
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
    if ((h_indices == nullptr) == (d_indices == nullptr)) return rz_fail(RZ_ERR_ARG, "exactly one of h_indices / d_indices");
    if (n == 0) return RZ_OK;
    const long long n_entries = r->dev.S * r->count;
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
    hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(rp_block(r)), 0, s, r->dev, idx, rp_oldest(r), n_entries, d_states, d_pis, d_zs,
                       rp_mixing(r) ? (const float *)r->q : (const float *)nullptr, r->mix);
    return h_indices != nullptr ? r->stage.launched(s, "k_replay_gather") : rz_launched("k_replay_gather");
}

int rz_replay_sample(rz_replay *r, uint64_t seed, uint64_t step, int64_t n, float *d_states, float *d_pis, float *d_zs, void *stream) {
    RZ_ENTER(rp_ready, r);
    RZ_TRY(rp_outputs(r, n, d_states, d_pis, d_zs));
    const long long n_entries = r->dev.S * r->count;
    if (n_entries == 0) return rz_fail(RZ_ERR_ARG, "the replay buffer is empty");
    if (n == 0) return RZ_OK;
    auto kernel = rp_mixing(r) ? (rp_connect4(r) ? k_replay_sample<true, true> : k_replay_sample<false, true>)
                               : (rp_connect4(r) ? k_replay_sample<true, false> : k_replay_sample<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(rp_block(r)), 0, (hipStream_t)stream, r->dev, (unsigned long long)seed,
                       (unsigned long long)step, rp_oldest(r), n_entries, d_states, d_pis, d_zs,
                       rp_mixing(r) ? (const float *)r->q : (const float *)nullptr, r->mix);
    return rz_launched("k_replay_sample");
}

int rz_replay_ticket(rz_replay *r, int64_t *ticket) {
    if (r == nullptr) return rz_fail(RZ_ERR_ARG, "replay handle is NULL");
    if (ticket == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    *ticket = r->stored;
    return RZ_OK;
}

int rz_replay_positions(rz_replay *r, const int64_t *h_indices, const int64_t *d_indices, uint64_t seed, uint64_t step, int64_t n,
                        int32_t *d_where, uint64_t *d_stones, int32_t *d_to_move, int32_t *d_last_move, int64_t *ticket, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (n < 0 || n > (1LL << 24)) return rz_fail(RZ_ERR_ARG, "n outside 0 .. 2^24");
    if (ticket == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    if (h_indices != nullptr && d_indices != nullptr) return rz_fail(RZ_ERR_ARG, "at most one of h_indices / d_indices");
    *ticket = r->stored;
    if (n == 0) return RZ_OK;
    if (d_where == nullptr || d_stones == nullptr || d_to_move == nullptr || d_last_move == nullptr) return rz_fail(RZ_ERR_ARG, "NULL output buffer");
    if (r->count == 0) return rz_fail(RZ_ERR_ARG, "the replay buffer is empty");
    hipStream_t s = (hipStream_t)stream;
    const long long *idx = (const long long *)d_indices;
    if (h_indices != nullptr) {
        for (int64_t i = 0; i < n; ++i)
            if (h_indices[i] < 0 || h_indices[i] >= r->count) return rz_fail(RZ_ERR_ARG, "position index outside 0 .. count - 1");
        RZ_TRY(r->stage.reserve((size_t)n * 8, s));
        memcpy(r->stage.h, h_indices, (size_t)n * 8);
        RZ_TRY(r->stage.upload((size_t)n * 8, s));
        idx = (const long long *)r->stage.d;
    }
    const unsigned blocks = (unsigned)((n * kRecWords + kMaxCells - 1) / kMaxCells);
    hipLaunchKernelGGL(k_replay_positions, dim3(blocks), dim3(kMaxCells), 0, s, r->dev, idx, (unsigned long long)seed, (unsigned long long)step,
                       rp_oldest(r), r->count, (long long)n, d_where, (unsigned long long *)d_stones, d_to_move, d_last_move);
    return h_indices != nullptr ? r->stage.launched(s, "k_replay_positions") : rz_launched("k_replay_positions");
}

int rz_replay_update_pi(rz_replay *r, const int32_t *d_where, int64_t n, const int32_t *d_visits, int64_t ticket, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (n < 0 || n > (1LL << 24)) return rz_fail(RZ_ERR_ARG, "n outside 0 .. 2^24");
    // an add since rz_replay_positions may have given a slot to another position: the search's result has no home
    if (!rzrr::ticket_current(ticket, r->stored)) return rz_fail(RZ_ERR_ARG, "stale ticket: positions were stored since rz_replay_positions");
    if (n == 0) return RZ_OK;
    if (d_where == nullptr || d_visits == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    hipLaunchKernelGGL(k_replay_update_pi, dim3((unsigned)n), dim3(rp_pi_block(r)), 0, (hipStream_t)stream, r->dev, d_where, d_visits);
    return rz_launched("k_replay_update_pi");
}

int rz_replay_read(rz_replay *r, int64_t first, int64_t n, uint64_t *h_stones, int32_t *h_meta, float *h_pi, void *stream) {
    RZ_ENTER(rp_ready, r);
    if (first < 0 || n < 0 || first + n > r->count) return rz_fail(RZ_ERR_ARG, "positions outside 0 .. count - 1");
    hipStream_t s = (hipStream_t)stream;
    const long long cap = r->dev.capacity, start = (rp_oldest(r) + first) % cap;
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
