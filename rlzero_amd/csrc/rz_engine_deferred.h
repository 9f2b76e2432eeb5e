// rz_engine_deferred.h -- the deferred-priors route of rz_engine.hip: the tree step that finishes the value head itself and leaves a
// record per expansion (k_expand_backup_def, k_tree_step_def), the flush that forms the priors of those records (deferred_priors_body,
// k_deferred_priors) and the kept flush, which forms only the ones a move keeps (Keep, k_keep_mark, k_keep_rows,
// k_deferred_priors_rows); k_deferred_reset restarts the records' counters.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "rz_trace.h"
#include "rz_tree.h"

namespace {

using namespace rzt;   // rz_tree.h: Dev, ValueHead, value_quarter_def, the two bodies, the bitboard rules and the noise hashes

// ------------------------------------------------------------------ deferred priors (value_quarter_def: rz_tree.h)
// A value head of 4 * 8 * PER inputs covers a board of at most 16 * PER cells (deferred_ok): PER says how many words of the
// bitboards the tree code has to look at (rz_tree.h: W)
template <int PER> constexpr int words_of_per() { return PER <= 4 ? 1 : (PER == 8 ? 2 : kWords); }
template <int PER>
__global__ __launch_bounds__(kWave * kDefWaves) void k_expand_backup_def(Dev E, ValueHead vh) {
    __shared__ float part[kDefWaves][kWave];
    __builtin_amdgcn_s_setprio(3);
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    value_quarter_def<PER>(vh, blockIdx.x, lane, wave, part);
    if (wave != 0) {
        __syncthreads();
        return;
    }
    expand_backup_body<float, false, false, false, true, words_of_per<PER>()>(E, nullptr, nullptr, blockIdx.x, lane, RawHeads(), 0, vh, part);
}

// (`obs` is always NULL on this route -- the trunk reads positions -- but stays a run-time argument: with the constant hipcc
// schedules the selection into 115 registers instead of 107, and 112 is what a SIMD has left beside a wave of the trunk)
// TRACE: the instantiation launched while a trace buffer is attached (rz_trace_attach) leaves a record per game; the production
// one carries nothing of it (the trace's live values cost the latency chain 132 bytes of scratch).
template <int PER, bool TRACE>
__global__ __launch_bounds__(kWave * kDefWaves) void k_tree_step_def(Dev E, ValueHead vh, float *obs) {
    __shared__ float part[kDefWaves][kWave];
    __builtin_amdgcn_s_setprio(3);
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    __shared__ unsigned long long trace_t0;
    if (TRACE && threadIdx.x == 0) trace_t0 = rz_trace_now();
    value_quarter_def<PER>(vh, blockIdx.x, lane, wave, part);
    if (wave != 0) {
        __syncthreads();
        return;
    }
    expand_backup_body<float, false, false, false, true, words_of_per<PER>()>(E, nullptr, nullptr, blockIdx.x, lane, RawHeads(), 0, vh, part);
    __syncthreads();   // (wave 0's alone: the other waves have ended)
    select_body<false, words_of_per<PER>()>(E, obs, blockIdx.x, lane);
    if (TRACE && lane == 0) rz_trace_write(E.trace, RZ_TRACE_TREE, E.pend[blockIdx.x] - 1, blockIdx.x, trace_t0);
}

// The flush: the priors of the node expanded in step `slot` of game g -- exp(log_softmax) of the leaf's logits over its legal
// moves, mixed with the Dirichlet noise of counter pend_ctr: expand_backup_body<RAW>'s operations on the same numbers (the
// logits are final: k_heads_split's epilogue), into the block that step reserved.  grid = (games, slots).
// record `rec` = slot * n_games + g, its logits at `r`: the body of both grids below
__device__ __forceinline__ void deferred_priors_body(const Dev &E, int g, long long rec, const float *__restrict__ r, int lane) {
    const int pb = E.pend_pb[rec];
    if (pb < 0) return;
    const int ctr = E.pend_ctr[rec];
    uint64_t st[2][kWords];
    load_board(E.pend_stones, (int)rec, st);
    float x[kWords];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < kWords; ++i) {
        const int j = lane + 64 * i;
        x[i] = j < E.A ? r[j] : -INFINITY;
        mx = fmaxf(mx, x[i]);
    }
    mx = wave_max(mx, lane);
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < kWords; ++i) sum += (lane + 64 * i < E.A) ? expf(x[i] - mx) : 0.0f;
    sum = wave_sum(sum, lane);
    const float lse = mx + logf(sum);
    float *P = arena_priors(E, g, E.cur_arena[g]);
    uint64_t occ[kWords];
#pragma unroll
    for (int j = 0; j < kWords; ++j) occ[j] = st[0][j] | st[1][j];
    const Legal L = legal_of(E, occ, lane);
    int ranks[kWords];
    int before = 0;
#pragma unroll
    for (int j = 0; j < kWords; ++j) ranks[j] = lane_action_rank(E, occ, L, j, lane, before);
    float noise[kWords] = {0.f, 0.f, 0.f, 0.f};
    float noise_sum = 1.0f;
    if (E.add_noise) {
        const uint64_t key = mix64(mix64(E.noise_key[g]) ^ (uint64_t)ctr);
        float local = 0.0f;
#pragma unroll
        for (int j = 0; j < kWords; ++j)
            if (ranks[j] >= 0) {
                noise[j] = gamma03(hash32((uint32_t)key ^ (uint32_t)(key >> 32)) + 0x9E3779B9u * (uint32_t)(64 * j + lane + 1));
                local += noise[j];
            }
        local = wave_sum(local, lane);
        noise_sum = local > 0.0f ? local : 1.0f;
    }
#pragma unroll
    for (int j = 0; j < kWords; ++j) {
        const int rk = ranks[j];
        if (rk < 0) continue;
        float prior = expf(x[j] - lse);
        if (E.add_noise) prior = 0.75f * prior + 0.25f * (noise[j] / noise_sum);
        P[pb + rk] = prior;
    }
}

__global__ __launch_bounds__(kWave) void k_deferred_priors(Dev E, const float *__restrict__ raw, int ld, long long rows_per_slot) {
    const int g = blockIdx.x, slot = blockIdx.y, lane = threadIdx.x;
    if (slot >= E.pend[g]) return;
    deferred_priors_body(E, g, (long long)slot * E.n_games + g, raw + ((size_t)slot * rows_per_slot + g) * ld, lane);
}

// ------------------------------------------------------------------ the kept flush (between k_play_draw and k_play_apply)
// The move is known (Play::keep), and a prior block matters only if it survives update_with_move: advance_body copies the blocks
// of the kept child's subtree and reads one float of the root's own block.  The priors of every other expansion of the search lie
// in the arena the move abandons: they are never formed.  A record is NEEDED when
//   * its leaf board is the root board (the root's own block, expanded in this search: the chosen child's prior is read from it), or
//   * the leaf board has the mover's stone on the cell the move occupies: every leaf below the kept child has, and so has a leaf
//     that reaches the same stones in another order -- a row too many, never one too few --, or
//   * no move was drawn (keep == -2: a stalled slot keeps its whole tree and its counter restarts in k_play_apply; a resignation),
//     or the move is not legal (advance_body flags it).
// k_keep_mark: one workgroup per game, a wave per 64 slots: the needed records as bit masks, their number and the number of
// records with a block (what the full flush writes).
struct Keep {
    unsigned long long *mask;   // [G][words]: bit s % 64 of word s / 64 = record (s, g) is needed
    int32_t *cnt, *pcnt;        // [G] needed records / records with a block
    int32_t *rows;              // [slots * G] the needed records, game-major, slots ascending
    int32_t *count;             // [1] their number
    unsigned long long *stats;  // [2] needed / with a block, summed since the last reset (rz_deferred_keep_stats)
    int words;
};

// (keep_of == NULL: every record with a block of every game -- the full flush of policy on demand, rz_deferred_keep_all)
__global__ __launch_bounds__(256) void k_keep_mark(Dev E, const int32_t *__restrict__ keep_of, Keep Kp) {
    __shared__ int sh[4][2];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = E.pend[g] < E.pend_cap ? E.pend[g] : E.pend_cap;
    const int keep = keep_of != nullptr ? keep_of[g] : -2;
    uint64_t root[2][kWords], occ[kWords];
    load_board(E.root_stones, g, root);
#pragma unroll
    for (int j = 0; j < kWords; ++j) occ[j] = root[0][j] | root[1][j];
    const Legal L = legal_of(E, occ, lane);
    int rank = 0, cell = 0;
    const bool all = keep < 0 || !locate_action(E, occ, L, keep, rank, cell);
    const bool second = E.root_to_move[g] != 0;   // the mover's colour
    int kept = 0, with_block = 0;
    for (int s0 = 64 * wave; s0 < n; s0 += 256) {
        const int s = s0 + lane;
        const long long rec = (long long)s * E.n_games + g;
        const bool has = s < n && E.pend_pb[rec] >= 0;
        bool need = has && all;
        if (has && !all) {
            uint64_t st[2][kWords];
            load_board(E.pend_stones, (int)rec, st);
            bool same = true;
            uint64_t mine[kWords];
#pragma unroll
            for (int j = 0; j < kWords; ++j) {
                same = same && st[0][j] == root[0][j] && st[1][j] == root[1][j];
                mine[j] = second ? st[1][j] : st[0][j];
            }
            need = same || test_bit(mine, cell);
        }
        const unsigned long long m = __ballot(need);
        if (lane == 0) Kp.mask[(long long)g * Kp.words + (s0 >> 6)] = m;
        kept += __popcll(m);
        with_block += __popcll(__ballot(has));
    }
    if (lane == 0) sh[wave][0] = kept, sh[wave][1] = with_block;
    __syncthreads();
    if (tid == 0) {
        Kp.cnt[g] = (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]);
        Kp.pcnt[g] = (sh[0][1] + sh[1][1]) + (sh[2][1] + sh[3][1]);
    }
}

// k_keep_rows: one wave per game: where the game's rows begin (the prefix of cnt over the games before it), then its needed
// records in slot order (ballot masks of k_keep_mark + mbcnt: k_play_order's compaction).  The last game's wave leaves the total.
__global__ __launch_bounds__(kWave) void k_keep_rows(Dev E, Keep Kp) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const bool last = g == E.n_games - 1;
    int base = 0, pending = 0;
    for (int h = lane; h < g; h += kWave) base += Kp.cnt[h];
    if (last)
        for (int h = lane; h < E.n_games; h += kWave) pending += Kp.pcnt[h];
    for (int off = 32; off >= 1; off >>= 1) {
        base += __shfl_xor(base, off);
        pending += __shfl_xor(pending, off);
    }
    const int n = E.pend[g] < E.pend_cap ? E.pend[g] : E.pend_cap;
    int at = base;
    for (int s0 = 0; s0 < n; s0 += kWave) {
        const unsigned long long m = Kp.mask[(long long)g * Kp.words + (s0 >> 6)];
        const int pre = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
        if ((m >> lane) & 1ull) Kp.rows[at + pre] = (s0 + lane) * E.n_games + g;
        at += __popcll(m);
    }
    if (last && lane == 0) {
        Kp.count[0] = at;
        if (Kp.stats != nullptr) {   // (NULL: a full flush by rows -- the counters are the kept flushes')
            Kp.stats[0] += (unsigned long long)at;
            Kp.stats[1] += (unsigned long long)pending;
        }
    }
}

// k_deferred_priors over the listed records: a fixed grid of waves (the count is the device's), logits of row i in row i
__global__ __launch_bounds__(kWave) void k_deferred_priors_rows(Dev E, const float *__restrict__ raw, int ld, const int32_t *__restrict__ rows,
                                                                const int32_t *__restrict__ count) {
    const int lane = threadIdx.x, n = count[0];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int rec = rows[i];
        deferred_priors_body(E, rec % E.n_games, rec, raw + (size_t)i * ld, lane);
    }
}

__global__ void k_deferred_reset(Dev E) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < E.n_games) E.pend[g] = 0;
}

}  // namespace
