// rz_replay_add.h -- the way in of rz_replay.hip: k_replay_add forms the positions of finished games from their move lists.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rlzero_hip.h"
#include "rz_replay_dev.h"
#include "rz_replay_rules.h"

namespace {

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

}  // namespace
