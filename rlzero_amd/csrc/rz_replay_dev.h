// rz_replay_dev.h -- no kernel: what every kernel of rz_replay.hip takes -- ReplayDev (the store's pointers and sizes, passed by value),
// the constants of a record and of the meta word -- and replay_emit, one entry of the store as one row of a mini-batch, which
// k_replay_gather and k_replay_sample (rz_replay_batch.h) share.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rlzero_hip.h"
#include "rz_replay_rules.h"

namespace {

constexpr int kMaxCells = RZ_MAX_BOARD_SIZE * RZ_MAX_BOARD_SIZE;   // 256: plies of a game = threads of k_replay_add
constexpr int kRecWords = 2 * RZ_BOARD_WORDS;                      // uint64 words of a position's stones
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

}  // namespace
