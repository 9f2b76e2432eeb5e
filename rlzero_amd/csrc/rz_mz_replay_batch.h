// rz_mz_replay_batch.h -- the mini-batch kernels of rz_mz_replay.hip, a thread per (entry, unroll step): k_mzr_gather (the caller's
// draws) and k_mzr_sample (the draws made here: rz_mz_target.h, draw).  Both write through mzr_emit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rz_mz_replay_dev.h"
#include "rz_mz_target.h"

namespace {

// row k of output entry b from position `pos` of the episode in `slot` (length `len`, 0 <= pos < len)
// VT (here and in the two kernels below; rz_mz_replay_set_value_transform): tv and tr through value_h (rz_mz_target.h: unroll_row<VT>)
template <bool VT>
__device__ __forceinline__ void mzr_emit(const MzrDev &R, const MzrOut &O, long long b, int k, int slot, int len, int pos, long long filler) {
    const long long base = (long long)slot * R.T;
    const int K = R.K, A = R.A, D = R.D;
    const rzmzt::Row r = rzmzt::unroll_row<VT>(R.reward + base, R.root_value + base, R.action + base, len, pos, k, R.td, R.disc, filler);
    const long long o = b * (K + 1) + k;
    O.tv[o] = r.value;
    O.tr[o] = r.reward;
    O.mask[o] = r.mask;
    const float uniform = rzmzt::uniform_policy(A);
    for (int a = 0; a < A; ++a) O.tp[o * A + a] = r.policy_step >= 0 ? R.policy[(base + r.policy_step) * A + a] : uniform;
    if (k > 0) {
        O.actions[b * K + (k - 1)] = r.action;
    } else {
        for (int d = 0; d < D; ++d) O.obs[b * D + d] = R.obs[(base + pos) * D + d];
    }
}

// A thread per (entry, unroll step).  draws int64 [n][K + 2]: episode (0 = the oldest held), position, the K filler actions.
template <bool VT = false>
__global__ __launch_bounds__(kThreads) void k_mzr_gather(MzrDev R, MzrOut O, const long long *__restrict__ draws, long long oldest, long long count,
                                                          long long n) {
    const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int K = R.K;
    const long long b = tid / (K + 1);
    const int k = (int)(tid % (K + 1));
    if (b >= n) return;
    const long long *dr = draws + b * (K + 2);
    const long long ep = dr[0], pos = dr[1];
    bool bad = ep < 0 || ep >= count;
    int slot = 0, len = 0;
    if (!bad) {
        slot = mzr_slot(R, oldest + ep);
        len = mzr_length(R, slot);
        bad = pos < 0 || pos >= len;
    }
    for (int j = 0; j < K; ++j) bad = bad || dr[2 + j] < 0 || dr[2 + j] >= R.A;   // every thread of the entry comes to the same verdict
    if (bad) {   // an index from the device: nothing of this entry is read or written
        if (k == 0) atomicOr(R.err, kFlagBadIndex);
        return;
    }
    mzr_emit<VT>(R, O, b, k, slot, len, (int)pos, k > 0 ? dr[2 + k - 1] : 0);
}

// The same rows with the draws made here: counter c = b (K + 2) + j of update `step` (rz_mz_target.h: draw) -- j = 0 the episode,
// uniform over the episodes held; j = 1 the position, uniform over that episode's length; j = 2 + k the filler action of step k.
template <bool VT = false>
__global__ __launch_bounds__(kThreads) void k_mzr_sample(MzrDev R, MzrOut O, unsigned long long seed, unsigned long long step, long long oldest,
                                                          long long count, long long n) {
    const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int K = R.K;
    const long long b = tid / (K + 1);
    const int k = (int)(tid % (K + 1));
    if (b >= n) return;
    const long long ep = rzmzt::draw(seed, step, rzmzt::draw_counter((uint64_t)b, K, 0), (uint64_t)count);
    const int slot = mzr_slot(R, oldest + ep);
    const int len = mzr_length(R, slot);
    if (len == 0) {   // (an episode held is never empty)
        if (k == 0) atomicOr(R.err, kFlagBadIndex);
        return;
    }
    const int pos = (int)rzmzt::draw(seed, step, rzmzt::draw_counter((uint64_t)b, K, 1), (uint64_t)len);
    const long long filler = k > 0 ? rzmzt::draw(seed, step, rzmzt::draw_counter((uint64_t)b, K, 2 + k - 1), (uint64_t)R.A) : 0;
    mzr_emit<VT>(R, O, b, k, slot, len, pos, filler);
}

}  // namespace
