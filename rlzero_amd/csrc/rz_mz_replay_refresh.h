// rz_mz_replay_refresh.h -- the Reanalyse kernels of rz_mz_replay.hip: k_mzr_positions (stored observations out, to a fresh search)
// and k_mzr_update (its visit counts and root value back into the steps they came from).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rz_mz_replay_dev.h"
#include "rz_mz_target.h"

namespace {

// Reanalyse, the way out: entry i resolved to a physical (slot, position) in `where` int32 [n][2] and its stored observation in
// obs float32 [n][D].  A thread per (entry, observation element).  draws int64 [n][2] (episode, 0 = the oldest held; position), or
// NULL: the draws of refresh `step` made here (rz_mz_target.h: reanalyse_draw).  An entry out of range: where = (-1, -1), a zeroed
// row, the flag, and nothing of the store is read for it.
__global__ __launch_bounds__(kThreads) void k_mzr_positions(MzrDev R, const long long *__restrict__ draws, unsigned long long seed,
                                                             unsigned long long step, long long oldest, long long count, long long n,
                                                             int32_t *__restrict__ where, float *__restrict__ obs) {
    const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int D = R.D;
    const long long i = tid / D;
    const int d = (int)(tid % D);
    if (i >= n) return;
    long long ep, pos = -1;
    if (draws != nullptr) {
        ep = draws[2 * i], pos = draws[2 * i + 1];
    } else {
        ep = rzmzt::reanalyse_draw(seed, step, (uint64_t)i, 0, (uint64_t)count);
    }
    bool bad = ep < 0 || ep >= count;
    int slot = 0;
    if (!bad) {
        slot = mzr_slot(R, oldest + ep);
        const int len = mzr_length(R, slot);
        if (draws == nullptr && len > 0) pos = rzmzt::reanalyse_draw(seed, step, (uint64_t)i, 1, (uint64_t)len);
        bad = pos < 0 || pos >= len;   // (len == 0 with draws made here: an episode held is never empty)
    }
    if (bad) {
        if (d == 0) {
            atomicOr(R.err, kFlagBadIndex);
            where[2 * i] = -1, where[2 * i + 1] = -1;
        }
        obs[i * D + d] = 0.0f;
        return;
    }
    if (d == 0) where[2 * i] = slot, where[2 * i + 1] = (int32_t)pos;
    obs[i * D + d] = R.obs[((long long)slot * R.T + pos) * D + d];
}

// Reanalyse, the way back: the policy and the root value of step where[i] from the visit counts and the root's (N, value sum) of a
// fresh search (rz_mz_target.h: policy_of_visits, root_value_of).  A thread per (entry, action) plus one for the value; nothing
// else of the step is written.  `where` is checked again here -- slot against E, position against T and the slot's length -- and
// an entry that fails (the (-1, -1) of a refused or padded row among them) writes nothing.
__global__ __launch_bounds__(kThreads) void k_mzr_update(MzrDev R, const int32_t *__restrict__ where, long long n, const int32_t *__restrict__ visits,
                                                          const int32_t *__restrict__ root_n, const double *__restrict__ root_sum) {
    const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int A = R.A;
    const long long i = tid / (A + 1);
    const int a = (int)(tid % (A + 1));
    if (i >= n) return;
    const int slot = where[2 * i], pos = where[2 * i + 1];
    if (slot < 0 || slot >= R.E || pos < 0 || pos >= R.T) return;
    if (pos >= mzr_length(R, slot)) return;
    const long long at = (long long)slot * R.T + pos;
    if (a < A) {
        R.policy[at * A + a] = rzmzt::policy_of_visits(visits + i * A, A, a);
    } else {
        R.root_value[at] = rzmzt::root_value_of(root_n[i], root_sum[i]);
    }
}

}  // namespace
