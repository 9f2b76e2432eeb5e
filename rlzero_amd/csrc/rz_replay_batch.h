// rz_replay_batch.h -- the mini-batch kernels of rz_replay.hip, a workgroup per output row: k_replay_gather (the caller's entry
// indices) and k_replay_sample (the draws made here: rz_replay_rules.h, replay_index).  Both write through replay_emit (rz_replay_dev.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rz_replay_dev.h"
#include "rz_replay_rules.h"

namespace {

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
    replay_emit<kC4, kMix>(R, rzrr::replay_index(seed, step, (unsigned long long)i, (unsigned long long)n_entries), oldest, i, states, pis, zs, q, lam);
}

}  // namespace
