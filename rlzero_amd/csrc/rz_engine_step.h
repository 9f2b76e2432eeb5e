// rz_engine_step.h -- the step-by-step tree kernels of rz_engine.hip, one wave per game around rz_tree.h's select_body and
// expand_backup_body: k_select, k_expand_backup (log-probabilities or probabilities), k_expand_backup_raw and k_tree_step_raw (the
// heads finished in the tree step), k_tree_step (backup of one simulation and selection of the next in one launch) and k_tree_step_vl,
// the sequential restatement of the level-synchronous in-flight kernel (rz_engine_ml.h).
#pragma once

#include <hip/hip_runtime.h>

#include "rz_tree.h"

namespace {

using namespace rzt;   // rz_tree.h: Dev, RawHeads and the two bodies

__global__ __launch_bounds__(kWave) void k_select(Dev E, float *obs) {
    __builtin_amdgcn_s_setprio(3);  // latency-bound: issue ahead of a co-resident MFMA kernel
    select_body<false, kWords, NoHook, true>(E, obs, blockIdx.x, threadIdx.x);
}

template <typename VT, bool PROBS = false>
__global__ __launch_bounds__(kWave) void k_expand_backup(Dev E, const float *logp, const VT *value) {
    __builtin_amdgcn_s_setprio(3);
    expand_backup_body<VT, PROBS>(E, logp, value, blockIdx.x, threadIdx.x);
}

__global__ __launch_bounds__(kWave) void k_expand_backup_raw(Dev E, RawHeads rh) {
    __builtin_amdgcn_s_setprio(3);
    expand_backup_body<float, false, true>(E, nullptr, nullptr, blockIdx.x, threadIdx.x, rh);
}

__global__ __launch_bounds__(kWave) void k_tree_step_raw(Dev E, RawHeads rh, float *obs) {
    __builtin_amdgcn_s_setprio(3);
    expand_backup_body<float, false, true>(E, nullptr, nullptr, blockIdx.x, threadIdx.x, rh);
    __syncthreads();
    select_body<false, kWords, NoHook, true>(E, obs, blockIdx.x, threadIdx.x);
}

// EXPAND + BACKUP of simulation s and SELECT + STEP of simulation s+1 in one launch (same
// wave, same game): saves a kernel boundary per simulation.  The barrier makes the tree
// updates of the first half visible to the loads of the second.
template <typename VT>
__global__ __launch_bounds__(kWave) void k_tree_step(Dev E, const float *logp, const VT *value, float *obs) {
    __builtin_amdgcn_s_setprio(3);
    expand_backup_body<VT>(E, logp, value, blockIdx.x, threadIdx.x);
    __syncthreads();
    select_body<false, kWords, NoHook, true>(E, obs, blockIdx.x, threadIdx.x);
}

// K simulations in flight (opt-in): the game's wave backs up the kb pending slots of the previous step one after
// the other, then selects ks new ones; the barrier between two slots orders the tree updates of one before the loads
// of the next (same wave: s_waitcnt + s_barrier).  kb = 0 / ks = 0 give the select-only / backup-only launches.
template <bool RAW>
__global__ __launch_bounds__(kWave) void k_tree_step_vl(Dev E, const float *logp, const float *value, RawHeads rh,
                                                        float *obs, int kb, int ks) {
    __builtin_amdgcn_s_setprio(3);
#pragma unroll 1
    for (int j = 0; j < kb; ++j) {
        expand_backup_body<float, false, RAW, true>(E, logp, value, blockIdx.x, threadIdx.x, rh, j);
        __syncthreads();
    }
#pragma unroll 1
    for (int j = 0; j < ks; ++j) {
        select_body<true>(E, obs, blockIdx.x, threadIdx.x, j);
        __syncthreads();
    }
}

}  // namespace
