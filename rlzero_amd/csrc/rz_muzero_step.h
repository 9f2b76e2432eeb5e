// rz_muzero_step.h -- the step-by-step kernels of rz_muzero.hip, one THREAD per game around rz_muzero_tree.h's walk and backup: k_mz_init
// (the roots), k_mz_select, k_mz_expand_backup.  The learned model stays outside: the caller runs it between the two.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rz_muzero_tree.h"
#include "rz_mz_roots.h"

#pragma clang fp contract(off)

namespace {

// expand_node for the roots (from the initial inference), optional Dirichlet mix
// (add_exploration_noise: prior * (1 - frac) + noise * frac), fresh MinMaxStats.
__global__ void k_mz_init(MzDev E, const float *probs, const double *noise, double frac, const uint8_t *mask) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    if (mask != nullptr && !mask[g]) return;
    const long long base = (long long)g * E.cap;
    const double *noise_row = noise != nullptr ? noise + (long long)g * E.n_actions : nullptr;
    E.nodes[base] = mz_root_record();   // (the rule: rz_mz_roots.h -- the search that starts from observations calls it too)
    for (int a = 0; a < E.n_actions; ++a)
        E.nodes[base + 1 + a] = mz_root_child(mz_root_prior(probs[(long long)g * E.n_actions + a], noise_row, a, frac));
    const MzRootStart start = mz_root_start(E.n_actions);
    E.top[g] = start.top;
    E.vmin[g] = start.lo;
    E.vmax[g] = start.hi;
    E.depth[g] = start.depth;
}

__global__ void k_mz_select(MzDev E, int32_t *parent, int32_t *action, int32_t *leaf, const uint8_t *mask) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    int par = 0, act = 0, lf = 0;
    if (mask == nullptr || mask[g]) mz_select_one(E, g, par, act, lf);
    parent[g] = par;
    action[g] = act;
    leaf[g] = lf;
}

__global__ void k_mz_expand_backup(MzDev E, const float *reward, const float *probs, const float *value,
                                   const uint8_t *mask) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    if (mask != nullptr && !mask[g]) return;
    mz_expand_backup_one(E, g, reward[g], probs + (long long)g * E.n_actions, value[g]);
}

}  // namespace
