// rz_muzero_step.h -- the step-by-step kernels of rz_muzero.hip, one THREAD per game around rz_muzero_tree.h's walk and backup: k_mz_init
// (the roots), k_mz_select, k_mz_expand_backup.  The learned model stays outside: the caller runs it between the two.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rz_muzero_tree.h"

#pragma clang fp contract(off)

namespace {

// expand_node for the roots (from the initial inference), optional Dirichlet mix
// (add_exploration_noise: prior * (1 - frac) + noise * frac), fresh MinMaxStats.
__global__ void k_mz_init(MzDev E, const float *probs, const double *noise, double frac, const uint8_t *mask) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    if (mask != nullptr && !mask[g]) return;
    const long long base = (long long)g * E.cap;
    E.nodes[base] = MzNode{0, 1, 0.0, 0.0, 0.0f, 0};
    for (int a = 0; a < E.n_actions; ++a) {
        double p = (double)probs[(long long)g * E.n_actions + a];
        if (noise != nullptr) p = p * (1.0 - frac) + noise[(long long)g * E.n_actions + a] * frac;
        E.nodes[base + 1 + a] = MzNode{0, -1, 0.0, p, 0.0f, 0};
    }
    E.top[g] = 1 + E.n_actions;
    E.vmin[g] = INFINITY;   // MinMaxStats(): minimum = +MAX, maximum = -MAX
    E.vmax[g] = -INFINITY;
    E.depth[g] = 0;
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
