// rz_muzero_roots.h -- the root readers of rz_muzero.hip, a thread per game: k_mz_root_children, k_mz_root_stats.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rz_muzero_tree.h"

namespace {

// what: 0 = visit counts (int32 [G][A]), 1 = value sums (f64 [G][A]), 2 = rewards, 3 = priors of the root's children
__global__ void k_mz_root_children(MzDev E, int what, void *out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    const long long base = (long long)g * E.cap;
    const int fc = E.nodes[base].first_child;
    for (int a = 0; a < E.n_actions; ++a) {
        const long long o = (long long)g * E.n_actions + a;
        const MzNode c = fc >= 0 ? E.nodes[base + fc + a] : MzNode{0, -1, 0.0, 0.0, 0.0f, 0};
        if (what == 0) ((int32_t *)out)[o] = c.N;
        else if (what == 1) ((double *)out)[o] = c.value_sum;
        else if (what == 2) ((double *)out)[o] = (double)c.reward;
        else ((double *)out)[o] = c.prior;
    }
}

__global__ void k_mz_root_stats(MzDev E, int32_t *n, double *value_sum, double *vmin, double *vmax) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    const long long base = (long long)g * E.cap;
    if (n) n[g] = E.nodes[base].N;
    if (value_sum) value_sum[g] = E.nodes[base].value_sum;
    if (vmin) vmin[g] = E.vmin[g];
    if (vmax) vmax[g] = E.vmax[g];
}

}  // namespace
