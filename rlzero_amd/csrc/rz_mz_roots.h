// rz_mz_roots.h -- how a search's roots are made, once for every route that makes them: expand_node for a root from the initial
// inference's probabilities with the optional noise mix (add_exploration_noise: prior * (1 - frac) + noise * frac) and a fresh
// MinMaxStats.  k_mz_init (rz_muzero_step.h) writes the records with these functions from a row of probabilities the caller computed;
// the ROOTS stage of k_mz_search (rz_muzero_search.h) calls them on the row it has just formed from the observations -- the same
// operations on the same operands, so a root made inside the search launch is k_mz_init's root for that row, bit for bit.  No kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rz_muzero_tree.h"

#pragma clang fp contract(off)

namespace {

// the prior of the root's child `a`: the float32 probability widened, mixed with the game's noise row when there is one
__device__ __forceinline__ double mz_root_prior(float prob, const double *noise_row, int a, double frac) {
    double p = (double)prob;
    if (noise_row != nullptr) p = p * (1.0 - frac) + noise_row[a] * frac;
    return p;
}

// the records: an expanded root whose children are the slots 1 .. A, and an unvisited child with its prior
__device__ __forceinline__ MzNode mz_root_record() { return MzNode{0, 1, 0.0, 0.0, 0.0f, 0}; }
__device__ __forceinline__ MzNode mz_root_child(double prior) { return MzNode{0, -1, 0.0, prior, 0.0f, 0}; }

// what a game's search starts from behind its root: the slots handed out and MinMaxStats() (minimum = +MAX, maximum = -MAX)
struct MzRootStart {
    int top, depth;
    double lo, hi;
};
__device__ __forceinline__ MzRootStart mz_root_start(int n_actions) { return MzRootStart{1 + n_actions, 0, INFINITY, -INFINITY}; }

}  // namespace
