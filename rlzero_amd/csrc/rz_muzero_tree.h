// rz_muzero_tree.h -- the MuZero tree of rz_muzero.hip and its arithmetic: the node record MzNode, the engine's device view MzDev,
// select_child down to a leaf (mz_descend) and expand_node + backpropagate (mz_grow_backup) of the pseudocode, each once for every
// route -- the step-by-step kernels (rz_muzero_step.h) call them on HBM, k_mz_search (rz_muzero_search.h) on HBM or LDS.  No kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rlzero_hip.h"

#pragma clang fp contract(off)

namespace {

// A tree node is ONE 32-byte record (one sector: a level of the walk costs one load for the node and one 64-byte
// transaction for its two children instead of a scattered load per field)
struct __attribute__((aligned(16))) MzNode {
    int32_t N, first_child;   // visit count; slot of the first child (-1 = not expanded)
    double value_sum, prior;
    float reward;             // (the network's float, widened when used)
    int32_t pad;
};
static_assert(sizeof(MzNode) == 32, "MzNode layout");

struct MzDev {
    int n_games, n_actions, n_sims, cap, path_stride;
    double discount, pb_c_init;
    MzNode *nodes;
    int32_t *top, *path, *depth, *err;
    double *vmin, *vmax;
    const double *pb_log;  // [n_sims + 2]: log((n + pb_c_base + 1) / pb_c_base)
};

// Node.value(): value_sum / visit_count, 0 for an unvisited node
__device__ __forceinline__ double node_value(const MzNode &nd) {
    return nd.N > 0 ? nd.value_sum / (double)nd.N : 0.0;
}

// MinMaxStats.normalize
__device__ __forceinline__ double normalize(double v, double lo, double hi) {
    return hi > lo ? (v - lo) / (hi - lo) : v;
}

// select_child down to the first unexpanded node; max() over (score, action): ties go to the LARGER action.
// ``nodes`` = slot 0 of this game's tree, ``path`` = its path buffer, ``pb_log`` = the host's log table (each in HBM
// for the step-by-step kernels, in LDS inside k_mz_search: the arithmetic is this one function).  -> depth of the leaf
template <typename NodeP, typename PathP, typename LogP>
__device__ __forceinline__ int mz_descend(const MzDev &E, NodeP nodes, PathP path, LogP pb_log, double lo, double hi,
                                          int &par_out, int &act_out, int &leaf_out) {
    int node = 0, depth = 0, last_action = 0, par = 0;
    path[0] = 0;
    MzNode cur = nodes[0];
    while (cur.first_child >= 0 && depth + 1 < E.path_stride) {
        const int fc = cur.first_child;
        const int pn = cur.N;
        const double pb_c0 = pb_log[pn <= E.n_sims + 1 ? pn : E.n_sims + 1] + E.pb_c_init;
        const double sq = sqrt((double)pn);
        double best = -INFINITY;
        int besta = 0;
        MzNode bestn = cur;
        for (int a = 0; a < E.n_actions; ++a) {
            const MzNode ch = nodes[fc + a];
            const int cn = ch.N;
            const double pb_c = pb_c0 * (sq / (double)(cn + 1));
            const double prior_score = pb_c * ch.prior;
            double value_score = 0.0;
            if (cn > 0) value_score = normalize((double)ch.reward + E.discount * node_value(ch), lo, hi);
            const double score = prior_score + value_score;
            if (score >= best) {  // the later (larger) action wins a tie
                best = score;
                besta = a;
                bestn = ch;
            }
        }
        par = node;
        last_action = besta;
        node = fc + besta;
        cur = bestn;
        depth += 1;
        path[depth] = node;
    }
    par_out = par;
    act_out = last_action;
    leaf_out = node;
    return depth;
}

__device__ __forceinline__ void mz_select_one(const MzDev &E, int g, int &par_out, int &act_out, int &leaf_out) {
    E.depth[g] = mz_descend(E, E.nodes + (long long)g * E.cap, E.path + (long long)g * E.path_stride, E.pb_log, E.vmin[g],
                            E.vmax[g], par_out, act_out, leaf_out);
}

// expand_node(leaf, network_output) + backpropagate(search_path, value, discount, min_max_stats); `probs` = the
// n_actions probabilities of this game (MAXA > 0: a register array of MAXA entries, indexed by an unrolled loop)
template <int MAXA, typename NodeP, typename PathP>
__device__ __forceinline__ void mz_grow_backup(const MzDev &E, NodeP nodes, PathP path, int depth, int &top, double &lo,
                                               double &hi, float reward_g, const float *probs, float value_g) {
    const int leaf = path[depth];
    if (top + E.n_actions > E.cap) {
        atomicOr(E.err, RZ_FLAG_ARENA_FULL);
    } else {
        nodes[leaf].reward = reward_g;
        nodes[leaf].first_child = top;
        if (MAXA > 0) {
#pragma unroll
            for (int a = 0; a < (MAXA > 0 ? MAXA : 1); ++a)
                if (a < E.n_actions) nodes[top + a] = MzNode{0, -1, 0.0, (double)probs[a], 0.0f, 0};
        } else {
            for (int a = 0; a < E.n_actions; ++a) nodes[top + a] = MzNode{0, -1, 0.0, (double)probs[a], 0.0f, 0};
        }
        top += E.n_actions;
    }
    double v = (double)value_g;
    for (int d = depth; d >= 0; --d) {
        const int slot = path[d];
        const double sum = nodes[slot].value_sum + v;
        const int n = nodes[slot].N + 1;
        nodes[slot].value_sum = sum;
        nodes[slot].N = n;
        const double nv = sum / (double)n;
        hi = nv > hi ? nv : hi;  // MinMaxStats.update
        lo = nv < lo ? nv : lo;
        v = (double)nodes[slot].reward + E.discount * v;
    }
}

__device__ __forceinline__ void mz_expand_backup_one(const MzDev &E, int g, float reward_g, const float *probs, float value_g) {
    int top = E.top[g];
    double lo = E.vmin[g], hi = E.vmax[g];
    mz_grow_backup<0>(E, E.nodes + (long long)g * E.cap, E.path + (long long)g * E.path_stride, E.depth[g], top, lo, hi,
                      reward_g, probs, value_g);
    E.top[g] = top;
    E.vmin[g] = lo;
    E.vmax[g] = hi;
}

}  // namespace
