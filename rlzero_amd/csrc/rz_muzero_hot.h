// rz_muzero_hot.h -- the LDS twins of rz_muzero_tree.h's walk and backup, for k_mz_search's TREE_LDS trees (rz_muzero_search.h, whose
// file comment says why): the record MzHot, the interleaved fp64 divisions (mz_divide), the quad exchanges, the touch of a hidden-state
// row, mz_descend_hot and mz_grow_backup_hot -- the four lanes of a quad on one tree.  Same operations on the same operands as
// mz_descend / mz_grow_backup: same bits.  No kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rlzero_hip.h"
#include "rz_muzero_tree.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMzHidden = 64;   // floats of a hidden state (= kMzH of rz_mz_pack.h)
struct __attribute__((aligned(16))) MzHot {
    int32_t N, first_child;
    double value_sum, prior, q;
};
static_assert(sizeof(MzHot) == 32, "MzHot layout");

// N IEEE fp64 divisions x[i] / y[i] with their dependent chains INTERLEAVED: a division is a chain of 11 dependent fp64
// operations (~200 cycles for a wave, however few lanes are active), and the compiler emits one chain after the other.
// The operations are exactly those of its own expansion of `x / y` (v_div_scale x 2, v_rcp, the Newton steps,
// v_div_fmas, v_div_fixup): same bits.
template <int N>
__device__ __forceinline__ void mz_divide(const double (&x)[N], const double (&y)[N], double (&out)[N]) {
    double d[N], ns[N], r[N], e[N], m[N];
    bool flag[N], unused;
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] = __builtin_amdgcn_div_scale(x[i], y[i], false, &unused);
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = __builtin_amdgcn_rcp(d[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = __builtin_fma(-d[i], r[i], 1.0);
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = __builtin_fma(r[i], e[i], r[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = __builtin_fma(-d[i], r[i], 1.0);
#pragma unroll
    for (int i = 0; i < N; ++i) ns[i] = __builtin_amdgcn_div_scale(x[i], y[i], true, &flag[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = __builtin_fma(r[i], e[i], r[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) m[i] = ns[i] * r[i];
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = __builtin_fma(-d[i], m[i], ns[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) m[i] = __builtin_amdgcn_div_fmas(e[i], r[i], m[i], flag[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = __builtin_amdgcn_div_fixup(m[i], y[i], x[i]);
}

// the value of lane l ^ 1 / l ^ 2 (DPP quad_perm: one VALU move per dword)
__device__ __forceinline__ int mz_quad_xor1(int x) { return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ int mz_quad_xor2(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true); }
template <int WHICH>
__device__ __forceinline__ double mz_quad_xor(double x) {
    const long long b = __double_as_longlong(x);
    const int lo = (int)b, hi = (int)(b >> 32);
    const int olo = WHICH == 1 ? mz_quad_xor1(lo) : mz_quad_xor2(lo), ohi = WHICH == 1 ? mz_quad_xor1(hi) : mz_quad_xor2(hi);
    return __longlong_as_double(((long long)ohi << 32) | (unsigned int)olo);
}

// the value of lane J of the quad in all four
template <int J>
__device__ __forceinline__ double mz_quad_bcast(double x) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, J * 0x55, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), J * 0x55, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Touch a hidden-state row the walk may need next (global_load into a register nobody reads: the line is on its way to
// L2 / L1 while the walk goes on).  `sink` keeps the destination register reserved until the caller has waited for its
// vector memory operations (they return in order, and the compiler's own s_waitcnt counts only get stricter).
__device__ __forceinline__ void mz_touch(const float *p, float &sink) {
    asm volatile("global_load_dword %0, %1, off" : "+v"(sink) : "v"(p) : "memory");
}
__device__ __forceinline__ void mz_touch_done(float &sink) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(sink) : : "memory");
}

// mz_descend on the MzHot trees with the FOUR lanes of a quad walking one tree together: lane `ca` of the quad scores
// ONE child of a level (the two divisions of a score are the walk's long operations; a single wave issues one
// instruction every ~5 cycles, so the walk is written for few instructions: straight-line, selects instead of
// branches), the quad then takes the best (score, action) -- larger action on a tie, as the sequential scan -- and all
// four lanes step down together.  Up to 2 actions lanes 2, 3 mirror lanes 0, 1 (one exchange); 3 or 4 actions take a
// second exchange; more fall back to every lane scanning the children ca, ca + 4, ...
// Every lane returns the same (depth, parent, action, leaf).
// AFIX > 0: the action count is a compile-time constant (2 for CartPole's whole MOVES: the per-level code loses its runtime tests)
template <int AFIX = 0, typename HotP, typename PathP, typename TabP>
__device__ __forceinline__ int mz_descend_hot(const MzDev &E, HotP hot, PathP path, TabP pb_log, TabP sq_tab, double lo, double hi,
                                              int ca, const float *hidden_g, float &sink, int &par_out, int &act_out, int &leaf_out) {
    const int A = AFIX > 0 ? AFIX : E.n_actions;
    int node = 0, depth = 0, last_action = 0, par = 0;
    path[0] = 0;
    int fc = hot[0].first_child, pn = hot[0].N;
    const bool ranged = hi > lo;   // MinMaxStats.normalize
    const double divisor = ranged ? hi - lo : 1.0;
    if (A <= 4) {
        const int my_a = A <= 2 ? (ca & 1) : ca;
        const bool has_child = my_a < A;
        const int a_eff = has_child ? my_a : 0;
        while (fc >= 0 && depth + 1 < E.path_stride) {
            const MzHot ch = hot[fc + a_eff];
            const int idx = pn <= E.n_sims + 1 ? pn : E.n_sims + 1;
            const double pb_c0 = pb_log[idx] + E.pb_c_init;
            const double sq = pn <= E.n_sims + 1 ? sq_tab[idx] : sqrt((double)pn);
            const double num[2] = {sq, ch.q - lo}, den[2] = {(double)(ch.N + 1), divisor};
            double quo[2];
            mz_divide<2>(num, den, quo);
            const double own = pb_c0 * quo[0] * ch.prior + (ch.N > 0 ? (ranged ? quo[1] : ch.q) : 0.0);
            const double score = has_child ? own : -INFINITY;
            // the neighbour's child (action my_a ^ 1) wins with a larger score, or the same score and the larger action
            double ob = mz_quad_xor<1>(score);
            int ofc = mz_quad_xor1(ch.first_child), on = mz_quad_xor1(ch.N);
            bool take = ob > score || (ob == score && (my_a & 1) == 0);
            double best = take ? ob : score;
            int besta = take ? (my_a ^ 1) : my_a, best_fc = take ? ofc : ch.first_child, best_n = take ? on : ch.N;
            if (A > 2) {
                ob = mz_quad_xor<2>(best);
                const int oa = mz_quad_xor2(besta);
                ofc = mz_quad_xor2(best_fc);
                on = mz_quad_xor2(best_n);
                take = ob > best || (ob == best && oa > besta);
                besta = take ? oa : besta;
                best_fc = take ? ofc : best_fc;
                best_n = take ? on : best_n;
            }
            par = node;
            last_action = besta;
            node = fc + besta;
            fc = best_fc;
            pn = best_n;
            depth += 1;
            path[depth] = node;
            // the node stepped into is the parent whose hidden state the gather reads if the walk ends below it: the
            // quad touches the four 64-byte pieces of its row now (~1 us from the Infinity Cache otherwise)
            mz_touch(hidden_g + (long long)node * kMzHidden + 16 * ca, sink);
        }
    } else {
        while (fc >= 0 && depth + 1 < E.path_stride) {
            const int idx = pn <= E.n_sims + 1 ? pn : E.n_sims + 1;
            const double pb_c0 = pb_log[idx] + E.pb_c_init;
            const double sq = pn <= E.n_sims + 1 ? sq_tab[idx] : sqrt((double)pn);
            double best = -INFINITY;
            int besta = -1, best_fc = -1, best_n = 0;
            for (int a = ca; a < A; a += 4) {
                const MzHot ch = hot[fc + a];
                const double num[2] = {sq, ch.q - lo}, den[2] = {(double)(ch.N + 1), divisor};
                double quo[2];
                mz_divide<2>(num, den, quo);
                const double score = pb_c0 * quo[0] * ch.prior + (ch.N > 0 ? (ranged ? quo[1] : ch.q) : 0.0);
                if (score >= best) {  // the later (larger) action wins a tie
                    best = score;
                    besta = a;
                    best_fc = ch.first_child;
                    best_n = ch.N;
                }
            }
            {   // best of the quad
                double ob = mz_quad_xor<1>(best);
                int oa = mz_quad_xor1(besta), ofc = mz_quad_xor1(best_fc), on = mz_quad_xor1(best_n);
                bool take = ob > best || (ob == best && oa > besta);
                best = take ? ob : best;
                besta = take ? oa : besta;
                best_fc = take ? ofc : best_fc;
                best_n = take ? on : best_n;
                ob = mz_quad_xor<2>(best);
                oa = mz_quad_xor2(besta);
                ofc = mz_quad_xor2(best_fc);
                on = mz_quad_xor2(best_n);
                take = ob > best || (ob == best && oa > besta);
                besta = take ? oa : besta;
                best_fc = take ? ofc : best_fc;
                best_n = take ? on : best_n;
            }
            par = node;
            last_action = besta;
            node = fc + besta;
            fc = best_fc;
            pn = best_n;
            depth += 1;
            path[depth] = node;
        }
    }
    par_out = par;
    act_out = last_action;
    leaf_out = node;
    return depth;
}

// expand + backup on the MzHot trees, the four lanes of a quad together: the backup takes four levels of the path at a
// time, lane `ca` the level d - ca (one load of its node, ONE value_sum / N division, one store); only
// v = reward + discount * v chains through the levels, so every lane runs that short chain on the quad's four rewards.
// A level above the root is played on the spare record `spare` (slot index relative to `hot` / `rew`; never read for a
// result).  MinMaxStats takes the quad's extremes (max / min do not depend on the order of the updates).
template <int MAXA, int AFIX = 0, typename HotP, typename RewP, typename PathP>
__device__ __forceinline__ void mz_grow_backup_hot(const MzDev &E, HotP hot, RewP rew, PathP path, int spare, int ca, int depth, int &top,
                                                   double &lo, double &hi, float reward_g, const float *probs, float value_g) {
    const int leaf = path[depth];
    const int A = AFIX > 0 ? AFIX : E.n_actions;
    if (top + A > E.cap) {
        atomicOr(E.err, RZ_FLAG_ARENA_FULL);
    } else {
        rew[leaf] = reward_g;
        hot[leaf].first_child = top;
#pragma unroll
        for (int a = 0; a < MAXA; ++a) {
            if (a < A) {
                hot[top + a] = MzHot{0, -1, 0.0, (double)probs[a], 0.0};
                rew[top + a] = 0.0f;
            }
        }
        top += A;
    }
    double v = (double)value_g;
    for (int d = depth; d >= 0; d -= 4) {
        const bool real = d - ca >= 0;
        const int slot = real ? path[real ? d - ca : 0] : spare;
        const double vs = hot[slot].value_sum, r = (double)rew[slot];
        const int n = real ? hot[slot].N + 1 : 1;
        const double r0 = mz_quad_bcast<0>(r), r1 = mz_quad_bcast<1>(r), r2 = mz_quad_bcast<2>(r), r3 = mz_quad_bcast<3>(r);
        const double v1 = r0 + E.discount * v;
        const double v2 = r1 + E.discount * v1;
        const double v3 = r2 + E.discount * v2;
        const double mine = ca == 0 ? v : ca == 1 ? v1 : ca == 2 ? v2 : v3;
        v = r3 + E.discount * v3;
        const double sum = real ? vs + mine : 0.0;
        const double nv = sum / (double)n;
        hot[slot].value_sum = sum;
        hot[slot].N = real ? n : 0;
        hot[slot].q = r + E.discount * nv;
        double up = real ? nv : -INFINITY, dn = real ? nv : INFINITY;   // MinMaxStats.update over the quad's levels
        double o = mz_quad_xor<1>(up);
        up = o > up ? o : up;
        o = mz_quad_xor<2>(up);
        up = o > up ? o : up;
        o = mz_quad_xor<1>(dn);
        dn = o < dn ? o : dn;
        o = mz_quad_xor<2>(dn);
        dn = o < dn ? o : dn;
        hi = up > hi ? up : hi;
        lo = dn < lo ? dn : lo;
    }
}

}  // namespace
