// rz_mz_learn_grad.h -- the gradient kernel of rz_mz_learn.hip: the records every kernel of the learner takes (MzlWeights, MzlTable,
// MzlBatch), the LDS a tile needs (mzl_act_stride, mzl_lds_floats: the host sizes the launch with them), the matrix-vector pieces
// (gemv_fwd, gemv_bwd, outer_acc, col_sum, store16) and k_mzl_grad, a tile of R batch rows through the K + 1 unroll steps and back.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rlzero_hip.h"
#include "rz_mz_learn.h"

namespace {

using namespace rzmzl;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kScal = 16;            // floats of a (row, step) record: den, free, imin, imax, dvalue, dreward, dlogits[8]
constexpr int kLdsBytes = 64 * 1024;
constexpr int kMaxRows = 4;          // the largest tile

enum { S_DEN = 0, S_FREE = 1, S_IMIN = 2, S_IMAX = 3, S_VALUE = 4, S_REWARD = 5, S_LOGITS = 6 };

struct MzlWeights {
    const float *p[RZ_MZL_TENSORS];
};
struct MzlTable {
    float *p[RZ_MZL_TENSORS];
    int off[RZ_MZL_TENSORS + 1];
};
struct MzlBatch {
    const float *obs;            // [n][D]
    const long long *actions;    // [n][K]
    const float *tv, *tr;        // [n][K + 1]
    const float *tp;             // [n][K + 1][A]
    const float *mask;           // [n][K + 1]
    const float *weights;        // [n] or NULL
    long long n;
};

// floats of LDS a tile of R rows takes
__host__ __device__ inline int mzl_act_stride(int K) { return (3 + 4 * K) * kH; }
__host__ __device__ inline int mzl_lds_floats(int R, int K) {
    return R * (mzl_act_stride(K) + (K + 1) * kScal + 4 * kH + RZ_MZL_MAX_OBS + RZ_MZL_MAX_UNROLL) + 4 * kMaxRows;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// y[m] += sum_{i < n_in} W[j][i] x[r_m][i] for the rows r_m = q + 4 m of wave q (x: LDS, row stride xs)
template <int R, bool VEC>
__device__ __forceinline__ void gemv_fwd(const float *__restrict__ W, int ld, int n_in, const float *x, int xs, int q, int j, float *y) {
    constexpr int RPW = (R + kWaves - 1) / kWaves;
    if (VEC) {
        const float4 *w4 = (const float4 *)(W + j * kH);
#pragma unroll 4
        for (int i = 0; i < kH / 4; ++i) {
            const float4 w = w4[i];
#pragma unroll
            for (int m = 0; m < RPW; ++m) {
                const int r = q + kWaves * m;
                if (r < R) {
                    const float4 v = *(const float4 *)(x + r * xs + 4 * i);
                    y[m] = fmaf(w.x, v.x, y[m]), y[m] = fmaf(w.y, v.y, y[m]), y[m] = fmaf(w.z, v.z, y[m]), y[m] = fmaf(w.w, v.w, y[m]);
                }
            }
        }
    } else {
        for (int i = 0; i < n_in; ++i) {
            const float w = W[j * ld + i];
#pragma unroll
            for (int m = 0; m < RPW; ++m) {
                const int r = q + kWaves * m;
                if (r < R) y[m] = fmaf(w, x[r * xs + i], y[m]);
            }
        }
    }
}

// y[m] += sum_{j < 64} W[j][i] dy[r_m][j] (dy: LDS, row stride 64): the transposed product, lanes along a row of W
template <int R>
__device__ __forceinline__ void gemv_bwd(const float *__restrict__ W, int ld, int i, const float *dy, int q, float *y) {
    constexpr int RPW = (R + kWaves - 1) / kWaves;
#pragma unroll 4
    for (int j = 0; j < kH; j += 4) {
        const float w0 = W[j * ld + i], w1 = W[(j + 1) * ld + i], w2 = W[(j + 2) * ld + i], w3 = W[(j + 3) * ld + i];
#pragma unroll
        for (int m = 0; m < RPW; ++m) {
            const int r = q + kWaves * m;
            if (r < R) {
                const float4 v = *(const float4 *)(dy + r * kH + j);
                y[m] = fmaf(w0, v.x, y[m]), y[m] = fmaf(w1, v.y, y[m]), y[m] = fmaf(w2, v.z, y[m]), y[m] = fmaf(w3, v.w, y[m]);
            }
        }
    }
}

// acc[c] += sum_r dy[r][j] x[r][16 q + c]: the thread's 16 elements of a 64 x 64 weight gradient, every row of the tile in order
template <int R>
__device__ __forceinline__ void outer_acc(float *acc, const float *dy, const float *x, int xs, int j, int q) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float d = dy[r * kH + j];
#pragma unroll
        for (int c = 0; c < 16; c += 4) {
            const float4 v = *(const float4 *)(x + r * xs + 16 * q + c);
            acc[c] = fmaf(d, v.x, acc[c]), acc[c + 1] = fmaf(d, v.y, acc[c + 1]), acc[c + 2] = fmaf(d, v.z, acc[c + 2]), acc[c + 3] = fmaf(d, v.w, acc[c + 3]);
        }
    }
}
template <int R>
__device__ __forceinline__ float col_sum(const float *dy, int j) {
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r) s += dy[r * kH + j];
    return s;
}
__device__ __forceinline__ void store16(float *dst, const float *acc) {
#pragma unroll
    for (int c = 0; c < 16; ++c) dst[c] = acc[c];
}

template <int R>
__global__ __launch_bounds__(kThreads) void k_mzl_grad(MzlWeights Wt, MzlBatch B, int D, int A, int K, int n_params, float *__restrict__ partial,
                                                       float *__restrict__ loss_partial, int32_t *__restrict__ err) {
    constexpr int RPW = (R + kWaves - 1) / kWaves;
    extern __shared__ float lds[];
    const int AS = mzl_act_stride(K);
    float *act = lds;                               // [R][AS]: step 0: h1 | s | p1; step k: d1 | s | r1 | p1
    float *scal = act + R * AS;                     // [R][K + 1][kScal]
    float *T1 = scal + R * (K + 1) * kScal;         // [R][64] each
    float *T2 = T1 + R * kH, *T3 = T2 + R * kH, *DS = T3 + R * kH;
    float *obsL = DS + R * kH;                      // [R][16]
    int *actL = (int *)(obsL + R * RZ_MZL_MAX_OBS); // [R][16]
    float *lossL = (float *)(actL + R * RZ_MZL_MAX_UNROLL);   // [4][kMaxRows]

    const int t = threadIdx.x, j = t & 63, q = t >> 6;
    const long long row0 = (long long)blockIdx.x * R;
    const int ld1 = kH + A;
    int off[RZ_MZL_TENSORS + 1];
    tensor_offsets(D, A, off);

    // ---- the tile's observations and actions; rows past n: zeros
    for (int e = t; e < R * RZ_MZL_MAX_OBS; e += kThreads) {
        const int r = e / RZ_MZL_MAX_OBS, d = e % RZ_MZL_MAX_OBS;
        obsL[e] = (row0 + r < B.n && d < D) ? B.obs[(row0 + r) * D + d] : 0.0f;
    }
    for (int e = t; e < R * RZ_MZL_MAX_UNROLL; e += kThreads) {
        const int r = e / RZ_MZL_MAX_UNROLL, k = e % RZ_MZL_MAX_UNROLL;
        long long a = 0;
        if (row0 + r < B.n && k < K) {
            a = B.actions[(row0 + r) * K + k];
            if (a < 0 || a >= A) {   // never an index
                atomicOr(err, RZ_MZ_LEARNER_BAD_ACTION);
                a = 0;
            }
        }
        actL[e] = (int)a;
    }
    for (int e = t; e < R * kH; e += kThreads) DS[e] = 0.0f;
    // the row of thread t < R: its factor on every gradient and its loss sums
    const bool my_row = t < R && row0 + t < B.n;
    const float rs = my_row ? (B.weights ? B.weights[row0 + t] : 1.0f) / (float)B.n : 0.0f;
    float lv = 0.0f, lr = 0.0f, lp = 0.0f, c_lv = 0.0f, c_lr = 0.0f, c_lp = 0.0f;   // (compensated: kahan_add)
    __syncthreads();

    // ================================================================ forward
    for (int k = 0; k <= K; ++k) {
        float *base = act + (k == 0 ? 0 : 3 * kH + (k - 1) * 4 * kH);
        float *sk = base + kH, *p1 = base + (k == 0 ? 2 * kH : 3 * kH);
        float y[RPW];
        if (k == 0) {
            // h1 = relu(rep1 obs)
#pragma unroll
            for (int m = 0; m < RPW; ++m) y[m] = Wt.p[REP1_B][j];
            gemv_fwd<R, false>(Wt.p[REP1_W], D, D, obsL, RZ_MZL_MAX_OBS, q, j, y);
#pragma unroll
            for (int m = 0; m < RPW; ++m)
                if (q + kWaves * m < R) base[(q + kWaves * m) * AS + j] = fmaxf(y[m], 0.0f);
        } else {
            // d1 = relu(dyn1 [s_{k-1}, onehot(a)])
            const float *sprev = act + (k == 1 ? kH : 3 * kH + (k - 2) * 4 * kH + kH);
#pragma unroll
            for (int m = 0; m < RPW; ++m) y[m] = Wt.p[DYN1_B][j];
            gemv_fwd<R, false>(Wt.p[DYN1_W], ld1, kH, sprev, AS, q, j, y);
#pragma unroll
            for (int m = 0; m < RPW; ++m) {
                const int r = q + kWaves * m;
                if (r < R) base[r * AS + j] = fmaxf(y[m] + Wt.p[DYN1_W][j * ld1 + kH + actL[r * RZ_MZL_MAX_UNROLL + k - 1]], 0.0f);
            }
        }
        __syncthreads();
        // the raw state = rep2 h1 / dyn2 d1, scaled inside the wave that holds the whole row; r1 = relu(rew1 d1)
#pragma unroll
        for (int m = 0; m < RPW; ++m) y[m] = Wt.p[k == 0 ? REP2_B : DYN2_B][j];
        gemv_fwd<R, true>(Wt.p[k == 0 ? REP2_W : DYN2_W], kH, kH, base, AS, q, j, y);
#pragma unroll
        for (int m = 0; m < RPW; ++m) {
            const int r = q + kWaves * m;
            if (r < R) {
                float lo = y[m], hi = y[m];
                int imin = j, imax = j;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const float olo = __shfl_xor(lo, d, 64), ohi = __shfl_xor(hi, d, 64);
                    const int oimin = __shfl_xor(imin, d, 64), oimax = __shfl_xor(imax, d, 64);
                    if (olo < lo || (olo == lo && oimin < imin)) lo = olo, imin = oimin;
                    if (ohi > hi || (ohi == hi && oimax < imax)) hi = ohi, imax = oimax;
                }
                bool free_;
                const float den = scale_den(lo, hi, &free_);
                sk[r * AS + j] = scale_fwd(y[m], lo, den);
                if (j == 0) {
                    float *rec = scal + (r * (K + 1) + k) * kScal;
                    rec[S_DEN] = den, rec[S_FREE] = free_ ? 1.0f : 0.0f, rec[S_IMIN] = __int_as_float(imin), rec[S_IMAX] = __int_as_float(imax);
                }
            }
        }
        if (k > 0) {
#pragma unroll
            for (int m = 0; m < RPW; ++m) y[m] = Wt.p[REW1_B][j];
            gemv_fwd<R, true>(Wt.p[REW1_W], kH, kH, base, AS, q, j, y);
#pragma unroll
            for (int m = 0; m < RPW; ++m)
                if (q + kWaves * m < R) base[(q + kWaves * m) * AS + 2 * kH + j] = fmaxf(y[m], 0.0f);
        }
        __syncthreads();
        // p1 = relu(pre1 s)
#pragma unroll
        for (int m = 0; m < RPW; ++m) y[m] = Wt.p[PRE1_B][j];
        gemv_fwd<R, true>(Wt.p[PRE1_W], kH, kH, sk, AS, q, j, y);
#pragma unroll
        for (int m = 0; m < RPW; ++m)
            if (q + kWaves * m < R) p1[(q + kWaves * m) * AS + j] = fmaxf(y[m], 0.0f);
        __syncthreads();
        // the heads: lane a < A a logit, lane A the value, lane A + 1 the reward
        if (j < A + 2 && (j < A + 1 || k > 0)) {
            const float *w = j < A ? Wt.p[POL_W] + j * kH : j == A ? Wt.p[VAL_W] : Wt.p[REW2_W];
            const float b = j < A ? Wt.p[POL_B][j] : j == A ? Wt.p[VAL_B][0] : Wt.p[REW2_B][0];
            const float *x = j <= A ? p1 : base + 2 * kH;
#pragma unroll
            for (int m = 0; m < RPW; ++m) {
                const int r = q + kWaves * m;
                if (r < R) {
                    float acc = b;
                    for (int i = 0; i < kH; ++i) acc = fmaf(w[i], x[r * AS + i], acc);
                    scal[(r * (K + 1) + k) * kScal + (j < A ? S_LOGITS + j : j == A ? S_VALUE : S_REWARD)] = acc;
                }
            }
        }
        __syncthreads();
        // the losses of row t at this step, and what they send back
        if (t < R) {
            float *rec = scal + (t * (K + 1) + k) * kScal;
            const long long at = (row0 + t) * (K + 1) + k;
            const float g = step_grad_scale<float>(k, K) * rs;
            float tpr[RZ_MZL_MAX_ACTIONS], lg[RZ_MZL_MAX_ACTIONS], dl[RZ_MZL_MAX_ACTIONS];
#pragma unroll
            for (int a = 0; a < RZ_MZL_MAX_ACTIONS; ++a) {
                lg[a] = a < A ? rec[S_LOGITS + a] : 0.0f;
                tpr[a] = (my_row && a < A) ? B.tp[at * A + a] : 0.0f;
            }
            float dv, dr = 0.0f;
            const float e_v = sq_loss_grad(rec[S_VALUE], my_row ? B.tv[at] : 0.0f, 0.25f * g, &dv);
            const float e_p = policy_loss_grad(lg, tpr, A, my_row ? B.mask[at] : 0.0f, g, dl);
            float e_r = 0.0f;
            if (k > 0) e_r = sq_loss_grad(rec[S_REWARD], my_row ? B.tr[at] : 0.0f, g, &dr);
            if (my_row) kahan_add(&lv, &c_lv, e_v), kahan_add(&lr, &c_lr, e_r), kahan_add(&lp, &c_lp, e_p);
            rec[S_VALUE] = dv, rec[S_REWARD] = dr;
#pragma unroll
            for (int a = 0; a < RZ_MZL_MAX_ACTIONS; ++a)
                if (a < A) rec[S_LOGITS + a] = dl[a];
        }
        __syncthreads();
    }

    // ================================================================ backward
    float a_dyn1[16] = {}, a_dyn2[16] = {}, a_rew1[16] = {}, a_pre1[16] = {}, a_rep2[16] = {};
    float a_dyn1a[2] = {}, a_polw[2] = {}, a_rep1[4] = {};
    float a_valw = 0.0f, a_rew2w = 0.0f, a_hb = 0.0f;   // val.w (wave 0), rew2.w (wave 1), the head biases (wave 2)
    float a_bias_dyn1 = 0.0f, a_bias_dyn2 = 0.0f, a_bias_rew1 = 0.0f, a_bias_pre1 = 0.0f, a_bias_rep2 = 0.0f, a_bias_rep1 = 0.0f;
    for (int k = K; k >= 0; --k) {
        float *base = act + (k == 0 ? 0 : 3 * kH + (k - 1) * 4 * kH);
        float *sk = base + kH, *p1 = base + (k == 0 ? 2 * kH : 3 * kH), *r1 = base + 2 * kH;
        const float *rec0 = scal + k * kScal;   // row r: + r (K + 1) kScal
        const int RS = (K + 1) * kScal;
        float y[RPW], keep[RPW];
        // ---- T1 = d relu(pre1) from the heads; T2 = d relu(rew1); the heads' own gradients
#pragma unroll
        for (int m = 0; m < RPW; ++m) {
            const int r = q + kWaves * m;
            if (r < R) {
                const float *rec = rec0 + r * RS;
                float dp = 0.0f;
                for (int a = 0; a < A; ++a) dp = fmaf(Wt.p[POL_W][a * kH + j], rec[S_LOGITS + a], dp);
                dp = fmaf(Wt.p[VAL_W][j], rec[S_VALUE], dp);
                T1[r * kH + j] = p1[r * AS + j] > 0.0f ? dp : 0.0f;
                if (k > 0) T2[r * kH + j] = r1[r * AS + j] > 0.0f ? Wt.p[REW2_W][j] * rec[S_REWARD] : 0.0f;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float *rec = rec0 + r * RS;
            const float pv = p1[r * AS + j];
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (2 * q + c < A) a_polw[c] = fmaf(rec[S_LOGITS + 2 * q + c], pv, a_polw[c]);
            if (q == 0) a_valw = fmaf(rec[S_VALUE], pv, a_valw);
            if (q == 1 && k > 0) a_rew2w = fmaf(rec[S_REWARD], r1[r * AS + j], a_rew2w);
            if (q == 2) {
                if (j < A) a_hb += rec[S_LOGITS + j];
                if (j == 8) a_hb += rec[S_VALUE];
                if (j == 9 && k > 0) a_hb += rec[S_REWARD];
            }
        }
        __syncthreads();
        // ---- the gradient at the scaled state = what later steps sent (DS) + pre1^T T1, then back through the scaling -> T3
#pragma unroll
        for (int m = 0; m < RPW; ++m) y[m] = (q + kWaves * m < R) ? DS[(q + kWaves * m) * kH + j] : 0.0f;
        gemv_bwd<R>(Wt.p[PRE1_W], kH, j, T1, q, y);
#pragma unroll
        for (int m = 0; m < RPW; ++m) {
            const int r = q + kWaves * m;
            if (r < R) {
                const float *rec = rec0 + r * RS;
                const float sv = sk[r * AS + j];
                const float sum_dy = wave_sum(y[m]), sum_dyy = wave_sum(y[m] * sv);
                float dlo, dhi;
                scale_bwd_ends(sum_dy, sum_dyy, rec[S_DEN], rec[S_FREE] != 0.0f, &dlo, &dhi);
                T3[r * kH + j] = scale_bwd_elem(y[m], rec[S_DEN], j, __float_as_int(rec[S_IMIN]), __float_as_int(rec[S_IMAX]), dlo, dhi);
            }
        }
        outer_acc<R>(a_pre1, T1, sk, AS, j, q);
        if (q == 3) a_bias_pre1 += col_sum<R>(T1, j);
        if (k > 0) {
#pragma unroll
            for (int m = 0; m < RPW; ++m) keep[m] = 0.0f;
            gemv_bwd<R>(Wt.p[REW1_W], kH, j, T2, q, keep);
            outer_acc<R>(a_rew1, T2, base, AS, j, q);
            if (q == 1) a_bias_rew1 += col_sum<R>(T2, j);
        }
        __syncthreads();
        if (k > 0) {
            // ---- T1 = d relu(dyn1) = (rew1^T T2 + dyn2^T T3) where d1 > 0
            gemv_bwd<R>(Wt.p[DYN2_W], kH, j, T3, q, keep);
#pragma unroll
            for (int m = 0; m < RPW; ++m) {
                const int r = q + kWaves * m;
                if (r < R) T1[r * kH + j] = base[r * AS + j] > 0.0f ? keep[m] : 0.0f;
            }
            outer_acc<R>(a_dyn2, T3, base, AS, j, q);
            if (q == 0) a_bias_dyn2 += col_sum<R>(T3, j);
            __syncthreads();
            // ---- DS = dyn1[:, :64]^T T1, halved unless it reaches step 0's state
            const float *sprev = act + (k == 1 ? kH : 3 * kH + (k - 2) * 4 * kH + kH);
#pragma unroll
            for (int m = 0; m < RPW; ++m) y[m] = 0.0f;
            gemv_bwd<R>(Wt.p[DYN1_W], ld1, j, T1, q, y);
#pragma unroll
            for (int m = 0; m < RPW; ++m)
                if (q + kWaves * m < R) DS[(q + kWaves * m) * kH + j] = y[m] * state_grad_scale<float>(k - 1);
            outer_acc<R>(a_dyn1, T1, sprev, AS, j, q);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int a = actL[r * RZ_MZL_MAX_UNROLL + k - 1];
                const float d = T1[r * kH + j];
                if (a == 2 * q) a_dyn1a[0] += d;
                if (a == 2 * q + 1) a_dyn1a[1] += d;
            }
            if (q == 2) a_bias_dyn1 += col_sum<R>(T1, j);
            __syncthreads();
        } else {
            // ---- T1 = d relu(rep1) = rep2^T T3 where h1 > 0; rep2's and rep1's gradients
#pragma unroll
            for (int m = 0; m < RPW; ++m) y[m] = 0.0f;
            gemv_bwd<R>(Wt.p[REP2_W], kH, j, T3, q, y);
#pragma unroll
            for (int m = 0; m < RPW; ++m) {
                const int r = q + kWaves * m;
                if (r < R) T1[r * kH + j] = base[r * AS + j] > 0.0f ? y[m] : 0.0f;
            }
            outer_acc<R>(a_rep2, T3, base, AS, j, q);
            if (q == 0) a_bias_rep2 += col_sum<R>(T3, j);
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float d = T1[r * kH + j];
#pragma unroll
                for (int c = 0; c < 4; ++c) a_rep1[c] = fmaf(d, obsL[r * RZ_MZL_MAX_OBS + 4 * q + c], a_rep1[c]);
            }
            if (q == 1) a_bias_rep1 += col_sum<R>(T1, j);
        }
    }

    // ================================================================ the workgroup's partial gradient and loss sums
    float *out = partial + (long long)blockIdx.x * n_params;
    store16(out + off[REP2_W] + j * kH + 16 * q, a_rep2);
    store16(out + off[DYN2_W] + j * kH + 16 * q, a_dyn2);
    store16(out + off[REW1_W] + j * kH + 16 * q, a_rew1);
    store16(out + off[PRE1_W] + j * kH + 16 * q, a_pre1);
    store16(out + off[DYN1_W] + j * ld1 + 16 * q, a_dyn1);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (2 * q + c < A) {
            out[off[DYN1_W] + j * ld1 + kH + 2 * q + c] = a_dyn1a[c];
            out[off[POL_W] + (2 * q + c) * kH + j] = a_polw[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (4 * q + c < D) out[off[REP1_W] + j * D + 4 * q + c] = a_rep1[c];
    if (q == 0) out[off[VAL_W] + j] = a_valw, out[off[DYN2_B] + j] = a_bias_dyn2, out[off[REP2_B] + j] = a_bias_rep2;
    if (q == 1) out[off[REW2_W] + j] = a_rew2w, out[off[REW1_B] + j] = a_bias_rew1, out[off[REP1_B] + j] = a_bias_rep1;
    if (q == 2) {
        out[off[DYN1_B] + j] = a_bias_dyn1;
        if (j < A) out[off[POL_B] + j] = a_hb;
        if (j == 8) out[off[VAL_B]] = a_hb;
        if (j == 9) out[off[REW2_B]] = a_hb;
    }
    if (q == 3) out[off[PRE1_B] + j] = a_bias_pre1;
    if (t < R) {
        const float w = B.weights && my_row ? B.weights[row0 + t] : 1.0f;
        lossL[t] = (0.25f * lv + lr + lp) * w, lossL[kMaxRows + t] = lv, lossL[2 * kMaxRows + t] = lr, lossL[3 * kMaxRows + t] = lp;
    }
    __syncthreads();
    if (t < 4) {
        float s = 0.0f, c = 0.0f;
        for (int r = 0; r < R; ++r) kahan_add(&s, &c, lossL[t * kMaxRows + r]);   // (rows past n hold zeros)
        loss_partial[4 * blockIdx.x + t] = s;
    }
}

}  // namespace
