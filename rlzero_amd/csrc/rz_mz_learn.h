// rz_mz_learn.h -- the arithmetic of the fused MuZero learner (rz_mz_learn.hip; rlzero_amd/muzero/agent.py: MuZeroAgent.learn is the
// definition).  Plain C++ templated on the scalar type, no HIP: the kernels call the per-element pieces in float, the CPU test drives
// the whole-row reference mzl_row_grad<T> in double (against torch float64 autograd) and in float.
//
// The model (rlzero_amd/muzero/network.py: MuZeroNet, hidden 64): nine Linear layers, 18 tensors in the order of net.parameters() --
// weight and bias of rep1 rep2 dyn1 dyn2 rew1 rew2 pre1 pol val -- laid one behind the other in the FLAT gradient.  One update unrolls
// K + 1 steps: step 0 = initial_inference(obs), step k = recurrent_inference(state, actions[k - 1]).
//   loss_row = 0.25 * sum_k (v_k - tv_k)^2 + sum_{k>=1} (r_k - tr_k)^2 - sum_k mask_k * sum_a tp_ka log_softmax(logits_k)_a
//   loss = mean(loss_row * weight_row); the GRADIENT of the terms of steps 1 .. K is scaled by 1 / K, the gradient into the state is
//   halved after every recurrent step (scale_gradient), the values are not.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RZL_FN __host__ __device__ __forceinline__
#else
#define RZL_FN inline
#endif

#define RZ_MZL_HIDDEN 64        /* the only hidden size */
#define RZ_MZL_MAX_OBS 16       /* D */
#define RZ_MZL_MAX_ACTIONS 8    /* A */
#define RZ_MZL_MAX_UNROLL 16    /* K */
#define RZ_MZL_TENSORS 18

namespace rzmzl {

constexpr int kH = RZ_MZL_HIDDEN;
enum Tensor { REP1_W, REP1_B, REP2_W, REP2_B, DYN1_W, DYN1_B, DYN2_W, DYN2_B, REW1_W, REW1_B, REW2_W, REW2_B, PRE1_W, PRE1_B, POL_W, POL_B, VAL_W, VAL_B };

RZL_FN int tensor_size(int t, int D, int A) {
    switch (t) {
        case REP1_W: return kH * D;
        case DYN1_W: return kH * (kH + A);
        case REP2_W: case DYN2_W: case REW1_W: case PRE1_W: return kH * kH;
        case REW2_W: case VAL_W: return kH;
        case POL_W: return A * kH;
        case POL_B: return A;
        case REW2_B: case VAL_B: return 1;
        default: return kH;   // the biases of the 64-wide layers
    }
}
// off[t] = where tensor t starts in the flat vector, off[18] = the number of parameters
RZL_FN void tensor_offsets(int D, int A, int *off) {
    int at = 0;
    for (int t = 0; t < RZ_MZL_TENSORS; ++t) off[t] = at, at += tensor_size(t, D, A);
    off[RZ_MZL_TENSORS] = at;
}

RZL_FN float mzl_exp(float x) { return expf(x); }
RZL_FN double mzl_exp(double x) { return exp(x); }
RZL_FN float mzl_log(float x) { return logf(x); }
RZL_FN double mzl_log(double x) { return log(x); }
RZL_FN float mzl_sqrt(float x) { return sqrtf(x); }
RZL_FN double mzl_sqrt(double x) { return sqrt(x); }
RZL_FN float mzl_fma(float a, float b, float c) { return fmaf(a, b, c); }
RZL_FN double mzl_fma(double a, double b, double c) { return fma(a, b, c); }

// ---- scale_hidden: y_i = (s_i - lo) / den, den = max(hi - lo, 1e-5); lo = s[imin], hi = s[imax], ties to the lowest index.
// `free`: the clamp is inactive and den carries a gradient to both ends.
template <typename T>
RZL_FN T scale_den(T lo, T hi, bool *free) {
    const T d = hi - lo, floor_ = (T)1e-5;
    *free = d >= floor_;
    return *free ? d : floor_;
}
template <typename T>
RZL_FN T scale_fwd(T s, T lo, T den) { return (s - lo) / den; }
// The gradients that reach s[imin] and s[imax] beside their own dy / den: sum_dy = sum_i dy_i, sum_dyy = sum_i dy_i y_i.
//   dL/dden = -sum_i dy_i (s_i - lo) / den^2 = -sum_dyy / den;  dhi = dL/dden, dlo = -sum_dy / den - dL/dden  (both through den only if free)
template <typename T>
RZL_FN void scale_bwd_ends(T sum_dy, T sum_dyy, T den, bool free, T *dlo, T *dhi) {
    const T dden = free ? -(sum_dyy / den) : (T)0;
    *dhi = dden;
    *dlo = -(sum_dy / den) - dden;
}
template <typename T>
RZL_FN T scale_bwd_elem(T dy, T den, int i, int imin, int imax, T dlo, T dhi) {
    T g = dy / den;
    if (i == imin) g += dlo;
    if (i == imax) g += dhi;
    return g;
}

// ---- the gradient scalings of unroll step k: its loss terms, and what flows back into the state it started from
template <typename T>
RZL_FN T step_grad_scale(int k, int K) { return k == 0 ? (T)1 : (T)(1.0 / (double)K); }
template <typename T>
RZL_FN T state_grad_scale(int k_from) { return k_from == 0 ? (T)1 : (T)0.5; }   // the state step k_from handed to step k_from + 1

// ---- squared error: -> the loss, *dx = d loss / d x * scale
template <typename T>
RZL_FN T sq_loss_grad(T x, T target, T scale, T *dx) {
    const T e = x - target;
    *dx = (T)2 * e * scale;
    return e * e;
}

// ---- -(tp . log_softmax(logits)) * mask -> the loss; dlogits_a = (softmax_a sum(tp) - tp_a) * mask * scale
template <typename T>
RZL_FN T policy_loss_grad(const T *logits, const T *tp, int A, T mask, T scale, T *dlogits) {
    T m = logits[0];
    for (int a = 1; a < A; ++a) m = logits[a] > m ? logits[a] : m;
    T z = (T)0, tsum = (T)0;
    for (int a = 0; a < A; ++a) z += mzl_exp(logits[a] - m), tsum += tp[a];
    const T lse = mzl_log(z);
    T dot = (T)0;
    for (int a = 0; a < A; ++a) {
        const T ls = logits[a] - m - lse;
        dot += tp[a] * ls;
        dlogits[a] = (mzl_exp(ls) * tsum - tp[a]) * mask * scale;
    }
    return -dot * mask;
}

// ---- a compensated sum (Kahan): the loss means are compared at the last bit, so their sums carry their rounding error along
template <typename T>
RZL_FN void kahan_add(T *sum, T *comp, T x) {
    const T y = x - *comp, t = *sum + y;
    *comp = (t - *sum) - y;
    *sum = t;
}

// ---- clip_grad_norm_(params, max_norm): the factor on every raw gradient
template <typename T>
RZL_FN T clip_coef(T norm, T max_norm) {
    const T c = max_norm / (norm + (T)1e-6);
    return c < (T)1 ? c : (T)1;
}

// ---- torch.optim.Adam, single-tensor path, one element.  The host forms the step-dependent numbers in double and casts once.
template <typename T>
struct AdamStep {
    T step_size;   // lr / (1 - beta1 ** step)
    T bc2_sqrt;    // (1 - beta2 ** step) ** 0.5
    T w1;          // 1 - beta1
    T beta2, w2;   // beta2, 1 - beta2
    T eps, weight_decay;
};
template <typename T>
RZL_FN void adam_elem(T g, const AdamStep<T> &h, T *p, T *m, T *v) {
    if (h.weight_decay != (T)0) g = g + h.weight_decay * *p;
    *m = *m + h.w1 * (g - *m);                 // exp_avg.lerp_(grad, 1 - beta1)
    *v = *v * h.beta2 + h.w2 * g * g;          // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const T denom = mzl_sqrt(*v) / h.bc2_sqrt + h.eps;
    *p = *p - h.step_size * (*m / denom);      // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// ---- the whole-row reference (host): one batch row through the K + 1 steps and back.
// params[18]: the tensors; actions int64 [K]; tv, tr, mask [K + 1]; tp [K + 1][A]; `weight` the row's importance weight, n the batch size.
// grad (flat, off[18] long) and losses[4] = sums of (weight * row loss, value, reward, policy) are ACCUMULATED.  An action outside
// 0 .. A-1 sets *bad and is read as 0.
template <typename T>
inline void mzl_linear(const T *W, const T *b, int n_out, int n_in, int ld, const T *x, T *y) {
    for (int j = 0; j < n_out; ++j) {
        T acc = b[j];
        for (int i = 0; i < n_in; ++i) acc = mzl_fma(W[j * ld + i], x[i], acc);
        y[j] = acc;
    }
}
// dW += dy x^T, db += dy, dx += W^T dy (dx may be null)
template <typename T>
inline void mzl_linear_bwd(const T *W, int n_out, int n_in, int ld, const T *x, const T *dy, T *dW, T *db, T *dx) {
    for (int j = 0; j < n_out; ++j) {
        db[j] += dy[j];
        for (int i = 0; i < n_in; ++i) {
            dW[j * ld + i] += dy[j] * x[i];
            if (dx) dx[i] = mzl_fma(W[j * ld + i], dy[j], dx[i]);
        }
    }
}

template <typename T>
struct RowScale {
    T den;
    int imin, imax;
    bool free;
};
template <typename T>
inline RowScale<T> mzl_scale_row(const T *s, T *y) {
    RowScale<T> r = {(T)0, 0, 0, false};
    for (int i = 1; i < kH; ++i) {
        if (s[i] < s[r.imin]) r.imin = i;
        if (s[i] > s[r.imax]) r.imax = i;
    }
    r.den = scale_den(s[r.imin], s[r.imax], &r.free);
    for (int i = 0; i < kH; ++i) y[i] = scale_fwd(s[i], s[r.imin], r.den);
    return r;
}
template <typename T>
inline void mzl_scale_row_bwd(const RowScale<T> &r, const T *y, const T *dy, T *ds) {
    T sum_dy = (T)0, sum_dyy = (T)0, dlo, dhi;
    for (int i = 0; i < kH; ++i) sum_dy += dy[i], sum_dyy += dy[i] * y[i];
    scale_bwd_ends(sum_dy, sum_dyy, r.den, r.free, &dlo, &dhi);
    for (int i = 0; i < kH; ++i) ds[i] = scale_bwd_elem(dy[i], r.den, i, r.imin, r.imax, dlo, dhi);
}

template <typename T>
inline void mzl_row_grad(int D, int A, int K, const T *const *params, const T *obs, const long long *actions, const T *tv, const T *tr,
                         const T *tp, const T *mask, T weight, long long n, T *grad, T *losses, int *bad) {
    constexpr int S = RZ_MZL_MAX_UNROLL + 1;
    int off[RZ_MZL_TENSORS + 1];
    tensor_offsets(D, A, off);
    const int ld1 = kH + A;
    static thread_local T h1[kH], sraw[kH], s[S][kH], p1[S][kH], d1[S][kH], r1[S][kH], x[S][kH + RZ_MZL_MAX_ACTIONS];
    RowScale<T> sc[S];
    T dlogits[S][RZ_MZL_MAX_ACTIONS], dvalue[S], dreward[S];
    const T rs = weight / (T)n;
    T lv = (T)0, lr = (T)0, lp = (T)0;
    // ---- forward
    for (int k = 0; k <= K; ++k) {
        if (k == 0) {
            mzl_linear(params[REP1_W], params[REP1_B], kH, D, D, obs, h1);
            for (int i = 0; i < kH; ++i) h1[i] = h1[i] > (T)0 ? h1[i] : (T)0;
            mzl_linear(params[REP2_W], params[REP2_B], kH, kH, kH, h1, sraw);
            dreward[0] = (T)0;
        } else {
            long long a = actions[k - 1];
            if (a < 0 || a >= A) *bad = 1, a = 0;
            for (int i = 0; i < kH; ++i) x[k][i] = s[k - 1][i];
            for (int c = 0; c < A; ++c) x[k][kH + c] = c == a ? (T)1 : (T)0;
            mzl_linear(params[DYN1_W], params[DYN1_B], kH, ld1, ld1, x[k], d1[k]);
            for (int i = 0; i < kH; ++i) d1[k][i] = d1[k][i] > (T)0 ? d1[k][i] : (T)0;
            mzl_linear(params[DYN2_W], params[DYN2_B], kH, kH, kH, d1[k], sraw);
            mzl_linear(params[REW1_W], params[REW1_B], kH, kH, kH, d1[k], r1[k]);
            for (int i = 0; i < kH; ++i) r1[k][i] = r1[k][i] > (T)0 ? r1[k][i] : (T)0;
            T reward;
            mzl_linear(params[REW2_W], params[REW2_B], 1, kH, kH, r1[k], &reward);
            lr += sq_loss_grad(reward, tr[k], step_grad_scale<T>(k, K) * rs, &dreward[k]);
        }
        sc[k] = mzl_scale_row(sraw, s[k]);
        mzl_linear(params[PRE1_W], params[PRE1_B], kH, kH, kH, s[k], p1[k]);
        for (int i = 0; i < kH; ++i) p1[k][i] = p1[k][i] > (T)0 ? p1[k][i] : (T)0;
        T logits[RZ_MZL_MAX_ACTIONS], value;
        mzl_linear(params[POL_W], params[POL_B], A, kH, kH, p1[k], logits);
        mzl_linear(params[VAL_W], params[VAL_B], 1, kH, kH, p1[k], &value);
        const T g = step_grad_scale<T>(k, K) * rs;
        lv += sq_loss_grad(value, tv[k], (T)0.25 * g, &dvalue[k]);
        lp += policy_loss_grad(logits, tp + k * A, A, mask[k], g, dlogits[k]);
    }
    losses[0] += ((T)0.25 * lv + lr + lp) * weight;
    losses[1] += lv, losses[2] += lr, losses[3] += lp;
    // ---- backward
    T ds[kH], dp1[kH], dy[kH], dsraw[kH], dd1[kH], dr1[kH], dx[kH + RZ_MZL_MAX_ACTIONS], dh1[kH];
    for (int i = 0; i < kH; ++i) ds[i] = (T)0;
    for (int k = K; k >= 0; --k) {
        for (int i = 0; i < kH; ++i) dp1[i] = (T)0;
        mzl_linear_bwd(params[POL_W], A, kH, kH, p1[k], dlogits[k], grad + off[POL_W], grad + off[POL_B], dp1);
        mzl_linear_bwd(params[VAL_W], 1, kH, kH, p1[k], &dvalue[k], grad + off[VAL_W], grad + off[VAL_B], dp1);
        for (int i = 0; i < kH; ++i) dp1[i] = p1[k][i] > (T)0 ? dp1[i] : (T)0;
        for (int i = 0; i < kH; ++i) dy[i] = ds[i];
        mzl_linear_bwd(params[PRE1_W], kH, kH, kH, s[k], dp1, grad + off[PRE1_W], grad + off[PRE1_B], dy);
        mzl_scale_row_bwd(sc[k], s[k], dy, dsraw);
        if (k == 0) {
            for (int i = 0; i < kH; ++i) dh1[i] = (T)0;
            mzl_linear_bwd(params[REP2_W], kH, kH, kH, h1, dsraw, grad + off[REP2_W], grad + off[REP2_B], dh1);
            for (int i = 0; i < kH; ++i) dh1[i] = h1[i] > (T)0 ? dh1[i] : (T)0;
            mzl_linear_bwd(params[REP1_W], kH, D, D, obs, dh1, grad + off[REP1_W], grad + off[REP1_B], (T *)nullptr);
            break;
        }
        for (int i = 0; i < kH; ++i) dr1[i] = (T)0, dd1[i] = (T)0;
        mzl_linear_bwd(params[REW2_W], 1, kH, kH, r1[k], &dreward[k], grad + off[REW2_W], grad + off[REW2_B], dr1);
        for (int i = 0; i < kH; ++i) dr1[i] = r1[k][i] > (T)0 ? dr1[i] : (T)0;
        mzl_linear_bwd(params[REW1_W], kH, kH, kH, d1[k], dr1, grad + off[REW1_W], grad + off[REW1_B], dd1);
        mzl_linear_bwd(params[DYN2_W], kH, kH, kH, d1[k], dsraw, grad + off[DYN2_W], grad + off[DYN2_B], dd1);
        for (int i = 0; i < kH; ++i) dd1[i] = d1[k][i] > (T)0 ? dd1[i] : (T)0;
        for (int i = 0; i < ld1; ++i) dx[i] = (T)0;
        mzl_linear_bwd(params[DYN1_W], kH, ld1, ld1, x[k], dd1, grad + off[DYN1_W], grad + off[DYN1_B], dx);
        for (int i = 0; i < kH; ++i) ds[i] = dx[i] * state_grad_scale<T>(k - 1);
    }
}

}  // namespace rzmzl
