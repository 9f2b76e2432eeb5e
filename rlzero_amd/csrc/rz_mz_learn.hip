// rz_mz_learn.hip -- the fused MuZero learner (include/rlzero_hip.h: rz_mz_learner_*, ABI 40; the arithmetic: rz_mz_learn.h).
//
// One update is three launches on the caller's stream:
//   k_mzl_grad    a workgroup takes a tile of R batch rows through the K + 1 unroll steps and back.  The tile's activations of every
//                 step stay in LDS (per row and recurrent step four 64-wide vectors: relu(dyn1), the scaled state, relu(rew1),
//                 relu(pre1); three for step 0), the f32 weights are read where torch keeps them (L2: 84 KB shared by every
//                 workgroup).  Thread (j = lane, q = wave) owns output j of the rows q, q + 4, .. of every matrix-vector product
//                 and the 16 elements [j][16 q ..] of every 64 x 64 weight gradient, which it carries in registers over the steps.
//                 Plain fmaf on the vector unit: the products are R x 64 x 64 with R <= 4 -- a quarter of an MFMA tile's rows --
//                 and the unroll is a chain of ~90 dependent phases, so the time is barriers and latency, not the multiply rate.
//                 It writes the workgroup's partial gradient and partial loss sums.
//   k_mzl_reduce  element p of the flat gradient = the partials summed workgroup 0, 1, 2, ..; every block leaves the sum of its
//                 squares (a fixed tree); block 0 forms the four loss means.
//   k_mzl_adam    every thread sums the blocks' squares in order (the norm, the clip coefficient), then updates its element of
//                 the parameters -- in torch's own storage, through the table of 18 pointers -- and of both moments.
// No atomics on floats, no grid-wide barrier: the same inputs give the same bits.
//
// Bounds: a row past n is computed with zero inputs and zero weight and contributes nothing; an action outside 0 .. A-1 is read
// as 0 and sets the flag (k_mzl_adam then updates nothing); R is chosen on the host so that the tile fits 64 KB of LDS.
//
// This file is the host side of ONE translation unit: the kernels lie in headers beside it, one per family, each of which compiles
// alone (tests/test_csrc_headers.py) and describes its kernels where they are defined.
//   rz_mz_learn_grad.h    MzlWeights, MzlTable, MzlBatch, the LDS a tile takes (mzl_lds_floats), k_mzl_grad and its matrix-vector pieces
//   rz_mz_learn_update.h  k_mzl_reduce, k_mzl_adam
// Below: struct rz_mz_learner, the launches of an update and every extern "C" entry point.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include "rlzero_hip.h"
#include "rz_host.h"
#include "rz_mz_learn.h"

// (this order is the order of the kernels in the code object; the template instantiations follow in the order the code below names them)
#include "rz_mz_learn_grad.h"
#include "rz_mz_learn_update.h"

struct rz_mz_learner {
    rz_mz_learner_config cfg = {};
    int device = 0;
    int rows = 1;        // R: batch rows of a workgroup's tile
    int max_wg = 0, n_params = 0, n_blocks = 0;
    size_t lds_bytes = 0;
    MzlTable table = {};
    float *exp_avg = nullptr, *exp_avg_sq = nullptr;
    bool bound = false;
    float *partial = nullptr, *loss_partial = nullptr, *grad = nullptr, *sq = nullptr;
    int32_t *err = nullptr;
    DevPool pool;
};

namespace {

int ml_ready(rz_mz_learner *l) {
    if (l == nullptr) return rz_fail(RZ_ERR_ARG, "MuZero learner handle is NULL");
    return rz_on_device(l->device);
}

// the launches every update opens with: the tiles' partials, then the flat gradient, the squares and the loss means
int ml_grads(rz_mz_learner *l, const float *d_obs, const int64_t *d_actions, const float *d_tv, const float *d_tr, const float *d_tp, const float *d_mask,
             const float *d_weights, int64_t n, float *d_flat_grad, float *d_out4, hipStream_t s) {
    if (!l->bound) return rz_fail(RZ_ERR_ARG, "no parameters are bound (rz_mz_learner_bind)");
    if (n < 1 || n > l->cfg.max_batch) return rz_fail(RZ_ERR_ARG, "n outside 1 .. max_batch (%d)", l->cfg.max_batch);
    if (d_obs == nullptr || d_actions == nullptr || d_tv == nullptr || d_tr == nullptr || d_tp == nullptr || d_mask == nullptr || d_flat_grad == nullptr ||
        d_out4 == nullptr)
        return rz_fail(RZ_ERR_ARG, "NULL batch or output buffer");
    MzlWeights W;
    for (int i = 0; i < RZ_MZL_TENSORS; ++i) W.p[i] = l->table.p[i];
    const MzlBatch B = {d_obs, (const long long *)d_actions, d_tv, d_tr, d_tp, d_mask, d_weights, (long long)n};
    const int R = l->rows, n_wg = (int)((n + R - 1) / R);
    const int D = l->cfg.obs_dim, A = l->cfg.n_actions, K = l->cfg.unroll_steps;
    if (n_wg > l->max_wg) return rz_fail(RZ_ERR_INTERNAL, "more tiles than the partials hold");
    const dim3 grid((unsigned)n_wg), block(kThreads);
    if (R == 4)
        hipLaunchKernelGGL(k_mzl_grad<4>, grid, block, l->lds_bytes, s, W, B, D, A, K, l->n_params, l->partial, l->loss_partial, l->err);
    else if (R == 2)
        hipLaunchKernelGGL(k_mzl_grad<2>, grid, block, l->lds_bytes, s, W, B, D, A, K, l->n_params, l->partial, l->loss_partial, l->err);
    else
        hipLaunchKernelGGL(k_mzl_grad<1>, grid, block, l->lds_bytes, s, W, B, D, A, K, l->n_params, l->partial, l->loss_partial, l->err);
    RZ_TRY(rz_launched("k_mzl_grad"));
    hipLaunchKernelGGL(k_mzl_reduce, dim3((unsigned)l->n_blocks), block, 0, s, l->partial, l->loss_partial, n_wg, l->n_params, (long long)n, d_flat_grad,
                       l->sq, d_out4);
    return rz_launched("k_mzl_reduce");
}

}  // namespace

extern "C" {

int rz_mz_learner_create(const rz_mz_learner_config *cfg, rz_mz_learner **out) {
    if (out == nullptr || cfg == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (cfg->abi_version != RZ_ABI_VERSION) return rz_fail(RZ_ERR_ARG, "abi_version %d != library %d", cfg->abi_version, RZ_ABI_VERSION);
    if (cfg->hidden != RZ_MZL_HIDDEN) return rz_fail(RZ_ERR_ARG, "hidden must be 64");
    if (cfg->obs_dim < 1 || cfg->obs_dim > RZ_MZL_MAX_OBS) return rz_fail(RZ_ERR_ARG, "obs_dim outside 1 .. 16");
    if (cfg->n_actions < 1 || cfg->n_actions > RZ_MZL_MAX_ACTIONS) return rz_fail(RZ_ERR_ARG, "n_actions outside 1 .. 8");
    if (cfg->unroll_steps < 1 || cfg->unroll_steps > RZ_MZL_MAX_UNROLL) return rz_fail(RZ_ERR_ARG, "unroll_steps outside 1 .. 16");
    if (cfg->max_batch < 1 || cfg->max_batch > (1 << 16)) return rz_fail(RZ_ERR_ARG, "max_batch outside 1 .. 65536");
    if (!(cfg->lr > 0.0) || !(cfg->weight_decay >= 0.0) || !(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0) || !(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0) ||
        !(cfg->eps > 0.0) || !(cfg->max_norm > 0.0))
        return rz_fail(RZ_ERR_ARG, "lr, eps, max_norm > 0, weight_decay >= 0 and betas in [0, 1) are required");
    RZ_TRY(rz_claim_device(cfg->device));
    rz_mz_learner *l = new (std::nothrow) rz_mz_learner();
    if (!l) return rz_fail(RZ_ERR_OOM, "host allocation failed");
    l->cfg = *cfg;
    l->device = cfg->device;
    tensor_offsets(cfg->obs_dim, cfg->n_actions, l->table.off);
    l->n_params = l->table.off[RZ_MZL_TENSORS];
    l->n_blocks = (l->n_params + kThreads - 1) / kThreads;
    l->rows = kMaxRows;
    while (l->rows > 1 && (size_t)mzl_lds_floats(l->rows, cfg->unroll_steps) * sizeof(float) > (size_t)kLdsBytes) l->rows /= 2;
    l->lds_bytes = (size_t)mzl_lds_floats(l->rows, cfg->unroll_steps) * sizeof(float);
    l->max_wg = (cfg->max_batch + l->rows - 1) / l->rows;
    if (l->lds_bytes > (size_t)kLdsBytes) {
        delete l;
        return rz_fail(RZ_ERR_INTERNAL, "one row's activations exceed the LDS budget");
    }
    DevPool &pool = l->pool;
    const bool ok = pool.alloc(&l->partial, (long long)l->max_wg * l->n_params) == RZ_OK && pool.alloc(&l->loss_partial, 4LL * l->max_wg) == RZ_OK &&
                    pool.alloc(&l->grad, l->n_params) == RZ_OK && pool.alloc(&l->sq, l->n_blocks) == RZ_OK && pool.alloc(&l->err, 2) == RZ_OK;
    if (!ok) {
        delete l;
        return rz_fail(RZ_ERR_OOM, "hipMalloc failed (MuZero learner)");
    }
    if (hipMemset(l->err, 0, 2 * sizeof(int32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        delete l;
        return rz_fail(RZ_ERR_HIP, "initialisation of the MuZero learner failed");
    }
    *out = l;
    return RZ_OK;
}

int rz_mz_learner_destroy(rz_mz_learner *l) {
    if (l == nullptr) return RZ_OK;
    (void)hipSetDevice(l->device);
    (void)hipDeviceSynchronize();
    delete l;
    return RZ_OK;
}

int rz_mz_learner_n_params(rz_mz_learner *l, int64_t *n_params) {
    if (l == nullptr || n_params == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    *n_params = l->n_params;
    return RZ_OK;
}

int rz_mz_learner_bind(rz_mz_learner *l, void *const *d_params, float *d_exp_avg, float *d_exp_avg_sq) {
    RZ_ENTER(ml_ready, l);
    if (d_params == nullptr || d_exp_avg == nullptr || d_exp_avg_sq == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    for (int i = 0; i < RZ_MZL_TENSORS; ++i) {
        if (d_params[i] == nullptr) return rz_fail(RZ_ERR_ARG, "parameter %d is NULL", i);
        if (((uintptr_t)d_params[i] & 15) != 0) return rz_fail(RZ_ERR_ARG, "parameter %d is not 16-byte aligned", i);
    }
    for (int i = 0; i < RZ_MZL_TENSORS; ++i) l->table.p[i] = (float *)d_params[i];
    l->exp_avg = d_exp_avg, l->exp_avg_sq = d_exp_avg_sq;
    l->bound = true;
    return RZ_OK;
}

int rz_mz_learner_grads(rz_mz_learner *l, const float *d_obs, const int64_t *d_actions, const float *d_tv, const float *d_tr, const float *d_tp,
                        const float *d_mask, const float *d_weights, int64_t n, float *d_flat_grad, float *d_out4, void *stream) {
    RZ_ENTER(ml_ready, l);
    return ml_grads(l, d_obs, d_actions, d_tv, d_tr, d_tp, d_mask, d_weights, n, d_flat_grad, d_out4, (hipStream_t)stream);
}

int rz_mz_learner_step(rz_mz_learner *l, const float *d_obs, const int64_t *d_actions, const float *d_tv, const float *d_tr, const float *d_tp,
                       const float *d_mask, const float *d_weights, int64_t n, int64_t step_count, float *d_out4, void *stream) {
    RZ_ENTER(ml_ready, l);
    if (step_count < 1) return rz_fail(RZ_ERR_ARG, "step_count < 1");
    hipStream_t s = (hipStream_t)stream;
    RZ_TRY(ml_grads(l, d_obs, d_actions, d_tv, d_tr, d_tp, d_mask, d_weights, n, l->grad, d_out4, s));
    // torch/optim/adam.py, _single_tensor_adam: Python doubles of the step count, cast where torch casts them
    const rz_mz_learner_config &c = l->cfg;
    const double bc1 = 1.0 - std::pow(c.beta1, (double)step_count), bc2 = 1.0 - std::pow(c.beta2, (double)step_count);
    AdamStep<float> h;
    h.step_size = (float)(c.lr / bc1);
    h.bc2_sqrt = (float)std::sqrt(bc2);
    h.w1 = (float)(1.0 - c.beta1);
    h.beta2 = (float)c.beta2, h.w2 = (float)(1.0 - c.beta2);
    h.eps = (float)c.eps, h.weight_decay = (float)c.weight_decay;
    hipLaunchKernelGGL(k_mzl_adam, dim3((unsigned)l->n_blocks), dim3(kThreads), 0, s, l->table, (const float *)l->grad, (const float *)l->sq, l->n_blocks,
                       l->n_params, (float)c.max_norm, h, l->exp_avg, l->exp_avg_sq, l->err);
    return rz_launched("k_mzl_adam");
}

int rz_mz_learner_poll_errors(rz_mz_learner *l, int32_t *flags, int32_t *skipped, void *stream) {
    RZ_ENTER(ml_ready, l);
    if (flags == nullptr || skipped == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    int32_t both[2] = {0, 0};
    if (hipMemcpyAsync(both, l->err, sizeof(both), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemsetAsync(l->err, 0, sizeof(both), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "reading the MuZero learner's flags failed");
    *flags = both[0], *skipped = both[1];
    return RZ_OK;
}

}  // extern "C"
