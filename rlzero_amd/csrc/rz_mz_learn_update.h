// rz_mz_learn_update.h -- what follows the tiles' partial gradients in rz_mz_learn.hip: k_mzl_reduce (the flat gradient, the blocks'
// squares, the loss means) and k_mzl_adam (the clipped Adam step on torch's own storage).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rlzero_hip.h"
#include "rz_mz_learn.h"
#include "rz_mz_learn_grad.h"

namespace {

// element p = the partials in workgroup order; sq[block] = the sum of the block's squares; block 0: the four loss means
__global__ __launch_bounds__(kThreads) void k_mzl_reduce(const float *__restrict__ partial, const float *__restrict__ loss_partial, int n_wg, int n_params,
                                                         long long n, float *__restrict__ grad, float *__restrict__ sq, float *__restrict__ out4) {
    __shared__ float tree[kThreads];
    const int p = blockIdx.x * kThreads + threadIdx.x;
    float g = 0.0f;
    if (p < n_params) {
        for (int w = 0; w < n_wg; ++w) g += partial[(long long)w * n_params + p];
        grad[p] = g;
    }
    tree[threadIdx.x] = g * g;
    __syncthreads();
    for (int d = kThreads / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) tree[threadIdx.x] += tree[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) sq[blockIdx.x] = tree[0];
    if (blockIdx.x == 0 && threadIdx.x < 4) {
        float s = 0.0f, c = 0.0f;
        for (int w = 0; w < n_wg; ++w) kahan_add(&s, &c, loss_partial[4 * w + threadIdx.x]);
        out4[threadIdx.x] = s / (float)n;
    }
}

__global__ __launch_bounds__(kThreads) void k_mzl_adam(MzlTable Tb, const float *__restrict__ grad, const float *__restrict__ sq, int n_blocks, int n_params,
                                                       float max_norm, AdamStep<float> h, float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                                       int32_t *__restrict__ err) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_params) return;
    if (err[0] != 0) {   // a refused batch updates nothing, nor does any update behind it until the flag is polled: err[1] counts them
        if (p == 0) err[1] += 1;
        return;
    }
    float total = 0.0f;
    for (int b = 0; b < n_blocks; ++b) total += sq[b];
    const float coef = clip_coef(sqrtf(total), max_norm);
    int tn = 0;
#pragma unroll
    for (int i = 1; i < RZ_MZL_TENSORS; ++i) tn += p >= Tb.off[i];
    float *param = Tb.p[0];
#pragma unroll
    for (int i = 1; i < RZ_MZL_TENSORS; ++i)
        if (tn == i) param = Tb.p[i];
    int first = 0;
#pragma unroll
    for (int i = 1; i < RZ_MZL_TENSORS; ++i)
        if (tn == i) first = Tb.off[i];
    adam_elem(grad[p] * coef, h, param + (p - first), exp_avg + p, exp_avg_sq + p);
}

}  // namespace
