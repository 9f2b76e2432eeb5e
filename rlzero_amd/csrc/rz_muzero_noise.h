// rz_muzero_noise.h -- what the whole moves of k_mz_search (rz_muzero_search.h) and the moves behind a search (rz_muzero_moves.h) share
// on the device: the gamma draws of the root's Dirichlet noise (mz_hash32, mz_gamma, mz_root_gammas) and the hand-over of a finished
// episode (mz_claim_episode).  The keys and every rule of a move are rz_mz_env.h's.  No kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rz_mz_env.h"

#pragma clang fp contract(off)

namespace {

// One Gamma(alpha, 1) sample for the root's Dirichlet noise (add_exploration_noise) from a counter-based stream:
// Marsaglia-Tsang (boosted by U^(1/alpha) below shape 1).  Noise, not parity: hardware transcendentals, 24-bit uniforms
// (the scheme of gamma03 in rz_tree.h with the shape as an argument).
__device__ __forceinline__ uint32_t mz_hash32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ float mz_gamma(float alpha, uint32_t key) {
    const float shape = alpha < 1.0f ? alpha + 1.0f : alpha;
    const float d = shape - 1.0f / 3.0f, c = 1.0f / sqrtf(9.0f * d);
    const float kLn2 = 0.69314718f, k2m24 = 1.0f / 16777216.0f;
    float g = d;
    for (int t = 0; t < 8; ++t) {
        const uint32_t h1 = mz_hash32(key + 3u * t), h2 = mz_hash32(key + 3u * t + 1u), h3 = mz_hash32(key + 3u * t + 2u);
        const float u1 = (float)((h1 >> 8) + 1u) * k2m24;   // (0, 1]
        const float u2 = (float)(h2 >> 8) * k2m24;           // [0, 1): a turn of the cosine
        const float u3 = (float)((h3 >> 8) + 1u) * k2m24;   // (0, 1]
        const float x = __builtin_amdgcn_sqrtf(-2.0f * kLn2 * __builtin_amdgcn_logf(u1)) * __builtin_amdgcn_cosf(u2);
        float v = 1.0f + c * x;
        if (v <= 0.0f) continue;
        v = v * v * v;
        if (kLn2 * __builtin_amdgcn_logf(u3) < 0.5f * x * x + d - d * v + d * kLn2 * __builtin_amdgcn_logf(v)) {
            g = d * v;
            break;
        }
    }
    if (alpha < 1.0f) {
        const float ub = (float)((mz_hash32(key + 0x5bd1e995u) >> 8) + 1u) * k2m24;
        g = g * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(ub) * (1.0f / alpha));  // ub^(1/alpha)
    }
    return fmaxf(g, 1e-30f);
}

// the gamma draws of a move's root noise under its key (rzmze::move_key, salt 0; 0 past the last action) -> their sum, in fp64 in
// action order
template <int MAXA>
__device__ __forceinline__ double mz_root_gammas(float alpha, uint64_t key, int A, float (&gam)[MAXA]) {
    double gsum = 0.0;
#pragma unroll
    for (int a = 0; a < MAXA; ++a) {
        gam[a] = a < A ? mz_gamma(alpha, rzmze::noise_key(key, a)) : 0.0f;
        gsum += (double)gam[a];
    }
    return gsum;
}

// the hand-over of an episode of `len` records that ended before step `end`: its run of arena rows (-1 and a count in counters[2]
// where they do not fit), its entry (environment, end step, length, first arena row) -> the first arena row.  GUARDED: counters that
// are not counts any more claim nothing
template <bool GUARDED>
__device__ __forceinline__ long long mz_claim_episode(long long *counters, long long arena_rows, long long *entries, long long max_entries, int g,
                                                      long long end, long long len) {
    long long off = (long long)atomicAdd(reinterpret_cast<unsigned long long *>(counters), (unsigned long long)len);
    if ((GUARDED && off < 0) || off + len > arena_rows) {
        off = -1;
        atomicAdd(reinterpret_cast<unsigned long long *>(counters + 2), 1ull);
    }
    const long long e = (long long)atomicAdd(reinterpret_cast<unsigned long long *>(counters + 1), 1ull);
    if ((!GUARDED || e >= 0) && e < max_entries) {
        entries[4 * e + 0] = g;
        entries[4 * e + 1] = end;
        entries[4 * e + 2] = len;
        entries[4 * e + 3] = off;
    }
    return off;
}

}  // namespace
