// rz_mz_replay_prio.h -- prioritized replay of rz_mz_replay.hip: MzrPrio (the priority tables), the marks of written slots
// (k_mzr_mark, k_mzr_mark_where), the prefix sums (k_mzr_prio inside an episode, k_mzr_scan over the episodes held) and the draw in
// proportion to them (k_mzr_draw_prio).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rz_mz_replay_dev.h"
#include "rz_mz_target.h"

namespace {

// ---- Prioritized replay (ABI 37; the arithmetic and the draws: rz_mz_target.h).  Step t of a held episode weighs
// w = priority_weight(|root value - n-step return|), an integer; cum[slot][t] is the inclusive prefix of w inside the episode,
// mass[slot] its last entry, ecum[j] the inclusive prefix of the masses over the episodes held, oldest first, and *total the sum
// of everything.  Integer sums: the scans below give the bits of a loop in any order.  dirty[slot] != 0: the slot was written
// (k_mzr_add / k_mzr_ingest / k_mzr_update) since its prefix was formed.
constexpr int kScanThreads = 1024, kScanWaves = kScanThreads / 64;

struct MzrPrio {
    uint64_t *cum;     // [E][T]
    uint64_t *mass;    // [E] by slot
    uint64_t *ecum;    // [E] by age: 0 = the oldest held
    uint64_t *total;   // [1]
    int32_t *dirty;    // [E] by slot
};

// the inclusive scan of v over the 64 lanes of a wave
__device__ __forceinline__ uint64_t mzr_wave_scan(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t below = (uint64_t)__shfl_up((unsigned long long)v, (unsigned)d, 64);
        if (lane >= d) v += below;
    }
    return v;
}

// the slots first .. first + n - 1 (modulo E) were written
__global__ __launch_bounds__(kThreads) void k_mzr_mark(MzrPrio P, int E, long long first, long long n) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || i >= E) return;
    P.dirty[(int)((first + i) % E)] = 1;
}

// the slots k_mzr_update wrote to: its own checks of `where`, entry by entry, and nothing but the mark of slot where[i].slot
__global__ __launch_bounds__(kThreads) void k_mzr_mark_where(MzrDev R, MzrPrio P, const int32_t *__restrict__ where, long long n) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int slot = where[2 * i], pos = where[2 * i + 1];
    if (slot < 0 || slot >= R.E || pos < 0 || pos >= R.T) return;
    if (pos >= mzr_length(R, slot)) return;
    P.dirty[slot] = 1;
}

// A workgroup per held episode; one whose slot is clean returns at once.  Chunks of kThreads steps: each thread forms its step's
// weight, a wave scan, the waves' sums through LDS, and the chunk's sum carried into the next chunk (any T).
__global__ __launch_bounds__(kThreads) void k_mzr_prio(MzrDev R, MzrPrio P, long long oldest, long long count) {
    __shared__ uint64_t wave_sum[kWaves];
    if ((long long)blockIdx.x >= count) return;
    const int slot = mzr_slot(R, oldest + blockIdx.x);
    const int mark = P.dirty[slot];
    __syncthreads();   // (every thread has read the mark before thread 0 clears it)
    if (mark == 0) return;
    const int len = mzr_length(R, slot), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)slot * R.T;
    uint64_t carry = 0;
    for (int first = 0; first < len; first += kThreads) {
        const int t = first + (int)threadIdx.x;
        const uint64_t w = t < len ? rzmzt::priority_weight(rzmzt::priority_of(R.reward + base, R.root_value + base, len, t, R.td, R.disc)) : 0;
        uint64_t s = mzr_wave_scan(w, lane);
        if (lane == 63) wave_sum[wave] = s;
        __syncthreads();
        uint64_t chunk = 0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) {
            if (v < wave) s += wave_sum[v];
            chunk += wave_sum[v];
        }
        if (t < len) P.cum[base + t] = carry + s;
        carry += chunk;
        __syncthreads();   // (wave_sum is read before the next chunk writes it)
    }
    if (threadIdx.x == 0) {
        P.mass[slot] = carry;
        P.dirty[slot] = 0;
    }
}

// ONE workgroup: thread i sums the masses of the episodes i * per .. (i + 1) * per - 1 (by age), a scan of the partial sums over
// the workgroup, and the run walked again to write its prefixes.
__global__ __launch_bounds__(kScanThreads) void k_mzr_scan(MzrPrio P, int E, long long oldest, long long count) {
    __shared__ uint64_t wave_sum[kScanWaves];
    if (count > E) count = E;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long per = (count + kScanThreads - 1) / kScanThreads;
    const long long from = min((long long)threadIdx.x * per, count), to = min(from + per, count);
    uint64_t run = 0;
    for (long long j = from; j < to; ++j) run += P.mass[(int)((oldest + j) % E)];
    uint64_t s = mzr_wave_scan(run, lane);
    if (lane == 63) wave_sum[wave] = s;
    __syncthreads();
    uint64_t all = 0;
#pragma unroll
    for (int v = 0; v < kScanWaves; ++v) {
        if (v < wave) s += wave_sum[v];
        all += wave_sum[v];
    }
    uint64_t at = s - run;   // the sum of everything before this thread's run
    for (long long j = from; j < to; ++j) {
        at += P.mass[(int)((oldest + j) % E)];
        P.ecum[j] = at;
    }
    if (threadIdx.x == 0) *P.total = all;
}

// A thread per entry: ONE target g in 0 .. total - 1 -- from the entry's stream or from `targets` -- resolved by two searches,
// the episode in ecum, the position in the episode's cum; the draw row (episode by age, position, K fillers) in the layout of
// k_mzr_gather and the step's probability w / total.  A target out of range (or a table that does not hold it): the flag, a row
// of -1 that k_mzr_gather refuses as well, and probability 0.
__global__ __launch_bounds__(kThreads) void k_mzr_draw_prio(MzrDev R, MzrPrio P, unsigned long long seed, unsigned long long step,
                                                             const long long *__restrict__ targets, long long oldest, long long count, long long n,
                                                             long long *__restrict__ draws, double *__restrict__ prob) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int K = R.K;
    long long *dr = draws + i * (K + 2);
    const uint64_t total = *P.total;
    if (count > R.E) count = R.E;
    bool bad = total == 0 || count <= 0;
    uint64_t g = 0;
    if (targets != nullptr) {
        bad = bad || targets[i] < 0 || (uint64_t)targets[i] >= total;
        g = (uint64_t)targets[i];
    } else if (!bad) {
        g = rzmzt::prio_target(seed, step, (uint64_t)i, K, total);
    }
    long long ep = 0, pos = 0;
    uint64_t w = 0;
    if (!bad) {
        ep = rzmzt::upper_bound_u64(P.ecum, count, g);
        bad = ep >= count;
    }
    if (!bad) {
        const int slot = mzr_slot(R, oldest + ep);
        const int len = mzr_length(R, slot);
        const uint64_t *cum = P.cum + (long long)slot * R.T;
        pos = rzmzt::upper_bound_u64(cum, len, g - (ep > 0 ? P.ecum[ep - 1] : 0));
        bad = pos >= len;
        if (!bad) w = cum[pos] - (pos > 0 ? cum[pos - 1] : 0);
    }
    if (bad) {
        atomicOr(R.err, kFlagBadIndex);
        for (int j = 0; j < K + 2; ++j) dr[j] = -1;
        prob[i] = 0.0;
        return;
    }
    dr[0] = ep, dr[1] = pos;
    for (int k = 0; k < K; ++k) dr[2 + k] = rzmzt::prio_filler(seed, step, (uint64_t)i, K, k, (uint64_t)R.A);
    prob[i] = (double)w / (double)total;
}

}  // namespace
