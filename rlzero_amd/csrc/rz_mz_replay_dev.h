// rz_mz_replay_dev.h -- no kernel: what every kernel of rz_mz_replay.hip takes -- MzrDev (the store's pointers and sizes, passed by
// value), MzrOut (a mini-batch's tensors), the launch shape, the flags and the entry table's width -- and the two reads every kernel
// makes before it touches an episode: mzr_slot (any slot number reduced modulo the capacity) and mzr_length (clamped to 0 .. T).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rlzero_hip.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kFlagBadIndex = RZ_MZ_REPLAY_BAD_INDEX, kFlagBadRows = RZ_MZ_REPLAY_BAD_ROWS;
constexpr int kEntryWords = 4;   // an entry of the table of k_mzr_add / k_mzr_ingest: length, first row, slot, flags (bit 0: final policy)

struct MzrDev {
    float *obs;           // [E][T][D]
    int32_t *action;      // [E][T]
    double *reward;       // [E][T]
    double *root_value;   // [E][T]
    float *policy;        // [E][T][A]
    int32_t *length;      // [E]
    const double *disc;   // [td + 1]: discount ** i, formed on the host
    int32_t *err;
    int E, T, D, A, K, td;
};

struct MzrOut {
    float *obs;           // [n][D]
    long long *actions;   // [n][K]
    float *tv, *tr;       // [n][K + 1]
    float *tp;            // [n][K + 1][A]
    float *mask;          // [n][K + 1]
};

__device__ __forceinline__ int mzr_slot(const MzrDev &R, long long s) { return (int)(((s % R.E) + R.E) % R.E); }
__device__ __forceinline__ int mzr_length(const MzrDev &R, int slot) { return min(max(R.length[slot], 0), R.T); }

}  // namespace
