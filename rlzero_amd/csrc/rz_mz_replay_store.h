// rz_mz_replay_store.h -- the way in of rz_mz_replay.hip: k_mzr_add (rows from a staged host block) and k_mzr_ingest (rows from a
// launch's device arena), one body (mzr_store).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rz_mz_replay_dev.h"
#include "rz_mz_target.h"

namespace {

// Entry e of the table: its rows of `rows` [n_rows][D + 4 + A] into its slot.  A workgroup per entry, a wave per step row with the
// lanes across the row (D + 4 + A <= 28 doubles: one coalesced read), each lane casting and storing its own column.
__device__ __forceinline__ void mzr_store(const MzrDev &R, const int32_t *__restrict__ table, const double *__restrict__ rows, long long n_rows) {
    const int e = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int len = min(max(table[kEntryWords * e], 0), R.T);
    const long long first = table[kEntryWords * e + 1];
    const int slot = mzr_slot(R, table[kEntryWords * e + 2]);
    const bool final_policy = (table[kEntryWords * e + 3] & 1) != 0;
    if (first < 0 || first + len > n_rows) {   // (checked on the host too: nothing outside the block is read)
        if (threadIdx.x == 0) atomicOr(R.err, kFlagBadRows);
        return;
    }
    const int D = R.D, A = R.A, W = D + 4 + A;
    for (int t = wave; t < len; t += kWaves) {
        const double *row = rows + (first + t) * W;
        const long long at = (long long)slot * R.T + t;
        if (lane < D) {
            R.obs[at * D + lane] = (float)row[lane];
        } else if (lane == D) {
            R.action[at] = (int32_t)row[lane];
        } else if (lane == D + 1) {
            R.reward[at] = row[lane];
        } else if (lane < D + 2 + A) {
            R.policy[at * A + (lane - D - 2)] = rzmzt::policy_of_row(row, D, A, lane - D - 2, final_policy);
        } else if (lane == D + 2 + A) {
            R.root_value[at] = row[lane];
        }
    }
    if (threadIdx.x == 0) R.length[slot] = len;
}

__global__ __launch_bounds__(kThreads) void k_mzr_add(MzrDev R, const int32_t *__restrict__ table, const double *__restrict__ rows, long long n_rows) {
    mzr_store(R, table, rows, n_rows);
}

// the same body, the rows read from the arena of a launch of rz_mz_play_cartpole (device memory: the records never leave the GPU)
__global__ __launch_bounds__(kThreads) void k_mzr_ingest(MzrDev R, const int32_t *__restrict__ table, const double *__restrict__ arena,
                                                          long long arena_rows) {
    mzr_store(R, table, arena, arena_rows);
}

}  // namespace
