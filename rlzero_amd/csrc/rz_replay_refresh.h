// rz_replay_refresh.h -- the Reanalyse kernels of rz_replay.hip: k_replay_positions (stored records out, as roots of the search
// engine), k_replay_update_pi and k_replay_update_q (a fresh search's visit counts and root values back into the slots they came from).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rz_replay_dev.h"
#include "rz_replay_rules.h"

namespace {

// Reanalyse, the way out: position index -> ring slot (`where`, -1 for an index outside 0 .. count - 1) and the stored record as a
// root of the search engine.  A thread per (row, record word): word j of the record goes to rzrr::root_word of row i; thread 0 of a
// row also writes the slot, the side to move and the last move.  indices NULL: the draws of refresh `step` made here.  A bad index
// sets the flag and writes only where[i] = -1: nothing of the store is read for it and its root is left as it was.
__global__ __launch_bounds__(kMaxCells) void k_replay_positions(ReplayDev R, const long long *__restrict__ indices, unsigned long long seed,
                                                                 unsigned long long step, long long oldest, long long count, long long n,
                                                                 int32_t *__restrict__ where, unsigned long long *__restrict__ stones,
                                                                 int32_t *__restrict__ to_move, int32_t *__restrict__ last_move) {
    const long long tid = (long long)blockIdx.x * kMaxCells + threadIdx.x;
    const long long i = tid / kRecWords;
    const int j = (int)(tid % kRecWords);
    if (i >= n) return;
    const long long index = indices != nullptr ? indices[i] : rzrr::reanalyse_position(seed, step, (uint64_t)i, (uint64_t)count);
    const long long slot = rzrr::slot_of_position(index, oldest, count, R.capacity);
    if (slot < 0) {
        if (j == 0) {
            atomicOr(R.err, kFlagBadIndex);
            where[i] = -1;
        }
        return;
    }
    const int32_t meta = R.meta[slot];
    stones[i * kRecWords + rzrr::root_word(meta, j)] = R.stones[slot * kRecWords + j];
    if (j == 0) {
        where[i] = (int32_t)slot;
        to_move[i] = rzrr::root_to_move(meta);
        last_move[i] = rzrr::root_last_move(meta);
    }
}

// Reanalyse, the way back: pi[where[i]][a] = N[i][a] / sum N[i] (rzrr::pi_of_visits).  A workgroup per row, a thread per action
// (blockDim.x = A rounded up to whole waves: one wave for Connect4's A = cols <= 16, up to four for Gomoku).  The sum is an INTEGER reduction -- across the lanes of a wave, then across the waves
// through LDS -- so it is exact whatever the order.  where < 0 (a refused or a padding row), a slot outside the capacity or a sum of
// 0 writes nothing; stones and meta are never written.  Every branch before the barrier is uniform across the workgroup.
__global__ __launch_bounds__(kMaxCells) void k_replay_update_pi(ReplayDev R, const int32_t *__restrict__ where, const int32_t *__restrict__ visits) {
    __shared__ long long s_part[kMaxCells / 64];
    const long long i = blockIdx.x;
    const int a = threadIdx.x, A = R.A, lane = a & 63, wave = a >> 6;
    const long long slot = where[i];
    if (slot < 0 || slot >= R.capacity) return;
    const int32_t mine = a < A ? visits[i * A + a] : 0;
    long long part = rzrr::visit_count(mine);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
    if (lane == 0) s_part[wave] = part;
    __syncthreads();
    long long sum = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) sum += s_part[w];
    if (sum == 0 || a >= A) return;
    R.pi[slot * A + a] = rzrr::pi_of_visits(mine, sum);
}

// Reanalyse, the way back for the value target: q[where[i]] = float32(values[i][0]) -- values: the engine's rz_root_values,
// float64 [n][2], of which [0] is the root value for the player to move.  A thread per row.  where < 0 (a refused or a padding row), a
// slot outside the capacity or a NaN value (an unvisited root) writes nothing (rzrr::value_written); stones, meta and pi are never
// written.  Two rows that name one slot write the same bits: the search is deterministic.
__global__ __launch_bounds__(kMaxCells) void k_replay_update_q(float *__restrict__ q, long long capacity, const int32_t *__restrict__ where,
                                                                const double *__restrict__ values, long long n) {
    const long long i = (long long)blockIdx.x * kMaxCells + threadIdx.x;
    if (i >= n) return;
    const long long slot = where[i];
    const double v = values[2 * i];
    if (rzrr::value_written(slot, capacity, v)) q[slot] = (float)v;
}

}  // namespace
