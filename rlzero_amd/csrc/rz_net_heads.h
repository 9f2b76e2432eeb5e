// rz_net_heads.h -- the first FC layers of both heads on the f16 matrix pipe, fed by the f16 feature pieces the split-f16 trunks
// write: k_heads_split, k_heads_rows (rows of the deferred store) and k_heads_part (K quarters left to the consumer); and
// k_heads_finish (log_softmax, fc2 + tanh), which ends every FC route: these and the f32 one, k_heads_gemm of rz_net_f32.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "rz_net_dev.h"
#include "rz_net_split.h"

namespace {

// k_heads_split: the same two FC layers on the f16 matrix pipe, operands as hi + lo f16 pairs (three
// v_mfma_f32_32x32x16_f16 per product, f32 accumulation -- the arithmetic of k_trunk_split, which also writes the
// features as f16 pieces in A-fragment order; weights packed by pack_split_fc).  M = boards, N = outputs, so a
// lane's accumulator registers are boards of ONE output column and the stores of a tile row are 128 contiguous
// bytes.  A workgroup = TM 32-board tiles x TN policy N-tiles (group blockIdx.y) or x one of the two value N-tiles;
// its 4 waves split K into quarters (policy: 4S/16 steps, value: 2S/16) and every wave carries the whole block, so
// a fragment it loads (1 KB, one 16-byte load per lane, fully coalesced) feeds 3*TN or 3*TM MFMAs; DEPTH K-steps
// are in flight per wave.  The four partial blocks are summed through LDS in wave order.  The K quarters and the
// order of the sums do not depend on the shape, so every instantiation gives the same bits:
//   <2, 4, 3, true>   64 boards x half of the policy outputs AND one value tile per workgroup (policy first, then
//                     the value tile in the same LDS): 22 workgroups for 672 boards -- for the 32 CUs a capped
//                     trunk leaves free; the loads stay below the ~64 B/clk of a CU's vector memory path
//   <1, 2, 5, false>  32 boards x 2 policy tiles, the value tiles in workgroups of their own: 96 small workgroups
//                     for 512 boards, deep prefetch -- for the whole chip (the kernel is load-latency bound)
template <int TM, int TN>
struct FsFrags {
    sp::f16x8 a[TM][2], b[TN][2];
};

// Fragments of K-step `step` (A: TM feature tiles, steps_a K-steps apart; B: TN weight tiles at fb[n]).  Every load
// is unconditional -- a load under a branch makes hipcc wait for ALL outstanding loads (vmcnt(0)) before each use,
// which serialises the ring: a step past the end of the wave's K range re-reads the last feature step against the
// all-zero weight fragment `zero` (pack_split_fc appends one), and so does an N-tile past the last output tile.
// ROWS (k_heads_rows): the lane's board of A-tile m is a row of its own somewhere in the store -- far[m] points at that board's
// fragment of K-step 0 (its tile, its place lane_a in the fragment); the step is added as for a whole tile.
template <int TM, int TN, bool ROWS = false>
__device__ __forceinline__ void fs_load(FsFrags<TM, TN> &f, const f32x4 *__restrict__ fa, const f32x4 *const (&fb)[TN],
                                        const f32x4 *__restrict__ zero, int steps_a, int a_step0, int step, int k1, int lane,
                                        const f32x4 *const *far = nullptr) {
    const bool live = step < k1;
    const int sa = a_step0 + (live ? step : k1 - 1);
    const int lane_a = ((lane & 31) << 1) | (lane >> 5);  // features: [board % 32][k / 8 % 2] x 8 f16 (k_trunk_split)
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if constexpr (ROWS) f.a[m][p] = __builtin_bit_cast(sp::f16x8, far[m][((size_t)sa * 2 + p) * 64]);
            else f.a[m][p] = __builtin_bit_cast(sp::f16x8, fa[(((size_t)m * steps_a + sa) * 2 + p) * 64 + lane_a]);
        }
#pragma unroll
    for (int n = 0; n < TN; ++n) {
        // (a tile that does not exist has fb[n] == zero: every step of it reads the one zero fragment)
        const f32x4 *src = live && fb[n] != zero ? fb[n] + (size_t)step * 128 : zero;
#pragma unroll
        for (int p = 0; p < 2; ++p) f.b[n][p] = __builtin_bit_cast(sp::f16x8, src[p * 64 + lane]);
    }
}

// acc[m][n] += sum over K-steps [k0, k1) of A-tile m (features) x B-tile n (weights, fb[n] -> its step 0, or the zero
// fragment for a tile that does not exist)
template <int TM, int TN, int DEPTH, bool ROWS = false>
__device__ __forceinline__ void fs_gemm(sp::f32x16 (&acc)[TM][TN], const f32x4 *__restrict__ fa, const f32x4 *const (&fb)[TN],
                                        const f32x4 *__restrict__ zero, int steps_a, int a_step0, int k0, int k1, int lane,
                                        const f32x4 *const *far = nullptr) {
    if (k0 >= k1) return;
    FsFrags<TM, TN> ring[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) fs_load<TM, TN, ROWS>(ring[d], fa, fb, zero, steps_a, a_step0, k0 + d, k1, lane, far);
    __builtin_amdgcn_sched_barrier(0);
    for (int k = k0; k < k1; k += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
#pragma unroll
            for (int combo = 0; combo < 3; ++combo)
#pragma unroll
                for (int m = 0; m < TM; ++m)
#pragma unroll
                    for (int n = 0; n < TN; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ring[d].a[m][combo == 2], ring[d].b[n][combo == 1],
                                                                          acc[m][n], 0, 0, 0);
            fs_load<TM, TN, ROWS>(ring[d], fa, fb, zero, steps_a, a_step0, k + d + DEPTH, k1, lane, far);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// PAIRED (the GEMM over the deferred store: policy outputs only, hundreds of MB of features read once per move): a 1-D grid in
// which the workgroups of the SAME board tiles and different output groups are 8 apart -- workgroups go to the 8 XCDs round robin,
// so the two share an L2 and run together: the second one's feature reads hit there instead of HBM (a (tiles, groups) grid
// dispatches them thousands of workgroups apart: the store came from HBM twice, profiles/r04/pmc_traffic.json).
template <int TM, int TN, int DEPTH, bool VAL_FUSED, bool PAIRED = false>
__global__ __launch_bounds__(256) void k_heads_split(NetDev nd, const f32x4 *__restrict__ feat16,
                                                     float *__restrict__ raw, float *__restrict__ hid, int n_boards) {
    __shared__ sp::f32x16 part[4][TM * TN][64];  // [K quarter][tile][lane]
    const int n_act_tiles = nd.Npad / 32, n_groups = (n_act_tiles + TN - 1) / TN;
    int block_x = blockIdx.x, block_y = blockIdx.y;
    if constexpr (PAIRED) {
        static_assert(!VAL_FUSED, "policy outputs only");
        if (n_groups == 2) {   // (at most 256 outputs = 8 tiles = 2 groups of TN = 4)
            block_y = (block_x >> 3) & 1;
            block_x = ((block_x >> 4) << 3) | (block_x & 7);
        } else {
            block_y = 0;
        }
        if (block_x * TM * 32 >= n_boards) return;   // (the grid is rounded up to whole groups of 16; uniform, before any barrier)
    }
    __builtin_amdgcn_s_setprio(3);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mt0 = block_x * TM;
    const int steps_all = nd.groups_act + nd.groups_val;
    const f32x4 *fa = feat16 + (size_t)mt0 * steps_all * 128;  // 128 f32x4 = one K-step (hi | lo) of one tile
    const f32x4 *zero = nd.fs_act + (size_t)n_act_tiles * nd.groups_act * 128;  // one all-zero K-step behind the weights
    const int col = lane & 31, h = lane >> 5;
    const int group = block_y;                                       // policy outputs 32 * TN * group ..
    const int vtile = VAL_FUSED ? block_y : block_y - n_groups;  // value hidden units 32 * vtile ..
    if (group < n_groups) {
        const f32x4 *fb[TN];
#pragma unroll
        for (int n = 0; n < TN; ++n)
            fb[n] = TN * group + n < n_act_tiles ? nd.fs_act + (size_t)(TN * group + n) * nd.groups_act * 128 : zero;
        sp::f32x16 acc[TM][TN];
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int n = 0; n < TN; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;
        const int K = nd.groups_act, k0 = wave * K / 4, k1 = (wave + 1) * K / 4;
        fs_gemm<TM, TN, DEPTH>(acc, fa, fb, zero, steps_all, 0, k0, k1, lane);
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int n = 0; n < TN; ++n) part[wave][m * TN + n][lane] = acc[m][n];
        __syncthreads();
        const float scale = nd.s_inv[3];
        // wave w finishes tiles w, w + 4, ...: D column = output (lane & 31), rows = boards 8g + 4h + j
#pragma unroll
        for (int t = wave; t < TM * TN; t += 4) {
            const int m = t / TN, n = t % TN;
            if (TN * group + n >= n_act_tiles) continue;
            sp::f32x16 v = part[0][t][lane];
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                const sp::f32x16 pq = part[q][t][lane];
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] += pq[r];
            }
            const int c = 32 * (TN * group + n) + col;
            const float bias = nd.fc_act_b[c];
            // raw / hid have rows for whole 64-board tiles (rz_net_reserve): the stores need no bounds test -- under a
            // branch each one would wait for the previous store to be acknowledged (vmcnt(0) per basic block)
            float *dst = raw + (size_t)(32 * (mt0 + m) + 4 * h) * nd.Npad + c;
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[(size_t)(8 * (r >> 2) + (r & 3)) * nd.Npad] = fmaf(v[r], scale, bias);
        }
        if (VAL_FUSED) __syncthreads();
    }
    if (vtile >= 0 && vtile < 2) {
        const f32x4 *fb[1] = {nd.fs_val + (size_t)vtile * nd.groups_val * 128};
        sp::f32x16 acc[TM][1];
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][0][r] = 0.0f;
        const int K = nd.groups_val, k0 = wave * K / 4, k1 = (wave + 1) * K / 4;
        fs_gemm<TM, 1, DEPTH>(acc, fa, fb, zero, steps_all, nd.groups_act, k0, k1, lane);
#pragma unroll
        for (int m = 0; m < TM; ++m) part[wave][m][lane] = acc[m][0];
        __syncthreads();
        if (wave < TM) {
            const int m = wave;
            sp::f32x16 v = part[0][m][lane];
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                const sp::f32x16 pq = part[q][m][lane];
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] += pq[r];
            }
            const float scale = nd.s_inv[4];
            const int c = 32 * vtile + col;
            const float bias = nd.fc_val1_b[c];
            float *dst = hid + (size_t)(32 * (mt0 + m) + 4 * h) * 64 + c;
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[(8 * (r >> 2) + (r & 3)) * 64] = fmaxf(fmaf(v[r], scale, bias), 0.0f);
        }
    }
}

// k_heads_rows: k_heads_split<TM, TN, DEPTH, false, PAIRED>'s policy GEMM over a LIST of rows of the deferred store (the kept flush:
// rz_deferred_keep) -- rows[i] = slot * n_games + game is board game % 32 of store tile slot * store_tiles + game / 32, and lane l of
// A-tile m of row block b gathers row rows[32 * (TM * b + m) + (l & 31)]: a per-lane base under fs_load's index.  The K quarters per
// wave, the MFMA order, the LDS sum in wave order and fmaf(sum, scale, bias) are k_heads_split's and MFMA rows do not mix: the logits
// of a row are the bits of the GEMM over the whole store.  Output row i = listed row i.  The count is the device's (the launch sits
// in a captured move), so the grid is FIXED: its workgroups stride over the row blocks below the count -- the two output groups of a
// block 8 apart, one XCD (PAIRED) -- and meet at a barrier before `part` is written again.  Every load is unconditional (fs_load): a
// row past the count reads the first listed row again, and what it computes lands in rows nobody reads (the logits buffer has rows
// for whole blocks: the list's capacity is a multiple of 32 * TM).
template <int TM, int TN, int DEPTH>
__global__ __launch_bounds__(256) void k_heads_rows(NetDev nd, const f32x4 *__restrict__ store16, float *__restrict__ raw,
                                                    const int32_t *__restrict__ rows, const int32_t *__restrict__ count, int n_games,
                                                    int store_tiles) {
    __shared__ sp::f32x16 part[4][TM * TN][64];  // [K quarter][tile][lane]
    const int n_act_tiles = nd.Npad / 32, n_groups = (n_act_tiles + TN - 1) / TN;
    int block0 = blockIdx.x, group = 0, stride = gridDim.x;
    if (n_groups == 2) {   // (the host's grid is a multiple of 16)
        group = (block0 >> 3) & 1;
        block0 = ((block0 >> 4) << 3) | (block0 & 7);
        stride >>= 1;
    }
    const int n = count[0];
    const int n_blocks = (n + 32 * TM - 1) / (32 * TM);
    __builtin_amdgcn_s_setprio(3);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = nd.groups_act, k0 = wave * K / 4, k1 = (wave + 1) * K / 4;
    const f32x4 *zero = nd.fs_act + (size_t)n_act_tiles * K * 128;  // one all-zero K-step behind the weights
    const int col = lane & 31, h = lane >> 5;
    const f32x4 *fb[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) fb[t] = TN * group + t < n_act_tiles ? nd.fs_act + (size_t)(TN * group + t) * K * 128 : zero;
    const float scale = nd.s_inv[3];
    for (int blk = block0; blk < n_blocks; blk += stride) {   // (uniform: every wave of the workgroup meets the barriers)
        const f32x4 *far[TM];
#pragma unroll
        for (int m = 0; m < TM; ++m) {
            const int i = 32 * (TM * blk + m) + col;
            const int rec = rows[i < n ? i : 0];
            const int slot = rec / n_games, g = rec - slot * n_games;
            far[m] = store16 + (size_t)(slot * store_tiles + (g >> 5)) * K * 128 + (((g & 31) << 1) | h);
        }
        sp::f32x16 acc[TM][TN];
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int t = 0; t < TN; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.0f;
        fs_gemm<TM, TN, DEPTH, true>(acc, nullptr, fb, zero, K, 0, k0, k1, lane, far);
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int t = 0; t < TN; ++t) part[wave][m * TN + t][lane] = acc[m][t];
        __syncthreads();
        // wave w finishes tiles w, w + 4, ...: D column = output (lane & 31), rows = boards 8g + 4h + j
#pragma unroll
        for (int t = wave; t < TM * TN; t += 4) {
            const int m = t / TN, nt = t % TN;
            if (TN * group + nt >= n_act_tiles) continue;
            sp::f32x16 v = part[0][t][lane];
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                const sp::f32x16 pq = part[q][t][lane];
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] += pq[r];
            }
            const int c = 32 * (TN * group + nt) + col;
            const float bias = nd.fc_act_b[c];
            float *dst = raw + (size_t)(32 * (TM * blk + m) + 4 * h) * nd.Npad + c;
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[(size_t)(8 * (r >> 2) + (r & 3)) * nd.Npad] = fmaf(v[r], scale, bias);
        }
        __syncthreads();   // `part` is written again in the next round
    }
}

// k_heads_part: the arithmetic of k_heads_split with the reduction left to the consumer.  One single-wave workgroup
// per (32-board tile, 32-output tile, K quarter): no LDS, no barrier, ~170 registers -- a wave fits on a SIMD beside a
// wave of a resident k_trunk_split workgroup (344 registers of 512, 151 KB of LDS), so with two lanes of games this
// GEMM runs UNDER the other lane's trunk on all CUs instead of waiting for it (or for CUs reserved for it).  Part q of
// tile (m, n) goes to raw + q * raw_stride (policy) / hid + q * hid_stride (value) un-scaled; the consumer adds the four
// parts in the order k_heads_split does, ((p0 + p1) + p2) + p3, then fmaf(sum, scale, bias): the same bits.
// blockIdx = (board tile, output tile: policy tiles then the two value tiles, K quarter).
template <int DEPTH>
__global__ __launch_bounds__(64) void k_heads_part(NetDev nd, const f32x4 *__restrict__ feat16, float *__restrict__ raw,
                                                   float *__restrict__ hid, long long raw_stride, long long hid_stride) {
    __builtin_amdgcn_s_setprio(3);
    const int lane = threadIdx.x;
    const int mt = blockIdx.x, q = blockIdx.z;
    const int steps_all = nd.groups_act + nd.groups_val;
    const int n_act_tiles = nd.Npad / 32;
    const f32x4 *fa = feat16 + (size_t)mt * steps_all * 128;
    const f32x4 *zero = nd.fs_act + (size_t)n_act_tiles * nd.groups_act * 128;
    const int col = lane & 31, h = lane >> 5;
    const int tile = blockIdx.y;
    const bool is_act = tile < n_act_tiles;
    const int vtile = tile - n_act_tiles;
    const f32x4 *fb[1] = {is_act ? nd.fs_act + (size_t)tile * nd.groups_act * 128 : nd.fs_val + (size_t)vtile * nd.groups_val * 128};
    sp::f32x16 acc[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.0f;
    const int K = is_act ? nd.groups_act : nd.groups_val, k0 = q * K / 4, k1 = (q + 1) * K / 4;
    fs_gemm<1, 1, DEPTH>(acc, fa, fb, zero, steps_all, is_act ? 0 : nd.groups_act, k0, k1, lane);
    // rows for whole 64-board tiles exist in every part (rz_net_reserve): unconditional stores
    float *dst = is_act ? raw + (size_t)q * raw_stride + (size_t)(32 * mt + 4 * h) * nd.Npad + 32 * tile + col
                        : hid + (size_t)q * hid_stride + (size_t)(32 * mt + 4 * h) * 64 + 32 * vtile + col;
    const size_t ld = is_act ? (size_t)nd.Npad : (size_t)64;
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[(size_t)(8 * (r >> 2) + (r & 3)) * ld] = acc[0][0][r];
}

__global__ __launch_bounds__(64) void k_heads_finish(NetDev nd, const float *__restrict__ raw,
                                                     const float *__restrict__ hid, float *__restrict__ logp,
                                                     float *__restrict__ value, int n_boards, int n_parts,
                                                     long long raw_stride, long long hid_stride) {
    __builtin_amdgcn_s_setprio(3);
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= n_boards) return;
    const int S = nd.A;  // number of policy outputs
    const float *r = raw + (size_t)b * nd.Npad;
    const float act_scale = nd.s_inv[3], val_scale = nd.s_inv[4];
    float v[4];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = lane + 64 * i;
        v[i] = -INFINITY;
        if (j < S) {
            if (n_parts == 4)  // k_heads_part left the four K-quarter sums: finish them as k_heads_split does
                v[i] = fmaf(((r[j] + r[j + raw_stride]) + r[j + 2 * raw_stride]) + r[j + 3 * raw_stride], act_scale, nd.fc_act_b[j]);
            else
                v[i] = r[j];
        }
        mx = fmaxf(mx, v[i]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) sum += (lane + 64 * i < S) ? expf(v[i] - mx) : 0.0f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    const float lse = mx + logf(sum);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = lane + 64 * i;
        if (j < S) logp[(size_t)b * S + j] = v[i] - lse;
    }
    const float *hp = hid + (size_t)b * 64 + lane;
    float hv = hp[0];
    if (n_parts == 4)
        hv = fmaxf(fmaf(((hp[0] + hp[hid_stride]) + hp[2 * hid_stride]) + hp[3 * hid_stride], val_scale, nd.fc_val1_b[lane]), 0.0f);
    float h = hv * nd.fc_val2_w[lane];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) h += __shfl_xor(h, off);
    if (lane == 0) value[b] = tanhf(h + nd.fc_val2_b[0]);
}

}  // namespace
