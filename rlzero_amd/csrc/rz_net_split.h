// rz_net_split.h -- the split-f16 tile trunk of rz_net.hip: namespace sp (hi + lo f16 operands on v_mfma_f32_32x32x16_f16; its
// types, LDS geometry and conversions also serve the row trunk, the delta kernels and the f16 FC GEMMs) and k_trunk_split.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <utility>

#include "rlzero_hip.h"
#include "rz_net_dev.h"
#include "rz_pack.h"
#include "rz_tree.h"

namespace {

// ------------------------------------------------------------------ split-operand direct convolution
// conv1 .. conv3 as DIRECT 3x3 convolutions on the f16 matrix pipe (v_mfma_f32_32x32x16_f16: 16x the rate of
// the f32-input MFMA, which runs at the vector rate and does not overlap with vector work at all -- DESIGN.md
// section 5), with every f32 operand carried as an unevaluated sum of two f16 values:
//     x * s = hi + lo,  hi = f16(x * s),  lo = f16(x * s - hi)           (s: a power of two, see below)
// and every product formed as hi*hi + hi*lo + lo*hi on three MFMAs that accumulate in f32.  hi + lo holds 22
// significant bits of x and the dropped lo*lo term is below 2^-22 of the product, so the result is within a
// few 1e-7 (relative) of the f32 kernels -- the level of their own accumulation rounding (measured in
// tests/test_gpu_parity.py; the tolerance of the path is 1e-4).  Scales keep the lo halves out of f16's
// subnormal range: the activations of a layer are stored times a power of two <= 16 that rz_net_load derives from a
// bound on that layer's activations (bias + positive weights x input bounds, observation planes in [0, 1]), so a
// network of ANY weight scale stays inside the f16 range on the 0 / 1 planes of the MCTS leaves -- no fallback is
// needed for trained weights (inputs beyond [0, 1] through rz_net_trunk / rz_net_forward can still overflow: that
// raises RZ_NET_FLAG_F16_RANGE); the weights of a layer are stored times the power of two that brings their
// largest magnitude into [2^13, 2^14); the accumulator is rescaled (exactly) in the epilogue.
//   * LDS: conv1's and conv2's outputs as [piece][18 rows][18 cols][channels + 8] f16, channels innermost, so
//     the B fragment of a lane (8 consecutive input channels of one position) is ONE ds_read_b128; position
//     strides of 80 / 144 bytes spread the 8 lanes of an LDS cycle over all 64 banks.  147.4 KB + 3.5 KB of
//     head weights and conv3 biases, staged once per persistent workgroup.
//   * MFMA tile: M = 32 output channels, N = 32 positions = two board rows x 16 columns, K = 16 input channels
//     of one tap.  Wave w owns board rows 4w .. 4w+3 (2 N-tiles) and ALL M-tiles of a layer (conv2: 2, conv3:
//     4), so one K-step is 6*TM MFMAs on 2*TM weight fragments (buffer loads from L2, packed on the host in
//     fragment order, two steps ahead) and 4 activation fragments (one step ahead); one load is pinned behind
//     each of the first MFMAs of the step.  The chip is at its power limit in these loops (DESIGN.md section
//     5): what counts is the amount of work, not where it is placed.
//   * conv1 (4 -> 32): the observation planes live in LDS as [piece][position][4 planes] f16, K-step = one kernel
//     row (4 columns x 4 planes, the 4th column meeting zero weights), its 6 weight fragments and biases stay in
//     registers across boards; conv3's output feeds the two 1x1 head convolutions from registers in f32.
namespace sp {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef const __attribute__((address_space(3))) f16x8 *lds_frag;

using rzp::kObsScale;   // (rz_pack.h: the host scales the weights by what the kernels scale the planes and activations by)
constexpr int kGridPos = 18 * 18;
// POS: positions of the halo grid (18 x 18 in general; the compact layout of small boards: see k_trunk_split's RW / RH)
template <int CIN, int POS = kGridPos> struct Geo {
    static constexpr int pos_bytes = (CIN + 8) * 2;          // 80 / 144
    static constexpr int piece_bytes = POS * pos_bytes;      // 25 920 / 46 656 on the 18 x 18 grid
    static constexpr int chunks = CIN / 16, steps = 9 * chunks;
};
constexpr int kC1Bytes = 2 * Geo<32>::piece_bytes, kC2Bytes = 2 * Geo<64>::piece_bytes;
// observation planes: [hi | lo][18 rows][20 cols][4 planes] f16 -- the 4 planes of a position are 8 contiguous bytes,
// so the 16 K-values of conv1's step "kernel row ky" (4 columns x 4 planes, the 4th column meeting zero weights)
// are two 16-byte runs
constexpr int kInCols = 20, kInPieceBytes = 18 * kInCols * 8, kInBytes = 2 * kInPieceBytes;
constexpr int kHeadFloats = 128 * 7 + 8;  // head weights [128][6] + conv3 biases [128] + head biases [6] (+ 2 pad)
constexpr int kLdsBytes = kInBytes + kC1Bytes + kC2Bytes + kHeadFloats * 4;
static_assert(kLdsBytes <= 160 * 1024, "LDS budget");
static_assert(kInBytes % 16 == 0, "piece alignment");

__device__ __forceinline__ f16x8 load_w(__amdgpu_buffer_rsrc_t rsrc, int lane_off, int uniform_off) {
    return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_off, uniform_off, 0));
}

// x (already scaled) -> hi, lo in 8 vector instructions per 4 values: two packed conversions for the hi pieces
// (v_cvt_pk_f16_f32, round to nearest even like the scalar conversion), the residuals z - hi as v_fma_mix_f32 with the f16
// operand widened inside the instruction (the same single rounding as convert + subtract; hipcc folds fma(x, -1, z) back
// into the two instructions, hence the asm), two packed conversions for lo.
__device__ __forceinline__ float resid_lo(float z, unsigned pair) {
    float r;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(pair), "v"(z));
    return r;
}
__device__ __forceinline__ float resid_hi(float z, unsigned pair) {
    float r;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(pair), "v"(z));
    return r;
}
__device__ __forceinline__ void split4(const float (&z)[4], f16x4 &hi, f16x4 &lo) {
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const f32x4v zv = {z[0], z[1], z[2], z[3]};
    hi = __builtin_convertvector(zv, f16x4);
    const u32x2 pairs = __builtin_bit_cast(u32x2, hi);
    const f32x4v r = {resid_lo(z[0], pairs[0]), resid_hi(z[1], pairs[0]), resid_lo(z[2], pairs[1]), resid_hi(z[3], pairs[1])};
    lo = __builtin_convertvector(r, f16x4);
}

// slot I of K-step S: MFMA I of the step plus (behind the first MFMAs) one load of a coming step
// (D = depth of the ring of weight fragments: a step's fragments are requested D - 1 steps ahead -- 2 where a step has
// 6 or more MFMAs to cover the L2 round trip, 4 for the small tiles of the channel-split variants)
constexpr int ring_depth(int tm, int tn) { return tm * tn >= 3 ? 3 : 5; }
// (and of the ring of activation fragments: read from LDS one step ahead)
constexpr int act_depth(int, int) { return 2; }   // (3 for the small tiles was tried: no gain, their steps are bound by the accumulator chain)
template <int CIN, int TM, int TN, int RPT, int RW, int S, int I>
__device__ __forceinline__ void slot(f32x16 (&acc)[TM][TN], f16x8 (&a)[ring_depth(TM, TN)][TM][2], f16x8 (&b)[act_depth(TM, TN)][TN][2], lds_frag q0,
                                     lds_frag q1, __amdgpu_buffer_rsrc_t w_rsrc, int w_base, int w_lane) {
    using G = Geo<CIN>;
    constexpr int D = ring_depth(TM, TN);
    constexpr int combo = I / (TM * TN), m = (I / TN) % TM, n = I % TN;
    constexpr int pa = combo == 2 ? 1 : 0, pb = combo == 1 ? 1 : 0;
    constexpr int DB = act_depth(TM, TN);
    if constexpr (S == 0 && combo == 0) {   // the first MFMA of a tile starts from the constant 0: no zeroing of 16 registers per tile
        const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[S % D][m][pa], b[S % DB][n][pb], zero, 0, 0, 0);
    } else {
        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[S % D][m][pa], b[S % DB][n][pb], acc[m][n], 0, 0, 0);
    }
    if constexpr (I < 2 * TN) {
        if constexpr (S + DB - 1 < G::steps) {
            constexpr int s1 = S + DB - 1, tap = s1 / G::chunks, c = s1 % G::chunks, nn = I / 2, piece = I % 2;
            constexpr int off = ((RPT * nn + tap / 3) * RW + tap % 3) * G::pos_bytes + c * 32;
            static_assert(off % 16 == 0 && off < 65536, "ds_read_b128 immediate");
            b[s1 % DB][nn][piece] = (piece ? q1 : q0)[off / 16];
        }
    } else if constexpr (I < 2 * TN + 2 * TM) {
        if constexpr (S + D - 1 < G::steps) {
            constexpr int s2 = S + D - 1, j = I - 2 * TN, mm = j / 2, piece = j % 2;
            a[s2 % D][mm][piece] = load_w(w_rsrc, w_lane, w_base + ((mm * G::steps + s2) * 2 + piece) * 1024);
            // one M-tile x one N-tile: three MFMAs per step but four fragments to fetch -- the last slot takes two
            if constexpr (TM == 1 && TN == 1 && I == 2)
                a[s2 % D][0][1] = load_w(w_rsrc, w_lane, w_base + (s2 * 2 + 1) * 1024);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

template <int CIN, int TM, int TN, int RPT, int RW, int S, int... Is>
__device__ __forceinline__ void step(std::integer_sequence<int, Is...>, f32x16 (&acc)[TM][TN], f16x8 (&a)[ring_depth(TM, TN)][TM][2],
                                     f16x8 (&b)[act_depth(TM, TN)][TN][2], lds_frag q0, lds_frag q1, __amdgpu_buffer_rsrc_t w_rsrc,
                                     int w_base, int w_lane) {
    (slot<CIN, TM, TN, RPT, RW, S, Is>(acc, a, b, q0, q1, w_rsrc, w_base, w_lane), ...);
}

template <int CIN, int TM, int TN, int RPT, int RW, int... Ss>
__device__ __forceinline__ void steps(std::integer_sequence<int, Ss...>, f32x16 (&acc)[TM][TN], f16x8 (&a)[ring_depth(TM, TN)][TM][2],
                                      f16x8 (&b)[act_depth(TM, TN)][TN][2], lds_frag q0, lds_frag q1, __amdgpu_buffer_rsrc_t w_rsrc,
                                      int w_base, int w_lane) {
    (step<CIN, TM, TN, RPT, RW, Ss>(std::make_integer_sequence<int, 3 * TM * TN>{}, acc, a, b, q0, q1, w_rsrc, w_base, w_lane), ...);
}

// The weight fragments of the first K-steps (M-tiles 0 .. TM-1): no dependence on LDS, so a layer's first
// fragments are requested while the previous layer is still being reduced.
template <int CIN, int TM, int TN>
__device__ __forceinline__ void preload_w(f16x8 (&a)[ring_depth(TM, TN)][TM][2], const void *wts, int lane) {
    using G = Geo<CIN>;
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(wts), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int s = 0; s < ring_depth(TM, TN) - 1; ++s)
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int p = 0; p < 2; ++p) a[s][m][p] = load_w(w_rsrc, lane * 16, ((m * G::steps + s) * 2 + p) * 1024);
}

// acc[m][n] = sum over taps and input channels for M-tiles 0 .. TM-1 (all output channels of the layer) and
// N-tiles nt0 .. nt0 + TN - 1 (`in` = piece 0 of the layer's input in LDS, `a` primed by preload_w).
// The lane's MFMA column is the position (row0 + ry, x) of the wave's first N-tile; a further tile of the wave (TN = 2
// only) lies two rows below (RPT rows in general: the 3 + 1 variant runs three 3-row tiles in one wave).
template <int CIN, int TM, int TN, int RPT = 2, int RW = kRowW, int POS = kGridPos>
__device__ __forceinline__ void conv(const char *in, const void *wts, int row0, int ry, int x, int lane,
                                     f16x8 (&a)[ring_depth(TM, TN)][TM][2], f32x16 (&acc)[TM][TN]) {
    using G = Geo<CIN, POS>;
    const int h = lane >> 5;
    // halo position (row0 + ry, x) = the top-left tap of output (row0 + ry, x)
    const int lane_byte = ((row0 + ry) * RW + x) * G::pos_bytes + h * 16;
    const lds_frag q0 = (lds_frag)(in + lane_byte), q1 = (lds_frag)(in + lane_byte + G::piece_bytes);
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(wts), 0, 0x7fffffff, 0x00020000);
    f16x8 b[act_depth(TM, TN)][TN][2];
#pragma unroll
    for (int s0 = 0; s0 < act_depth(TM, TN) - 1; ++s0) {   // the fragments of the first step(s): tap = s0 / chunks, chunk = s0 % chunks
        const int tap = s0 / G::chunks, c = s0 % G::chunks;
#pragma unroll
        for (int nn = 0; nn < TN; ++nn) {
            const int off = ((RPT * nn + tap / 3) * RW + tap % 3) * G::pos_bytes + c * 32;
            b[s0][nn][0] = q0[off / 16];
            b[s0][nn][1] = q1[off / 16];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    steps<CIN, TM, TN, RPT, RW>(std::make_integer_sequence<int, G::steps>{}, acc, a, b, q0, q1, w_rsrc, 0, lane * 16);
}

}  // namespace sp

// Wave w owns board rows 4w .. 4w+3 (N-tiles 2w, 2w+1) and ALL output channels of conv2 and of conv3, so the
// 1x1 head convolutions see every channel of a position in one wave (two lane halves, one shuffle) and the head
// features go from registers to memory: two barriers per board.  TN = N-tiles per wave: 2 (tiles of 2 rows x 16
// columns) in general; when four tiles of 32 / width rows x width columns cover the board (9x9: 3 x 9, 10x10: 3 x 10,
// 8x8: 4 x 8, Connect4: 4 x 7, 6x6: 5 x 6) a wave owns ONE such tile (TN = 1) and issues half the MFMAs or fewer; a
// wave whose rows lie below the board skips its MFMA loops.

// MS (with TN = 1): when the board needs only 2 (MS = 2) or 1 (MS = 4) of the four N-tiles, the waves that would idle
// take a share of the OUTPUT CHANNELS instead: wave = part * (4 / MS) + tile, part p computes M-tiles p * TM / MS .. of
// conv2 and conv3 for its tile (a 6x7 Connect4 board: 6 instead of 12 MFMAs per K-step and wave; a 3x3 board: 3).  The
// 1x1 head convolutions then sum over the channels of MS waves: partial sums meet in LDS (in the 16 padding bytes of
// conv1's positions, which nothing else touches), part 0 adds them in part order and stores the features.
// the value of lane l ^ 32 (h = l >> 5): v_permlane32_swap, two vector instructions instead of a trip through the LDS crossbar
__device__ __forceinline__ float other_half(float x, int h) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(h ? r[0] : r[1]);
}

// FC_HERE (small boards, TN = 1; `raw` / `hid` given): the workgroup also runs the first FC layers of both heads on ITS OWN
// board, behind the feature stage -- the arithmetic of k_heads_split (the same MFMA on the same K quarters, one per wave, the
// quarters summed in wave order, fmaf(sum, scale, bias)): the same bits, one launch and one kernel boundary less in the chain
// trunk -> FC -> tree step of a small batch.  A board is row 0 of the MFMA's 32 (the other rows are zero: rows do not mix), its
// features never leave the CU (f16 pieces in LDS), the weights stream from L2.
// RW x RH: the halo grid of the activations in LDS.  18 x 18 (a board of up to 16 x 16) in general: 154 KB, one workgroup per CU.
// COMPACT grids for small boards (RW = width + 2, RH such that RW x RH >= 128 positions: the channel-split variants park their
// partial head sums in the padding of positions 0 .. 127) cut that to 60-70 KB -- TWO workgroups per CU: a board of 6 x 7 is a
// latency chain of small MFMA loops, and two such chains interleave on a CU where one leaves the pipes idle most of the time.
// Tile rows beyond the board still read positions past its ring (MFMA columns that are stored nowhere): inside the grid or
// in the bytes behind it, always inside the workgroup's LDS.  (FC_HERE needs the big grid's spare rows: 18 x 18 only.)
// PUCT (with RES, TN = 1, the 18 x 18 grid; rz_net_search_resident_puct): the resident search under RZ_SCORE_PUCT, whose selection
// reads the priors of the node it stands on -- nothing of a simulation can wait for a flush.  The workgroup runs FC_HERE on its
// game's leaf (row blockIdx.x of `raw` / `hid`: final logits and the value head's hidden row, the arithmetic of k_heads_split) and
// wave 0 finishes the heads inside the tree code (expand_backup_body<RAW>: k_tree_step_raw's body, which holds NO barrier -- the other
// waves go straight to the barrier behind it): the trees, priors and values of trunk -> FC GEMM -> k_tree_step_raw, in one launch.
// Nothing goes to the deferred store, no value row or K-quarter sums in LDS, `pend` is not read.  One game per CU.
template <int TN, int MS = 1, bool RES = false, int RW = kRowW, int RH = 18, bool PUCT = false>
__global__ __launch_bounds__(256, (RW == kRowW ? 1 : 2)) void k_trunk_split(NetDev nd, const float *__restrict__ obs, LeafBits leaves,
                                                     float *__restrict__ feat, _Float16 *__restrict__ feat16,
                                                     int n_boards, unsigned *__restrict__ flags,
                                                     float *__restrict__ raw = nullptr, float *__restrict__ hid = nullptr,
                                                     DeferredOut later = DeferredOut{nullptr, 0, nullptr, 0, nullptr},
                                                     ResArgs<RES> res = ResArgs<RES>{}) {
#ifdef RZ_NET_PROFILE
    const long long prof_k0 = __builtin_readcyclecounter();
    long long prof_acc[24] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, prof_t = prof_k0;
#endif
    constexpr int kThreads = 256;
    static_assert(!PUCT || (RES && TN == 1 && RW == kRowW && RH == 18), "the resident PUCT search: RES, one N-tile per wave, the 18 x 18 grid (FC_HERE)");
    // the resident search's tree code (rz_tree.h: W): a board of one N-tile (MS = 4) or two (MS = 2) has at most 64 cells = one word
    // of a bitboard, every board of this kernel (four tiles of 32 positions) at most 128 = two
    constexpr int kResWords = (MS == 4 || MS == 2) ? 1 : 2;
    // RES (the resident search, see ResArgs): the value head's input row (boards of up to 10 rows and columns: 2 S <= 256 with
    // the padding), the K-quarter sums of its first layer, the next leaf
    __shared__ float res_vrow[RES && !PUCT ? 256 : 1];
    __shared__ float res_part[RES && !PUCT ? rzt::kDefWaves : 1][RES && !PUCT ? rzt::kWave : 1];
    __shared__ __attribute__((aligned(16))) uint64_t res_leaf[RES ? 2 * RZ_BOARD_WORDS + 1 : 1];
    int res_slot0 = 0;
    int res_n = 0;   // (RES: the simulations of this workgroup's game)
    if constexpr (RES) {
        if ((int)blockIdx.x >= n_boards || res.E.active[blockIdx.x] == 0) return;   // (uniform: before any barrier)
        res_n = res_sims(res, blockIdx.x);
        if constexpr (!PUCT) {
            res_slot0 = res.E.pend[blockIdx.x];
            res_vrow[threadIdx.x] = 0.0f;
        }
    }
    constexpr int POS = RW * RH, IC = RW + 2;   // positions of the halo grid; columns of the observation planes' grid
    constexpr int kInPiece = RH * IC * 8, kInB = 2 * kInPiece, kC1B = 2 * sp::Geo<32, POS>::piece_bytes, kC2B = 2 * sp::Geo<64, POS>::piece_bytes;
    static_assert(kInB % 16 == 0 && POS >= 128, "the grid: 16-byte pieces, 128 positions for the channel-split variants' partial sums");
    __shared__ __attribute__((aligned(16))) char lds_raw[kInB + kC1B + kC2B + sp::kHeadFloats * 4];
    char *in0 = lds_raw;                      // observation planes, pieces hi | lo
    char *c1 = lds_raw + kInB;                // conv1 output, pieces hi | lo
    char *c2 = c1 + kC1B;                     // conv2 output, pieces hi | lo
    float *hw = reinterpret_cast<float *>(c2 + kC2B);  // head weights [128][6], then conv3 biases [128]
    const int tid0 = threadIdx.x;
    const int BH = nd.BH, BW = nd.BW, S = nd.S;
    float zmax = 0.0f;  // largest scaled value this thread stored as f16 pieces
    constexpr int kObsPer = (4 * RZ_MAX_BOARD_SIZE * RZ_MAX_BOARD_SIZE + kThreads - 1) / kThreads;
    float ob[kObsPer];
    auto load_obs = [&](int board, int tid) {
        const float *src = obs + (size_t)board * 4 * S;
#pragma unroll
        for (int k = 0; k < kObsPer; ++k) {
            const int i = tid + k * kThreads;
            ob[k] = i < 4 * S ? src[i] : 0.0f;
        }
    };
    const bool from_bits = leaves.stones != nullptr;
    int obs_off[kObsPer];
#pragma unroll
    for (int k = 0; k < kObsPer; ++k) obs_off[k] = -1;
    if (!from_bits) {  // (two integer divisions per element: ~1.5 k cycles of the prologue that the bitboard route does not need)
#pragma unroll
        for (int k = 0; k < kObsPer; ++k) {
            const int i = tid0 + k * kThreads;
            const int c = i / S, r = i - c * S, y = r / BW, x = r - y * BW;
            obs_off[k] = i < 4 * S ? ((y + 1) * IC + (x + 1)) * 8 + c * 2 : -1;
        }
    }
    // bit mode: thread t owns cell t (S <= 256 = threads); its 4 plane values as f16 (x 16: exact, the lo piece is 0)
    const int cell_y = tid0 / BW, cell_x = tid0 - cell_y * BW;
    const int cell_off = tid0 < S ? ((cell_y + 1) * IC + (cell_x + 1)) * 8 : -1;
    sp::f16x4 cell_planes = {(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
    auto load_bits = [&](int board, int tid) {
        const uint64_t *sb = leaves.stones + (size_t)board * 8;
        const int tm = leaves.to_move[board], lc = leaves.last[board];
        int nst = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) nst += __popcll(sb[q]);  // (uniform address: scalar loads)
        const int word = (tid >> 6) & 3, bit = tid & 63;
        const uint64_t w0 = sb[word], w1 = sb[4 + word];
        const bool s0 = (w0 >> bit) & 1ull, s1 = (w1 >> bit) & 1ull;
        const bool mine = tm == 0 ? s0 : s1, theirs = tm == 0 ? s1 : s0;
        const _Float16 one = (_Float16)sp::kObsScale, zero = (_Float16)0.0f;
        cell_planes[0] = mine ? one : zero;
        cell_planes[1] = theirs ? one : zero;
        cell_planes[2] = (nst > 0 && tid == lc) ? one : zero;
        cell_planes[3] = (nst & 1) ? zero : one;
    };
    auto store_obs = [&](int) {
        if (from_bits) {
            if (cell_off >= 0) {
                *reinterpret_cast<sp::f16x4 *>(in0 + cell_off) = cell_planes;
                *reinterpret_cast<sp::f16x4 *>(in0 + kInPiece + cell_off) =
                    sp::f16x4{(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
            }
            return;
        }
#pragma unroll
        for (int k = 0; k < kObsPer; ++k)
            if (obs_off[k] >= 0) {
                const float z = ob[k] * sp::kObsScale;
                const _Float16 hi = (_Float16)z;
                zmax = fmaxf(zmax, fabsf(z));
                *reinterpret_cast<_Float16 *>(in0 + obs_off[k]) = hi;
                *reinterpret_cast<_Float16 *>(in0 + kInPiece + obs_off[k]) = (_Float16)(z - (float)hi);
            }
    };
    // Prologue of a persistent workgroup.  Every global load it needs -- head weights and conv3 biases (3.5 KB, bound for
    // LDS), the rescaling factors and activation scales, conv1's weights and biases (registers), the first board -- is
    // ISSUED first, the parts of the LDS that no board writes are zeroed under their latency, and only then the values are stored: with one board
    // per workgroup (256 boards per launch) the prologue is not amortised, and two lanes alternate such launches.
    constexpr int kHwPer = (128 * 7 + kThreads - 1) / kThreads;
    float hw_reg[kHwPer];
#pragma unroll
    for (int k = 0; k < kHwPer; ++k) {
        const int i = tid0 + k * kThreads;
        hw_reg[k] = i < 768 ? nd.whp[i] : (i < 128 * 7 ? nd.b3[i - 768] : 0.0f);
    }
    // the 6 head biases too: a global load in the epilogue would sit between the feature stores, and its
    // s_waitcnt vmcnt(0) also waits for the stores before it -- six store round trips per board
    const float bh_reg = tid0 < 6 ? nd.bh[tid0] : 0.0f;
    // the rescaling factors and the activation scales of the layers (powers of two chosen by rz_net_load from
    // bounds on the activations) once per workgroup: a load placed behind a layer's MFMA loop is exposed in full
    const float k1 = nd.s_inv[2], k2 = nd.s_inv[0], k3 = nd.s_inv[1];
    const float act1 = nd.s_inv[5], act2 = nd.s_inv[6], act3 = nd.s_inv[7];
    // conv1's weights (3 kernel rows x hi / lo, 6 KB per workgroup) and biases stay in registers for all boards
    sp::f16x8 a1[3][2];
    f32x4 bias1[4];
    {
        const int lane0 = tid0 & 63;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int p_ = 0; p_ < 2; ++p_) a1[ky][p_] = __builtin_bit_cast(sp::f16x8, nd.s1[(ky * 2 + p_) * 64 + lane0]);
#pragma unroll
        for (int g = 0; g < 4; ++g) bias1[g] = *reinterpret_cast<const f32x4 *>(nd.b1 + 8 * g + 4 * (lane0 >> 5)) * act1;
    }
    const bool first = (int)blockIdx.x < n_boards;
    bool sel_first = false;   // RES: the first leaf is selected by this launch (below, behind the zeroing)
    if constexpr (RES) sel_first = res.select_first != 0;
    if (first && !sel_first) {
        if (from_bits) load_bits(blockIdx.x, tid0); else load_obs(blockIdx.x, tid0);
    }
    // the planes of a leaf handed over through LDS by the tree code of this workgroup (select_body's lds_leaf): what load_bits forms
    auto planes_from_lds = [&](int tid) {
        int nst = 0;
#pragma unroll
        for (int q8 = 0; q8 < 8; ++q8) nst += __popcll(res_leaf[q8]);
        const int tm = reinterpret_cast<const int *>(res_leaf + 2 * RZ_BOARD_WORDS)[0], lc = reinterpret_cast<const int *>(res_leaf + 2 * RZ_BOARD_WORDS)[1];
        const int word = (tid >> 6) & 3, bit = tid & 63;
        const uint64_t w0 = res_leaf[word], w1 = res_leaf[4 + word];
        const bool s0 = (w0 >> bit) & 1ull, s1 = (w1 >> bit) & 1ull;
        const bool mine_ = tm == 0 ? s0 : s1, theirs = tm == 0 ? s1 : s0;
        const _Float16 one = (_Float16)sp::kObsScale, zero = (_Float16)0.0f;
        cell_planes[0] = mine_ ? one : zero;
        cell_planes[1] = theirs ? one : zero;
        cell_planes[2] = (nst > 0 && tid == lc) ? one : zero;
        cell_planes[3] = (nst & 1) ? zero : one;
    };
    __builtin_amdgcn_sched_barrier(0);  // the loads above stay above the zeroing
    NET_TICK(11);
    {
        // What a VALID position reads and no board writes must be zero: the observation planes' halo (all of in0: 5.8 KB)
        // and, in c1 / c2, the ring of positions around the board (row 0, row BH + 1, column 0, column BW + 1 of the halo
        // grid).  Positions further out are read only by MFMA columns that are not positions of the board (tile padding:
        // a column's garbage stays in that column and is never stored), and the board's own positions are overwritten by
        // every board: 64 positions x 2 pieces on a 15x15 board instead of 147 KB, numbered densely (an LDS store costs
        // its issue whatever the number of active lanes).
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 *z = reinterpret_cast<f32x4 *>(lds_raw);
        for (int i = tid0; i < kInB / 16; i += kThreads) z[i] = zero;
        const int n_ring = 2 * (BW + 2) + 2 * BH;
        for (int it = tid0; it < 2 * n_ring; it += kThreads) {
            const int piece = it >= n_ring, idx = it - piece * n_ring;
            int py, px;
            if (idx < 2 * (BW + 2)) {
                const int bottom = idx >= BW + 2;
                py = bottom ? BH + 1 : 0;
                px = idx - bottom * (BW + 2);
            } else {
                const int j = idx - 2 * (BW + 2);
                py = 1 + (j >> 1);
                px = (j & 1) ? BW + 1 : 0;
            }
            const int pos = py * RW + px;
            f32x4 *q1 = reinterpret_cast<f32x4 *>(c1 + piece * sp::Geo<32, POS>::piece_bytes + pos * sp::Geo<32>::pos_bytes);
#pragma unroll
            for (int i = 0; i < sp::Geo<32>::pos_bytes / 16; ++i) q1[i] = zero;
            f32x4 *q2 = reinterpret_cast<f32x4 *>(c2 + piece * sp::Geo<64, POS>::piece_bytes + pos * sp::Geo<64>::pos_bytes);
#pragma unroll
            for (int i = 0; i < sp::Geo<64>::pos_bytes / 16; ++i) q2[i] = zero;
        }
    }
    NET_TICK(12);
    __syncthreads();
    NET_TICK(13);
    // (the head weights go to LDS behind the first board's conv1: they are first read two barriers later, and their
    // loads need not be waited for here)
    bool hw_pending = true;
    if constexpr (RES) {
        if (sel_first) {   // AlphaZeroMCTS._playout's select loop for the first simulation of the search (rz_select_step's work)
            if ((tid0 >> 6) == 0) rzt::select_body<false, kResWords, rzt::NoHook, PUCT>(res.E, nullptr, blockIdx.x, tid0 & 63, 0, res_leaf);
            __syncthreads();
            planes_from_lds(tid0);
        }
    }
    if (first) store_obs(tid0);
    NET_TICK(14);
    __syncthreads();
#ifdef RZ_NET_PROFILE
    NET_TICK(15);
    prof_acc[9] = prof_t - prof_k0;   // the prologue
#endif
    for (int board = blockIdx.x, sim = 0; RES ? sim < res_n : board < n_boards; RES ? (void)++sim : (void)(board += gridDim.x)) {
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int next_board = RES ? n_boards : board + (int)gridDim.x;   // (RES: the next leaf does not exist yet)
    // MS = 3 (three N-tiles of 3 rows: 9x9): waves 0 .. 2 = the tiles with M-tiles 0 .. 2 of conv3 (and all of conv1 / conv2),
    // wave 3 = part 1 = conv3's M-tile 3 for ALL three tiles: 9 MFMAs per K-step in every wave instead of 12 in three
    constexpr int kTiles = MS == 3 ? 3 : 4 / MS;          // waves side by side over the board's rows
    const int tile = MS == 1 ? wave : (MS == 3 ? (wave < 3 ? wave : 0) : wave % kTiles);
    const int part = MS == 1 ? 0 : (MS == 3 ? (wave == 3 ? 1 : 0) : wave / kTiles);
    constexpr int TM2 = (MS == 1 || MS == 3) ? 2 : 1, TM3 = MS == 3 ? 3 : 4 / MS;   // M-tiles of conv2 / conv3 per wave
    const int m2 = (MS == 1 || MS == 3) ? 0 : (part & 1), m3 = MS == 3 ? 0 : part * TM3;   // ... starting at
    const bool conv2_mine = MS == 3 ? part == 0 : (MS < 4 || part < 2);   // (conv2 has two M-tiles: with MS = 4 parts 2, 3 sit it out)
    const char *s2p = reinterpret_cast<const char *>(nd.s2) + (size_t)m2 * sp::Geo<32>::steps * 2 * 1024;
    const char *s3p = reinterpret_cast<const char *>(nd.s3) + (size_t)m3 * sp::Geo<64>::steps * 2 * 1024;
    sp::f16x8 a2[sp::ring_depth(TM2, TN)][TM2][2];
    sp::preload_w<32, TM2, TN>(a2, s2p, lane);
    // the lane's column of an N-tile: position (ry, x) of a tile of RT rows (TN = 2: always 2 x 16); a lane past the
    // tile's positions computes position (0, 0) again and stores nothing
    const int RT = TN == 2 ? 2 : nd.tile_rows, CT = TN == 2 ? 16 : nd.tile_cols;
    const int n = lane & 31, h = lane >> 5;
    const int ry_raw = TN == 2 ? n >> 4 : (n * nd.tile_rcp) >> 16;
    const bool col_ok = ry_raw < RT;
    const int ry = col_ok ? ry_raw : 0, x = col_ok ? n - ry_raw * CT : 0;
    const int row0 = RT * TN * tile;       // first board row of this wave
    // a wave below the board skips its MFMA loops (it still meets the barriers); with TN = 2 its rows stay inside the
    // halo grid and it computes them unconditionally (a branch around the loops costs the accumulators their registers)
    const bool busy = row0 < BH;
    if (busy && part == 0) {   // conv1: 4 -> 32 (one M-tile), N-tiles TN*wave ..; K-step = kernel row ky
        typedef const __attribute__((address_space(3))) sp::f16x4 *lds_half;
        const lds_half q = (lds_half)(in0 + ((row0 + ry) * IC + x + 2 * h) * 8);
        sp::f16x8 b1[3][TN][2];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int t = 0; t < TN; ++t)
#pragma unroll
                for (int p_ = 0; p_ < 2; ++p_) {
                    const int o = ((2 * t + ky) * IC * 8 + p_ * kInPiece) / 8;
                    const sp::f16x4 lo4 = q[o], hi4 = q[o + 1];
                    b1[ky][t][p_] = __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
                }
        sp::f32x16 acc1[TN];
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc1[t][r] = 0.0f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int combo = 0; combo < 3; ++combo)
#pragma unroll
                for (int t = 0; t < TN; ++t)
                    acc1[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[ky][combo == 2], b1[ky][t][combo == 1], acc1[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            const int y = row0 + 2 * t + ry;
            if (col_ok && y < BH && x < BW) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float z[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[j] = fmaxf(fmaf(acc1[t][4 * g + j], k1, bias1[g][j]), 0.0f);
                    zmax = fmaxf(fmaxf(zmax, fmaxf(z[0], z[1])), fmaxf(z[2], z[3]));
                    sp::f16x4 hi, lo;
                    sp::split4(z, hi, lo);
                    char *dst = c1 + ((y + 1) * RW + (x + 1)) * sp::Geo<32>::pos_bytes + (8 * g + 4 * h) * 2;
                    *reinterpret_cast<sp::f16x4 *>(dst) = hi;
                    *reinterpret_cast<sp::f16x4 *>(dst + sp::Geo<32, POS>::piece_bytes) = lo;
                }
            }
        }
    }
    if (hw_pending) {
#pragma unroll
        for (int k = 0; k < kHwPer; ++k) {
            const int i = tid0 + k * kThreads;
            if (i < 128 * 7) hw[i] = hw_reg[k];
        }
        if (tid0 < 8) hw[128 * 7 + tid0] = bh_reg;
        hw_pending = false;
    }
    NET_TICK(0);
    __syncthreads();
    NET_TICK(1);
    if (next_board < n_boards) {
        if (from_bits) load_bits(next_board, tid); else load_obs(next_board, tid);
    }
    sp::f16x8 a3[sp::ring_depth(TM3, TN)][TM3][2];
    {   // conv2: 32 -> 64
        sp::f32x16 acc[TM2][TN];
        f32x4 bias2[TM2][4];  // fetched before the MFMA loop
#pragma unroll
        for (int m = 0; m < TM2; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) bias2[m][g] = *reinterpret_cast<const f32x4 *>(nd.b2 + (m2 + m) * 32 + 8 * g + 4 * h) * act2;
        if (TN == 2 || (busy && conv2_mine)) sp::conv<32, TM2, TN, 2, RW, POS>(c1, s2p, row0, ry, x, lane, a2, acc);
        NET_TICK(2);
        sp::preload_w<64, TM3, TN>(a3, s3p, lane);
        // (position outermost: ONE guarded region per N-tile instead of one per group of 4 channels)
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            const int y = row0 + 2 * t + ry;
            if (busy && conv2_mine && col_ok && y < BH && x < BW) {
                char *pos = c2 + ((y + 1) * RW + (x + 1)) * sp::Geo<64>::pos_bytes + (m2 * 32 + 4 * h) * 2;
#pragma unroll
                for (int m = 0; m < TM2; ++m)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 bv = bias2[m][g];
                        float z[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) z[j] = fmaxf(fmaf(acc[m][t][4 * g + j], k2, bv[j]), 0.0f);
                        zmax = fmaxf(fmaxf(zmax, fmaxf(z[0], z[1])), fmaxf(z[2], z[3]));
                        sp::f16x4 hi, lo;
                        sp::split4(z, hi, lo);
                        char *dst = pos + (m * 32 + 8 * g) * 2;
                        *reinterpret_cast<sp::f16x4 *>(dst) = hi;
                        *reinterpret_cast<sp::f16x4 *>(dst + sp::Geo<64, POS>::piece_bytes) = lo;
                    }
            }
        }
    }
    if (next_board < n_boards) store_obs(tid);
    NET_TICK(3);
    __syncthreads();
    NET_TICK(4);
    {   // conv3: 64 -> 128; its ReLU'd output feeds the two 1x1 head convolutions from registers
        f32x2 vals2[TN][3];  // [position][pair of head outputs]
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int o2 = 0; o2 < 3; ++o2) vals2[t][o2] = f32x2{0.0f, 0.0f};
        f32x2 vals3[3][3];   // MS = 3, wave 3: [tile][pair of head outputs] over the channels of M-tile 3
        if (MS == 3 && part == 1) {
            constexpr int kM = 3;   // the M-tile
            const char *s3q = reinterpret_cast<const char *>(nd.s3) + (size_t)kM * sp::Geo<64>::steps * 2 * 1024;
            sp::f16x8 a3w[sp::ring_depth(1, 3)][1][2];
            sp::preload_w<64, 1, 3>(a3w, s3q, lane);
            sp::f32x16 accw[1][3];
            sp::conv<64, 1, 3, 3, RW, POS>(c2, s3q, 0, ry, x, lane, a3w, accw);
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int o2 = 0; o2 < 3; ++o2) vals3[t][o2] = f32x2{0.0f, 0.0f};
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = kM * 32 + 8 * g + 4 * h;
                f32x4 wc[7];
#pragma unroll
                for (int i = 0; i < 6; ++i) wc[i] = *reinterpret_cast<const f32x4 *>(hw + c0 * 6 + 4 * i);
                wc[6] = *reinterpret_cast<const f32x4 *>(hw + 768 + c0);
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float hv = fmaxf(fmaf(accw[0][t][4 * g + j], k3, wc[6][j]), 0.0f);
#pragma unroll
                        for (int o2 = 0; o2 < 3; ++o2) {
                            const int e = 6 * j + 2 * o2;
                            vals3[t][o2] = __builtin_elementwise_fma(f32x2{wc[e >> 2][e & 3], wc[e >> 2][(e & 3) + 1]},
                                                                     f32x2{hv, hv}, vals3[t][o2]);
                        }
                    }
            }
        }
        if (MS != 3 || part == 0) {
            sp::f32x16 acc[TM3][TN];
            if (TN == 2 || busy) sp::conv<64, TM3, TN, 2, RW, POS>(c2, s3p, row0, ry, x, lane, a3, acc);
            NET_TICK(5);
            // per (m, g): the lane's channels c0 .. c0+3 = 32*m + 8*g + 4*h ..: 24 head weights [j][output] and 4
            // biases from LDS, fetched one group ahead (the fences keep hipcc from hoisting all 16 groups' reads)
            f32x4 w[2][7];
            auto load_group = [&](int mg, f32x4 (&dstw)[7]) {
                const int c0 = (m3 + (mg >> 2)) * 32 + 8 * (mg & 3) + 4 * h;
#pragma unroll
                for (int i = 0; i < 6; ++i) dstw[i] = *reinterpret_cast<const f32x4 *>(hw + c0 * 6 + 4 * i);
                dstw[6] = *reinterpret_cast<const f32x4 *>(hw + 768 + c0);
            };
            load_group(0, w[0]);
#pragma unroll
            for (int mg = 0; mg < 4 * TM3; ++mg) {
                const int m = mg >> 2, g = mg & 3;
                if (mg + 1 < 4 * TM3) load_group(mg + 1, w[(mg + 1) & 1]);
                const f32x4(&wc)[7] = w[mg & 1];
#pragma unroll
                for (int t = 0; t < TN; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float hv = fmaxf(fmaf(acc[m][t][4 * g + j], k3, wc[6][j]), 0.0f);
#pragma unroll
                        for (int o2 = 0; o2 < 3; ++o2) {
                            const int e = 6 * j + 2 * o2;  // float index of (channel j, outputs 2*o2, 2*o2 + 1)
                            vals2[t][o2] = __builtin_elementwise_fma(f32x2{wc[e >> 2][e & 3], wc[e >> 2][(e & 3) + 1]},
                                                                     f32x2{hv, hv}, vals2[t][o2]);
                        }
                    }
                // pin the partial sums here: their only use is the guarded store below, and hipcc otherwise sinks
                // the whole chains of multiply-adds into that block (every weight and activation kept alive)
                if constexpr (TN == 2)
                    asm volatile("" : "+v"(vals2[0][0]), "+v"(vals2[0][1]), "+v"(vals2[0][2]), "+v"(vals2[TN - 1][0]),
                                 "+v"(vals2[TN - 1][1]), "+v"(vals2[TN - 1][2]));
                else
                    asm volatile("" : "+v"(vals2[0][0]), "+v"(vals2[0][1]), "+v"(vals2[0][2]));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        NET_TICK(6);
        // the two lane halves hold different channels of the same TN positions: with TN = 2 lane half h stores
        // position h, with TN = 1 half 0 stores the one position
        float *dst = feat ? feat + (size_t)board * nd.feat_ld : nullptr;  // null: only the f16 pieces are wanted
        const int y = row0 + (TN == 2 ? 2 * h : 0) + ry;
        const bool mine = busy && part == 0 && col_ok && (TN == 2 || h == 0);
        // MS > 1: the 6 sums of a position are spread over MS waves (their shares of the 128 channels): they meet in LDS
        float *pad_a = reinterpret_cast<float *>(c1 + ((part * kTiles + tile) * 32 + n) * sp::Geo<32>::pos_bytes + 64);
        float *pad_b = reinterpret_cast<float *>(reinterpret_cast<char *>(pad_a) + sp::Geo<32, POS>::piece_bytes);
        if (MS == 3) {   // wave 3 leaves its share of every tile's sums in slot (tile, n)
            if (part == 1) {
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    float *qa = reinterpret_cast<float *>(c1 + (t * 32 + n) * sp::Geo<32>::pos_bytes + 64);
                    float *qb = reinterpret_cast<float *>(reinterpret_cast<char *>(qa) + sp::Geo<32, POS>::piece_bytes);
#pragma unroll
                    for (int o = 0; o < 6; ++o) {
                        float v0 = vals3[t][o >> 1][o & 1];
                        v0 += other_half(v0, h);
                        if (h == 0) (o < 4 ? qa[o] : qb[o - 4]) = v0;
                    }
                }
            }
            __syncthreads();
        } else if (MS > 1) {
#pragma unroll
            for (int o = 0; o < 6; ++o) {
                float v0 = vals2[0][o >> 1][o & 1];
                v0 += other_half(v0, h);
                if (h == 0) (o < 4 ? pad_a[o] : pad_b[o - 4]) = v0;
            }
            __syncthreads();
        }
        // the same features as hi + lo f16 pieces for the A fragments of k_heads_split:
        // [32-board tile][K-step][hi | lo][board % 32][k % 16] -- the 16 values of a board and K-step are one 32-byte
        // sector (written whole by neighbouring lanes of this wave), a wave of the GEMM reads the 1 KB of a piece
        _Float16 *dst16 = feat16 ? feat16 + ((size_t)(board >> 5) * (nd.groups_act + nd.groups_val) * 1024 + (board & 31) * 16)
                                 : nullptr;
        const bool deferred = (RES && !PUCT) || later.slot_of != nullptr;   // (DeferredOut: the policy pieces wait in the store, the value inputs go on as f32)
        float *vdst = nullptr;
        if constexpr (PUCT) {   // no store: every piece stays in LDS for the FC layers behind this stage (fc_here)
            dst16 = nullptr;
        } else if constexpr (RES) {   // the game's slot advances by one per simulation; the value inputs stay in LDS
            dst16 = res_slot0 + sim < later.n_slots ? feat16 + (size_t)(res_slot0 + sim) * later.slot_halfs + (size_t)(board >> 5) * nd.groups_act * 1024 + (board & 31) * 16 : nullptr;
            vdst = res_vrow;
        } else if (deferred) {
            const int slot_ = later.slot_of[board];   // (uniform; beyond the store: nothing is written, expand_backup_body<DEF> flags the game)
            dst16 = slot_ < later.n_slots ? feat16 + (size_t)slot_ * later.slot_halfs + (size_t)(board >> 5) * nd.groups_act * 1024 + (board & 31) * 16 : nullptr;
            vdst = later.valfeat + (size_t)board * later.vf_ld;
        }
        // the six sums of the lane's position first (the other lane half's share by v_permlane32_swap, the biases in one
        // go), then the stores: nothing in the store sequence waits for a cross-lane or LDS round trip
        float vsum[6];
#pragma unroll
        for (int o = 0; o < 6; ++o) {
            float v0 = vals2[0][o >> 1][o & 1], v1 = vals2[TN - 1][o >> 1][o & 1];
            if (MS == 3) {  // channels 0 .. 95 (this wave) + 96 .. 127 (wave 3's slot of this tile)
                const float *q = o < 4 ? pad_a + o : pad_b + (o - 4);   // (part 0: slot (tile, n))
                v0 += other_half(v0, h);
                v0 += q[0];
            } else if (MS > 1) {  // the parts' shares, in part order (every lane reads: part 0's result is the one stored)
                const int stride = kTiles * 32 * sp::Geo<32>::pos_bytes / 4;   // floats from one part's slot to the next
                const float *q = (o < 4 ? pad_a + o : pad_b + (o - 4)) - part * stride;
                v0 = q[0];
#pragma unroll
                for (int p_ = 1; p_ < MS; ++p_) v0 += q[p_ * stride];
            } else {
                v0 += other_half(v0, h);
            }
            if (TN == 2) v1 += other_half(v1, h);
            vsum[o] = (TN == 2 && h) ? v1 : v0;
        }
        float hb[6];
#pragma unroll
        for (int o = 0; o < 6; ++o) hb[o] = hw[128 * 7 + o];
        // FC_HERE: the board's f16 feature pieces [K-step][hi | lo][16] in LDS, inside halo rows 12 .. of conv2's region (a
        // board of up to 10 rows never reads them); zeroed K tail
        const bool fc_here = TN == 1 && raw != nullptr;
        _Float16 *fa_lds = reinterpret_cast<_Float16 *>(c2 + 12 * RW * sp::Geo<64>::pos_bytes);
        const int fc_steps = nd.groups_act + nd.groups_val;
        if (fc_here) {
            for (int i = tid; i < fc_steps * 8; i += kThreads) reinterpret_cast<f32x2 *>(fa_lds)[i] = f32x2{0.0f, 0.0f};
            __syncthreads();
        }
        if (mine && y < BH && x < BW) {
            const int cell = y * BW + x;
#pragma unroll
            for (int o = 0; o < 6; ++o) {
                const float v = fmaxf(vsum[o] + hb[o], 0.0f);
                if (dst) dst[(o < 4 ? o * S : nd.feat_val_off + (o - 4) * S) + cell] = v;
                if (fc_here) {
                    const int k = (o < 4 ? o : o - 4) * S + cell;
                    const int step = (o < 4 ? 0 : nd.groups_act) + (k >> 4);
                    const float z = v * act3;
                    const _Float16 zh = (_Float16)z;
                    zmax = fmaxf(zmax, z);
                    fa_lds[step * 32 + (k & 15)] = zh;
                    fa_lds[step * 32 + 16 + (k & 15)] = (_Float16)(z - (float)zh);
                } else if (deferred && o >= 4) {
                    vdst[(o - 4) * S + cell] = v;
                } else if (dst16) {
                    const int k = (o < 4 ? o : o - 4) * S + cell;
                    const int step = (o < 4 ? 0 : nd.groups_act) + (k >> 4);
                    const float z = v * act3;
                    const _Float16 zh = (_Float16)z;
                    zmax = fmaxf(zmax, z);
                    _Float16 *q = dst16 + (size_t)step * 1024 + (k & 15);
                    q[0] = zh;
                    q[512] = (_Float16)(z - (float)zh);
                }
            }
        }
    }
    NET_TICK(7);
    if constexpr (TN == 1) {
        if (raw != nullptr) {
            // ---- the first FC layers of both heads on this board (k_heads_split's arithmetic: see the kernel's header)
            __syncthreads();   // the feature pieces are in LDS
            const _Float16 *fa_lds = reinterpret_cast<const _Float16 *>(c2 + 12 * RW * sp::Geo<64>::pos_bytes);
            float *ps = reinterpret_cast<float *>(c2 + 15 * RW * sp::Geo<64>::pos_bytes);   // [K quarter][tile][32 outputs]
            const int n_act_tiles = nd.Npad / 32, n_tiles = n_act_tiles + 2;
            const f32x4 *zero_frag = nd.fs_act + (size_t)n_act_tiles * nd.groups_act * 128;
            const int half = lane >> 5;
            const bool row0 = (lane & 31) == 0;   // the lanes that hold MFMA row 0 of the A operand
            for (int tile = 0; tile < n_tiles; ++tile) {
                const bool is_act = tile < n_act_tiles;
                const f32x4 *fb = is_act ? nd.fs_act + (size_t)tile * nd.groups_act * 128
                                         : nd.fs_val + (size_t)(tile - n_act_tiles) * nd.groups_val * 128;
                const int K = is_act ? nd.groups_act : nd.groups_val, a0 = is_act ? 0 : nd.groups_act;
                const int k0 = wave * K / 4, k1 = (wave + 1) * K / 4;
                sp::f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
                constexpr int D = 4;   // weight fragments in flight (every load unconditional: see fs_load)
                sp::f16x8 bw[D][2];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const f32x4 *src = k0 + d < k1 ? fb + (size_t)(k0 + d) * 128 : zero_frag;
#pragma unroll
                    for (int p_ = 0; p_ < 2; ++p_) bw[d][p_] = __builtin_bit_cast(sp::f16x8, src[p_ * 64 + lane]);
                }
                for (int k = k0; k < k1; k += D) {
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        if (k + d < k1) {   // (wave-uniform)
                            const sp::f16x8 zero8 = {(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f,
                                                     (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
                            const _Float16 *src = fa_lds + (a0 + k + d) * 32 + 8 * half;
                            const sp::f16x8 ah = row0 ? *reinterpret_cast<const sp::f16x8 *>(src) : zero8;
                            const sp::f16x8 al = row0 ? *reinterpret_cast<const sp::f16x8 *>(src + 16) : zero8;
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bw[d][0], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bw[d][1], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bw[d][0], acc, 0, 0, 0);
                        }
                        const f32x4 *src2 = k + d + D < k1 ? fb + (size_t)(k + d + D) * 128 : zero_frag;
#pragma unroll
                        for (int p_ = 0; p_ < 2; ++p_) bw[d][p_] = __builtin_bit_cast(sp::f16x8, src2[p_ * 64 + lane]);
                    }
                }
                if (half == 0) ps[(wave * n_tiles + tile) * 32 + (lane & 31)] = acc[0];   // D row 0 = this board, column = output
            }
            __syncthreads();
            const float sc_act = nd.s_inv[3], sc_val = nd.s_inv[4];
            for (int i = tid; i < n_tiles * 32; i += kThreads) {
                const int tile = i >> 5, col = i & 31;
                float v = ps[(0 * n_tiles + tile) * 32 + col];
#pragma unroll
                for (int q = 1; q < 4; ++q) v += ps[(q * n_tiles + tile) * 32 + col];
                if (tile < n_act_tiles) {
                    const int c = 32 * tile + col;
                    raw[(size_t)board * nd.Npad + c] = fmaf(v, sc_act, nd.fc_act_b[c]);
                } else {
                    const int c = 32 * (tile - n_act_tiles) + col;
                    hid[(size_t)board * 64 + c] = fmaxf(fmaf(v, sc_val, nd.fc_val1_b[c]), 0.0f);
                }
            }
            __syncthreads();   // (a further board of this workgroup reuses the pieces and the partial sums)
        }
    }
    if constexpr (PUCT) {
        // ---- the rest of the simulation under RZ_SCORE_PUCT: the body of k_tree_step_raw on this game's rows of raw / hid, which the
        // FC layers above have just written (their last barrier stands between those stores and wave 0's loads)
        const int game = blockIdx.x;
        rz_raw_heads rh = rz_raw_heads();
        rh.raw = raw;
        rh.hid = hid;
        rh.w2 = nd.fc_val2_w;
        rh.b2 = nd.fc_val2_b;
        rh.ld = nd.Npad;
        rh.n_parts = 1;
        // (expand_backup_body<RAW> holds no barrier: waves 1 .. 3 wait at the one below)
        if (wave == 0) rzt::expand_backup_body<float, false, true, false, false, kResWords>(res.E, nullptr, nullptr, game, lane, rh);
        __syncthreads();        // the tree's updates before the selection's loads
        NET_TICK(17);
        const bool more = sim + 1 < res_n;
        if (wave == 0 && more) rzt::select_body<false, kResWords, rzt::NoHook, true>(res.E, nullptr, game, lane, 0, res_leaf);   // (forced playouts: Dev::forced_k)
        __syncthreads();
        NET_TICK(18);
        if (more) {   // the planes of the next leaf, from LDS
            planes_from_lds(tid);
            store_obs(tid);
            __syncthreads();
        }
        NET_TICK(19);
    } else if constexpr (RES) {
        // ---- the rest of the simulation, by the same workgroup (see k_trunk_rows: the body of k_tree_step_def, rz_tree.h)
        __syncthreads();   // the value head's inputs are in LDS
        const int game = blockIdx.x;
        // (two workgroups per CU -- the compact grid --: the serial part of a simulation ahead of the other game's trunk waves at issue,
        // as in k_delta_res)
        if (RW != kRowW && RZ_SPLIT_TREE_PRIO) __builtin_amdgcn_s_setprio(RZ_SPLIT_TREE_PRIO);
        if (res.vh.groups == 64) rzt::value_quarter_lds<8>(res.vh, res_vrow, lane, wave, res_part);
        else if (res.vh.groups == 32) rzt::value_quarter_lds<4>(res.vh, res_vrow, lane, wave, res_part);
        else rzt::value_quarter_lds<2>(res.vh, res_vrow, lane, wave, res_part);
        NET_TICK(16);
        if (wave == 0) rzt::expand_backup_body<float, false, false, false, true, kResWords>(res.E, nullptr, nullptr, game, lane, rz_raw_heads(), 0, res.vh, res_part);
        else __syncthreads();   // (the barrier inside the body, where the quarters meet)
        __syncthreads();        // the tree's updates before the selection's loads
        NET_TICK(17);
        const bool more = sim + 1 < res_n;
        if (wave == 0 && more) rzt::select_body<false, kResWords>(res.E, nullptr, game, lane, 0, res_leaf);
        if (RW != kRowW && RZ_SPLIT_TREE_PRIO) __builtin_amdgcn_s_setprio(0);
        __syncthreads();
        NET_TICK(18);
        if (more) {   // the planes of the next leaf, from LDS: what load_bits forms from the leaf arrays
            planes_from_lds(tid);
            store_obs(tid);
            __syncthreads();
        }
        NET_TICK(19);
    }
    }  // boards
#ifdef RZ_NET_PROFILE
    if (blockIdx.x == 0 && tid0 == 0) {
        for (int i = 0; i < 24; ++i) net_prof[i] = prof_acc[i];
        net_prof[10] = __builtin_readcyclecounter() - prof_k0;
    }
#endif
    if (!(zmax <= 65504.0f)) atomicOr(flags, (unsigned)RZ_NET_FLAG_F16_RANGE);
}

}  // namespace
