// rz_net_rows.h -- the row trunk of rz_net.hip (boards of 11 .. 16 rows and columns): namespace rt, trunk_rows_body and its two
// kernels k_trunk_rows (a launch per step) and k_trunk_rows_res (the resident search).  rz_delta.h is this arithmetic cell by cell.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <utility>

#include "rlzero_hip.h"
#include "rz_net_dev.h"
#include "rz_net_split.h"
#include "rz_trace.h"
#include "rz_tree.h"

namespace {

// ------------------------------------------------------------------ row-tile trunk (wide boards: 11 .. 16 columns)
// The arithmetic of k_trunk_split (hi + lo f16 operands, three MFMAs per product, f32 accumulation) on
// v_mfma_f32_16x16x32_f16 with the work split over the waves by OUTPUT CHANNEL instead of by board row:
//   * N-tile = ONE board row (16 columns), K-step = 32 input channels of one tap, M-tile = 16 output channels.  A 15 x 15
//     board is 15 N-tiles (240 MFMA columns for 225 positions) where 2-row x 16-column tiles of the 32 x 32 MFMA need 8 x 32 =
//     256, and no wave owns a row that does not exist.
//   * wave w owns output channels 16 w .. 16 w + 15 of conv2 and 32 w .. 32 w + 31 of conv3 for ALL rows: every weight
//     fragment is fetched by one wave instead of four (L2 -> CU traffic of conv3: 295 KB per board instead of 1.18 MB), the
//     activation fragments (LDS) by all four.
//   * the chip holds a higher clock in this MFMA shape (profiles/r03/conv3_shapes.txt: the conv3 loop on every CU, random
//     data: 1.75 GHz against 1.52 GHz and 6 % fewer cycles: 17.1 against 20.5 us per board).
// LDS: a position's record is [hi: CIN f16][lo: CIN f16][32 bytes of padding] (160 / 288 bytes): lane = 16 * (k block) +
// column reads the 8 channels of its k block with one ds_read_b128, and record size / 16 = 2 (mod 4) puts the 16 lanes of
// every LDS cycle on 16 different 16-byte slots.  The head convolutions: a lane holds 8 of the 128 channels of a position,
// so the 6 sums of a position are spread over 4 lanes x 4 waves: lanes meet by v_permlane16/32_swap (reduce-scatter), waves
// in LDS (inside the board positions of conv1's region, which the next board overwrites anyway); thread = cell then adds
// the four waves' shares in wave order and stores the features.
namespace rt {

using sp::f16x4;
using sp::f16x8;
using sp::lds_frag;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

template <int CIN> struct Geo {
    static constexpr int pos_bytes = 4 * CIN + 32;               // 160 / 288
    static constexpr int grid_bytes = sp::kGridPos * pos_bytes;  // 51 840 / 93 312
    static constexpr int chunks = CIN / 32, steps = 9 * chunks;
    static_assert((pos_bytes / 16) % 4 == 2, "conflict-free ds_read_b128");
};
constexpr int kLA = 3;   // activation fragments are requested kLA rows ahead
constexpr int kLdsBytes = sp::kInBytes + Geo<32>::grid_bytes + Geo<64>::grid_bytes;
static_assert(kLdsBytes <= 160 * 1024, "LDS budget");

// The K loop, rows innermost: for every (tap column dx, channel chunk) -- a "combo" -- the NT live halo rows 1 .. NT are read
// ONCE each and a row's fragment meets the three kernel rows (output rows r - dy): 9 * TM MFMAs per pair of ds_read_b128, a
// third of the LDS reads of a (tap, row) order (profiles/microbench/conv3_shapes.hip: R16 against C16; +2.1 .. 2.7 % on the whole
// bench); the 3 * TM weight fragments of a combo's three kernel rows sit in registers, the next combo's arrive meanwhile.
// Halo rows 0 and NT + 1 are the zero ring above / below the board (the kernel runs boards of exactly NT rows): never read,
// their products never formed (2 of 45 (row, kernel row) pairs = 4.4 % of a layer's MFMAs; +2.3 %).
// F8 (conv3 of RZ_NET_SPLIT_F16_FP8; CIN = 64): a position's record is [hi: 64 f16][hi8: 64 e5m2 of the value][lo8: 64 e5m2 of
// (value - hi) 2^11][pad] and a "combo" is (tap column dx, part): part 0 = the hi x hi products of the tap's two 32-channel chunks (two
// v_mfma_f32_16x16x32_f16 per kernel row and M-tile), part 1 = BOTH cross terms of the tap's 64 channels in one
// v_mfma_scale_f32_16x16x128_f8f6f4 (A = e4m3 weights, B = e5m2 activations; lane group g: K block = [hi8 x (w_lo 2^5)8 | lo8 x
// (w_hi 2^-6)8] of channels 16 g .. 16 g + 15, one scale 2^-5 for the block).  The same fragment addresses, loads per slot and
// registers as the three-MFMA loop; 2 f16-MFMA equivalents per product instead of 3 (profiles/microbench/conv3_shapes.hip: F8).
__device__ __forceinline__ i32x8 cat8(f16x8 lo, f16x8 hi) {
    return __builtin_shufflevector(__builtin_bit_cast(i32x4, lo), __builtin_bit_cast(i32x4, hi), 0, 1, 2, 3, 4, 5, 6, 7);
}
constexpr int kF8ScaleA = 127 - 5, kF8ScaleB = 127;   // E8M0: the weights' bytes carry 2^5 (pack_rows_f8), the activations' 2^0
template <int CIN, int TM, int NT, int J, bool F8 = false>
__device__ __forceinline__ void slot_r(f32x4 (&acc)[TM][NT], f16x8 (&a)[2][3][TM][2], f16x8 (&b)[kLA + 1][2], lds_frag q, lds_frag qf,
                                       __amdgpu_buffer_rsrc_t w_rsrc, int w_lane) {
    using G = Geo<CIN>;
    static_assert(!F8 || CIN == 64, "the FP8 cross terms: one tap of 64 channels = one K = 128 block");
    constexpr int PD = kLA + 1, combos = 3 * G::chunks, cb = J / NT, r = J % NT + 1, J2 = J + kLA;   // r: halo row
    constexpr int second = F8 ? 64 : CIN * 2;   // the second fragment of a slot: the other chunk (F8) / the lo piece
    if constexpr (J2 < combos * NT) {
        constexpr int cb2 = J2 / NT, r2 = J2 % NT + 1, dx = cb2 / G::chunks, c = cb2 % G::chunks, far = r2 >= 8;
        constexpr int off = ((r2 - 8 * far) * kRowW + dx) * G::pos_bytes + c * (F8 ? 128 : 64);
        static_assert(off % 16 == 0 && off + second < 65536, "ds_read_b128 immediate");
        b[J2 % PD][0] = (far ? qf : q)[off / 16];
        b[J2 % PD][1] = (far ? qf : q)[(off + second) / 16];
    }
    if constexpr (cb + 1 < combos && r - 1 < 3 * TM) {   // the next combo's weight fragments behind this combo's first rows
        constexpr int dy = (r - 1) / TM, m = (r - 1) % TM, dx = (cb + 1) / G::chunks, c = (cb + 1) % G::chunks;
#pragma unroll
        for (int p = 0; p < 2; ++p)
            a[(cb + 1) % 2][dy][m][p] = sp::load_w(w_rsrc, w_lane, ((m * G::steps + (dy * 3 + dx) * G::chunks + c) * 2 + p) * 1024);
    }
    if constexpr (F8) {
        constexpr int part = cb % 2;
#pragma unroll
        for (int c = 0; c < (part ? 1 : 2); ++c)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int m = 0; m < TM; ++m) {
                    const int t = r - dy;
                    if (t >= 0 && t < NT) {
                        if (part) {
                            acc[m][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(cat8(a[cb % 2][dy][m][0], a[cb % 2][dy][m][1]),
                                                                                         cat8(b[J % PD][0], b[J % PD][1]), acc[m][t],
                                                                                         0 /* A: e4m3 */, 1 /* B: e5m2 */, 0, kF8ScaleA, 0, kF8ScaleB);
                        } else if (cb == 0 && c == 0 && (dy == 0 || (t == 0 && dy == 1))) {   // a row's first product (as below)
                            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                            acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0][dy][m][0], b[J % PD][0], zero, 0, 0, 0);
                        } else {
                            acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[cb % 2][dy][m][c], b[J % PD][c], acc[m][t], 0, 0, 0);
                        }
                    }
                }
        __builtin_amdgcn_sched_barrier(0);
        return;
    }
#pragma unroll
    for (int combo = 0; combo < 3; ++combo)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int m = 0; m < TM; ++m) {
                const int t = r - dy, pa = combo == 2 ? 1 : 0, pb = combo == 1 ? 1 : 0;   // halo row r = board row r - 1 = tap row dy of output row r - dy
                if (t >= 0 && t < NT) {
                    // a row's first product: combo 0 of (cb = 0, dy = 0) at halo row t -- board row 0 would meet dy = 0 at halo
                    // row 0 (the zero ring, never read): its first is dy = 1 at halo row 1
                    if (cb == 0 && combo == 0 && (dy == 0 || (t == 0 && dy == 1))) {
                        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                        acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[cb % 2][dy][m][pa], b[J % PD][pb], zero, 0, 0, 0);
                    } else {
                        acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[cb % 2][dy][m][pa], b[J % PD][pb], acc[m][t], 0, 0, 0);
                    }
                }
            }
    __builtin_amdgcn_sched_barrier(0);
}

template <int CIN, int TM, int NT, bool F8, int... Js>
__device__ __forceinline__ void slots_r(std::integer_sequence<int, Js...>, f32x4 (&acc)[TM][NT], f16x8 (&a)[2][3][TM][2],
                                        f16x8 (&b)[kLA + 1][2], lds_frag q, lds_frag qf, __amdgpu_buffer_rsrc_t w_rsrc, int w_lane) {
    (slot_r<CIN, TM, NT, Js, F8>(acc, a, b, q, qf, w_rsrc, w_lane), ...);
}

// the weight fragments of combo 0 (tap column 0, chunk 0; kernel rows 0 .. 2): requested while the previous layer is reduced
template <int CIN, int TM>
__device__ __forceinline__ void preload_w_r(f16x8 (&a)[2][3][TM][2], const void *wts, int lane) {
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(wts), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int p = 0; p < 2; ++p)
                a[0][dy][m][p] = sp::load_w(w_rsrc, lane * 16, ((m * Geo<CIN>::steps + dy * 3 * Geo<CIN>::chunks) * 2 + p) * 1024);
}

template <int CIN, int TM, int NT, bool F8 = false>
__device__ __forceinline__ void conv_r(const char *in, const void *wts, int lane, f16x8 (&a)[2][3][TM][2], f32x4 (&acc)[TM][NT]) {
    using G = Geo<CIN>;
    static_assert(3 * TM <= NT && kLA <= NT, "loads are spread over a combo's first rows");
    const int n = lane & 15, g = lane >> 4;
    const lds_frag q = (lds_frag)(in + n * G::pos_bytes + g * 16), qf = q + 8 * kRowW * G::pos_bytes / 16;
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(wts), 0, 0x7fffffff, 0x00020000);
    f16x8 b[kLA + 1][2];
#pragma unroll
    for (int j = 0; j < kLA; ++j) {   // slots 0 .. kLA - 1: combo 0 (dx = 0, chunk 0), halo rows 1 ..
        b[j][0] = q[((j + 1) * kRowW * G::pos_bytes) / 16];
        b[j][1] = q[((j + 1) * kRowW * G::pos_bytes + (F8 ? 64 : CIN * 2)) / 16];
    }
    __builtin_amdgcn_sched_barrier(0);
    slots_r<CIN, TM, NT, F8>(std::make_integer_sequence<int, 3 * G::chunks * NT>{}, acc, a, b, q, qf, w_rsrc, lane * 16);
}

}  // namespace rt

// Register budget: 200 VGPRs + 200 accumulation registers.  Two lanes of games overlap because a wave of the other lane's tree
// step or FC GEMM (112 / 104 registers) fits beside a trunk wave on the same SIMD (512 registers): at 400 registers or fewer the
// trunk leaves that room, at 408 it does not and the lanes' kernels take turns (measured: 10.7 -> 9.5 M sims/s from 8 registers).
// Left alone hipcc allocates 396 .. 420 here depending on details of the prologue; the cap holds it at 372, no scratch.
// TRACE (rz_trace.h): instantiated for the 15-row bitboard kernel only -- the layout whose schedule profiles/lane_timeline.py reads;
// the production kernels carry nothing of it (its live values cost ten registers of a budget that is pinned).
// F8: conv3 with its cross terms on the block-scaled FP8 pipe (RZ_NET_SPLIT_F16_FP8, opt-in: narrower arithmetic than the reference's
// f32 -- rt::slot_r): conv2's epilogue stores the e5m2 pieces where the lo f16 pieces stood, conv3 reads nd.t3f.
// The body is shared by two kernels: k_trunk_rows (the launches of a lane's step: the register cap above) and k_trunk_rows_res (the
// resident search: a workgroup has its CU to itself for a whole search, no other lane's waves to make room for -- no cap, so the
// tree code's registers beside the trunk's need no scratch).
template <int NT, bool BITS, bool TRACE, bool RES, bool F8>
__device__ __forceinline__ void trunk_rows_body(const NetDev &nd, const float *__restrict__ obs, LeafBits leaves,
                                                float *__restrict__ feat, _Float16 *__restrict__ feat16,
                                                int n_boards, unsigned *__restrict__ flags, const DeferredOut &later, const ResArgs<RES> &res) {
    static_assert(!RES || (BITS && !TRACE), "the resident search reads positions");
    static_assert(!F8 || (BITS && !TRACE), "the FP8 cross terms: position-fed launches only");
    // RES: the value head's input row (zero padded to 4 x groups floats), the K-quarter sums of its first layer, the next leaf
    __shared__ float res_vrow[RES ? 512 : 1];
    __shared__ float res_part[RES ? rzt::kDefWaves : 1][RES ? rzt::kWave : 1];
    __shared__ __attribute__((aligned(16))) uint64_t res_leaf[RES ? 2 * RZ_BOARD_WORDS + 1 : 1];
    int res_slot0 = 0;
    int res_n = 0;   // (RES: the simulations of this workgroup's game)
    if constexpr (RES) {
        if ((int)blockIdx.x >= n_boards || res.E.active[blockIdx.x] == 0) return;   // (uniform: before any barrier)
        res_slot0 = res.E.pend[blockIdx.x];
        res_n = res_sims(res, blockIdx.x);
        for (int i = threadIdx.x; i < 512; i += 256) res_vrow[i] = 0.0f;
    }
#ifdef RZ_NET_PROFILE
    const long long prof_k0 = __builtin_readcyclecounter();
    long long prof_acc[24] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, prof_t = prof_k0;
#endif
    constexpr int kThreads = 256;
    constexpr int P1 = rt::Geo<32>::pos_bytes, P2 = rt::Geo<64>::pos_bytes;
    __shared__ __attribute__((aligned(16))) char lds_raw[rt::kLdsBytes];
    char *in0 = lds_raw;                      // observation planes, pieces hi | lo (as k_trunk_split)
    char *c1 = lds_raw + sp::kInBytes;        // conv1 output, records [hi 32 | lo 32 | pad]
    char *c2 = c1 + rt::Geo<32>::grid_bytes;  // conv2 output, records [hi 64 | lo 64 | pad]
    const int tid0 = threadIdx.x;
    __shared__ unsigned long long trace_t0;   // (parked in LDS: the register budget below is pinned)
    if (TRACE && tid0 == 0) trace_t0 = rz_trace_now();
    const int BH = nd.BH, BW = nd.BW, S = nd.S;
    float zmax = 0.0f;  // largest scaled value this thread stored as f16 pieces (float planes only: bitboard planes are 0 / 1)
    constexpr int kObsPer = BITS ? 1 : (4 * RZ_MAX_BOARD_SIZE * RZ_MAX_BOARD_SIZE + kThreads - 1) / kThreads;
    float ob[kObsPer];
    int obs_off[kObsPer];
    if constexpr (!BITS) {
#pragma unroll
        for (int k = 0; k < kObsPer; ++k) {
            const int i = tid0 + k * kThreads;
            const int c = i / S, r = i - c * S, y = r / BW, x = r - y * BW;
            obs_off[k] = i < 4 * S ? ((y + 1) * sp::kInCols + (x + 1)) * 8 + c * 2 : -1;
        }
    }
    auto load_obs = [&](int board, int tid) {
        if constexpr (!BITS) {
            const float *src = obs + (size_t)board * 4 * S;
#pragma unroll
            for (int k = 0; k < kObsPer; ++k) {
                const int i = tid + k * kThreads;
                ob[k] = i < 4 * S ? src[i] : 0.0f;
            }
        }
    };
    // thread t owns cell t (S <= 256 = threads): the planes of the bitboard route, and the cell whose features it stores
    const int cell_y = tid0 / BW, cell_x = tid0 - cell_y * BW;
    const int cell_off = tid0 < S ? ((cell_y + 1) * sp::kInCols + (cell_x + 1)) * 8 : -1;
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
    auto load_board = [&](int board, int tid) {
        if constexpr (BITS) load_bits(board, tid); else load_obs(board, tid);
    };
    auto store_obs = [&]() {
        if constexpr (BITS) {
            if (cell_off >= 0) {
                *reinterpret_cast<sp::f16x4 *>(in0 + cell_off) = cell_planes;
                *reinterpret_cast<sp::f16x4 *>(in0 + sp::kInPieceBytes + cell_off) =
                    sp::f16x4{(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
            }
        } else {
#pragma unroll
            for (int k = 0; k < kObsPer; ++k)
                if (obs_off[k] >= 0) {
                    const float z = ob[k] * sp::kObsScale;
                    const _Float16 hi = (_Float16)z;
                    zmax = fmaxf(zmax, fabsf(z));
                    *reinterpret_cast<_Float16 *>(in0 + obs_off[k]) = hi;
                    *reinterpret_cast<_Float16 *>(in0 + sp::kInPieceBytes + obs_off[k]) = (_Float16)(z - (float)hi);
                }
        }
    };
    // Prologue of a persistent workgroup: every global load is issued first, the LDS is zeroed under their latency.
    const int lane0 = tid0 & 63, wave0 = tid0 >> 6, g0 = lane0 >> 4;
    // the 1x1 head convolutions: the lane's 8 channels of conv3 (32 wave + 16 m + 4 g + j) meet 6 outputs each -- 48 weights
    // and 8 biases that never change: registers for the whole launch
    f32x4 hwr[2][6], b3r[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int c0 = 32 * wave0 + 16 * m + 4 * g0;
#pragma unroll
        for (int i = 0; i < 6; ++i) hwr[m][i] = *reinterpret_cast<const f32x4 *>(nd.whp + c0 * 6 + 4 * i);
        b3r[m] = *reinterpret_cast<const f32x4 *>(nd.b3 + c0);
    }
    float hb[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) hb[o] = nd.bh[o];
    const float k1 = nd.s_inv[2], k2 = nd.s_inv[0], k3 = nd.s_inv[1];
    const float act1 = nd.s_inv[5], act2 = nd.s_inv[6], act3 = nd.s_inv[7];
    // conv1's weights (3 kernel rows x hi / lo) and biases stay in registers for all boards (32 x 32 x 16 tiles, as k_trunk_split)
    sp::f16x8 a1[3][2];
    f32x4 bias1[4];
    {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int p_ = 0; p_ < 2; ++p_) a1[ky][p_] = __builtin_bit_cast(sp::f16x8, nd.s1[(ky * 2 + p_) * 64 + lane0]);
#pragma unroll
        for (int g = 0; g < 4; ++g) bias1[g] = *reinterpret_cast<const f32x4 *>(nd.b1 + 8 * g + 4 * (lane0 >> 5)) * act1;
    }
    const f32x4 bias2 = *reinterpret_cast<const f32x4 *>(nd.b2 + 16 * wave0 + 4 * g0) * act2;
    const bool first = (int)blockIdx.x < n_boards;
    bool sel_first = false;   // RES: the first leaf is selected by this launch (below, behind the zeroing)
    if constexpr (RES) sel_first = res.select_first != 0;
    if (first && !sel_first) load_board(blockIdx.x, tid0);
    // the planes of a leaf handed over through LDS by the tree code of this workgroup (select_body's lds_leaf): what load_bits forms
    auto planes_from_lds = [&](int tid) {
        int nst = 0;
#pragma unroll
        for (int q8 = 0; q8 < 8; ++q8) nst += __popcll(res_leaf[q8]);
        const int tm = reinterpret_cast<const int *>(res_leaf + 2 * RZ_BOARD_WORDS)[0], lc = reinterpret_cast<const int *>(res_leaf + 2 * RZ_BOARD_WORDS)[1];
        const int word = (tid >> 6) & 3, bit = tid & 63;
        const uint64_t w0 = res_leaf[word], w1 = res_leaf[4 + word];
        const bool s0 = (w0 >> bit) & 1ull, s1 = (w1 >> bit) & 1ull;
        const bool mine = tm == 0 ? s0 : s1, theirs = tm == 0 ? s1 : s0;
        const _Float16 one = (_Float16)sp::kObsScale, zero = (_Float16)0.0f;
        cell_planes[0] = mine ? one : zero;
        cell_planes[1] = theirs ? one : zero;
        cell_planes[2] = (nst > 0 && tid == lc) ? one : zero;
        cell_planes[3] = (nst & 1) ? zero : one;
    };
    __builtin_amdgcn_sched_barrier(0);  // the loads above stay above the zeroing
    NET_TICK(11);
    {
        // what a valid position reads and no board writes must be zero: the observation planes' halo (all of in0) and, in
        // c1 / c2, the ring of positions around the board (whole records)
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 *z = reinterpret_cast<f32x4 *>(lds_raw);
        for (int i = tid0; i < sp::kInBytes / 16; i += kThreads) z[i] = zero;
        const int n_ring = 2 * (BW + 2) + 2 * BH;
        for (int idx = tid0; idx < n_ring; idx += kThreads) {
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
            const int pos = py * kRowW + px;
            f32x4 *q1 = reinterpret_cast<f32x4 *>(c1 + pos * P1);
#pragma unroll
            for (int i = 0; i < P1 / 16; ++i) q1[i] = zero;
            f32x4 *q2 = reinterpret_cast<f32x4 *>(c2 + pos * P2);
#pragma unroll
            for (int i = 0; i < P2 / 16; ++i) q2[i] = zero;
        }
    }
    NET_TICK(12);
    __syncthreads();
    NET_TICK(13);
    if constexpr (RES) {
        if (sel_first) {   // AlphaZeroMCTS._playout's select loop for the first simulation of the search (rz_select_step's work)
            if (wave0 == 0) rzt::select_body<false>(res.E, nullptr, blockIdx.x, lane0, 0, res_leaf);
            __syncthreads();
            planes_from_lds(tid0);
        }
    }
    if (first) store_obs();
    NET_TICK(14);
    __syncthreads();
#ifdef RZ_NET_PROFILE
    NET_TICK(15);
    prof_acc[9] = prof_t - prof_k0;   // the prologue
#endif
    // (RES: the "boards" of this workgroup are the leaves of its game's simulations, one after the other)
    for (int board = blockIdx.x, sim = 0; RES ? sim < res_n : board < n_boards; RES ? (void)++sim : (void)(board += gridDim.x)) {
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int next_board = RES ? n_boards : board + (int)gridDim.x;   // (RES: the next leaf does not exist yet)
    const int n = lane & 15, g = lane >> 4;
    const char *t2p = reinterpret_cast<const char *>(nd.t2) + (size_t)wave * rt::Geo<32>::steps * 2 * 1024;
    const char *t3p = reinterpret_cast<const char *>(F8 ? nd.t3f : nd.t3) + (size_t)(2 * wave) * rt::Geo<64>::steps * 2 * 1024;
    sp::f16x8 a2[2][3][1][2];
    rt::preload_w_r<32, 1>(a2, t2p, lane);
    {   // conv1: 4 -> 32 on 32 x 32 x 16 tiles of 2 rows x 16 columns, wave w = rows 4 w .. 4 w + 3; K-step = kernel row
        const int n32 = lane & 31, h = lane >> 5, ry = n32 >> 4, x = n32 & 15, row0 = 4 * wave;
        if (row0 < BH) {
            typedef const __attribute__((address_space(3))) sp::f16x4 *lds_half;
            const lds_half q = (lds_half)(in0 + ((row0 + ry) * sp::kInCols + x + 2 * h) * 8);
            sp::f16x8 b1[3][2][2];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int p_ = 0; p_ < 2; ++p_) {
                        const int o = ((2 * t + ky) * sp::kInCols * 8 + p_ * sp::kInPieceBytes) / 8;
                        const sp::f16x4 lo4 = q[o], hi4 = q[o + 1];
                        b1[ky][t][p_] = __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
                    }
            sp::f32x16 acc1[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc1[t][r] = 0.0f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int combo = 0; combo < 3; ++combo) {
                    if (BITS && combo == 1) continue;   // the lo pieces of 0 / 1 planes are zero
#pragma unroll
                    for (int t = 0; t < 2; ++t)
                        acc1[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[ky][combo == 2], b1[ky][t][combo == 1], acc1[t], 0, 0, 0);
                }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int y = row0 + 2 * t + ry;
                if (y < BH && x < BW) {
                    char *pos = c1 + ((y + 1) * kRowW + (x + 1)) * P1 + 4 * h * 2;
#pragma unroll
                    for (int gg = 0; gg < 4; ++gg) {
                        float z[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) z[j] = fmaxf(fmaf(acc1[t][4 * gg + j], k1, bias1[gg][j]), 0.0f);
                        if constexpr (!BITS) zmax = fmaxf(fmaxf(zmax, fmaxf(z[0], z[1])), fmaxf(z[2], z[3]));
                        sp::f16x4 hi, lo;
                        sp::split4(z, hi, lo);
                        *reinterpret_cast<sp::f16x4 *>(pos + 8 * gg * 2) = hi;
                        *reinterpret_cast<sp::f16x4 *>(pos + 8 * gg * 2 + 64) = lo;
                    }
                }
            }
        }
    }
    NET_TICK(0);
    __syncthreads();
    NET_TICK(1);
    if (next_board < n_boards) load_board(next_board, tid);
    sp::f16x8 a3[2][3][2][2];
    {   // conv2: 32 -> 64, wave w = output channels 16 w .. 16 w + 15
        f32x4 acc[1][NT];
        rt::conv_r<32, 1, NT>(c1, t2p, lane, a2, acc);
        NET_TICK(2);
        rt::preload_w_r<64, 2>(a3, t3p, lane);
        if (n < BW) {
            char *pos = c2 + (kRowW + n + 1) * P2 + (16 * wave + 4 * g) * 2;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float z[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) z[j] = fmaxf(fmaf(acc[0][t][j], k2, bias2[j]), 0.0f);
                if constexpr (!BITS) zmax = fmaxf(fmaxf(zmax, fmaxf(z[0], z[1])), fmaxf(z[2], z[3]));
                if constexpr (F8) {   // [hi f16 | e5m2 of the value | e5m2 of (value - hi) 2^11]: the lane's 4 channels, 8 + 4 + 4 bytes
                    typedef float f32x4v __attribute__((ext_vector_type(4)));
                    const sp::f16x4 hi = __builtin_convertvector((f32x4v){z[0], z[1], z[2], z[3]}, sp::f16x4);
                    *reinterpret_cast<sp::f16x4 *>(pos + t * kRowW * P2) = hi;
                    int h8 = __builtin_amdgcn_cvt_pk_bf8_f32(z[0], z[1], 0, false);
                    h8 = __builtin_amdgcn_cvt_pk_bf8_f32(z[2], z[3], h8, true);
                    float d[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) d[j] = (z[j] - (float)hi[j]) * 2048.0f;
                    int l8 = __builtin_amdgcn_cvt_pk_bf8_f32(d[0], d[1], 0, false);
                    l8 = __builtin_amdgcn_cvt_pk_bf8_f32(d[2], d[3], l8, true);
                    char *p8 = c2 + (kRowW + n + 1) * P2 + 128 + 16 * wave + 4 * g + t * kRowW * P2;
                    *reinterpret_cast<int *>(p8) = h8;
                    *reinterpret_cast<int *>(p8 + 64) = l8;
                } else {
                sp::f16x4 hi, lo;
                sp::split4(z, hi, lo);
                *reinterpret_cast<sp::f16x4 *>(pos + t * kRowW * P2) = hi;
                *reinterpret_cast<sp::f16x4 *>(pos + t * kRowW * P2 + 128) = lo;
                }
            }
        }
    }
    if (next_board < n_boards) store_obs();
    NET_TICK(3);
    __syncthreads();
    NET_TICK(4);
    // the waves' shares of the head sums: rows of 16 floats [wave][output], inside the board positions of halo row t + 1 of c1
    constexpr int kShare = 6 * 64;   // bytes of a wave's share of one board row
    {   // conv3: 64 -> 128, wave w = output channels 32 w .. 32 w + 31; its ReLU'd output feeds the two 1x1 head convolutions
        float vals[96];   // [row t][output o]: the lane's 8 channels of position (t, n)
        {
            f32x4 acc[2][NT];
            rt::conv_r<64, 2, NT, F8>(c2, t3p, lane, a3, acc);
            NET_TICK(5);
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                f32x2 v2[3] = {f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}};
                if (t < NT) {
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float hv = fmaxf(fmaf(acc[m][t < NT ? t : 0][j], k3, b3r[m][j]), 0.0f);
#pragma unroll
                            for (int o2 = 0; o2 < 3; ++o2) {
                                const int e = 6 * j + 2 * o2;  // float index of (channel j, outputs 2 o2, 2 o2 + 1)
                                v2[o2] = __builtin_elementwise_fma(f32x2{hwr[m][e >> 2][e & 3], hwr[m][e >> 2][(e & 3) + 1]},
                                                                   f32x2{hv, hv}, v2[o2]);
                            }
                        }
                }
#pragma unroll
                for (int o = 0; o < 6; ++o) vals[t * 6 + o] = v2[o >> 1][o & 1];
            }
        }
        // sum over the 4 k blocks (lanes n, n + 16, n + 32, n + 48); lane group g is left with rows 8 (g & 1) + 4 (g >> 1) + 0 .. 3
        float mine[24];
        f4::reduce_scatter_96(vals, mine);
        const int t0 = 8 * (g & 1) + 4 * (g >> 1);
        float *share = reinterpret_cast<float *>(c1 + ((t0 + 1) * kRowW + 1) * P1 + wave * kShare) + n;
#pragma unroll
        for (int i = 0; i < 24; ++i)
            if (t0 + i / 6 < NT) share[(i / 6) * (kRowW * P1 / 4) + (i % 6) * 16] = mine[i];
    }
    NET_TICK(6);
    __syncthreads();
    {
        float *dst = feat ? feat + (size_t)board * nd.feat_ld : nullptr;  // null: only the f16 pieces are wanted
        _Float16 *dst16 = feat16 ? feat16 + ((size_t)(board >> 5) * (nd.groups_act + nd.groups_val) * 1024 + (board & 31) * 16)
                                 : nullptr;
        const bool deferred = RES || later.slot_of != nullptr;
        float *vdst = nullptr;
        if constexpr (RES) {   // the game's slot advances by one per simulation (expand_backup_body<DEF>); the value inputs stay in LDS
            dst16 = res_slot0 + sim < later.n_slots ? feat16 + (size_t)(res_slot0 + sim) * later.slot_halfs + (size_t)(board >> 5) * nd.groups_act * 1024 + (board & 31) * 16 : nullptr;
            vdst = res_vrow;
        } else if (deferred) {   // the policy pieces wait in the store (tiles of groups_act K-steps), the value inputs go on as f32
            const int slot_ = later.slot_of[board];   // (uniform; beyond the store: nothing is written, expand_backup_body<DEF> flags the game)
            dst16 = slot_ < later.n_slots ? feat16 + (size_t)slot_ * later.slot_halfs + (size_t)(board >> 5) * nd.groups_act * 1024 + (board & 31) * 16 : nullptr;
            vdst = later.valfeat + (size_t)board * later.vf_ld;
        }
        if (tid < S) {
            const float *share = reinterpret_cast<const float *>(c1 + ((cell_y + 1) * kRowW + 1) * P1) + cell_x;
            float vsum[6];
#pragma unroll
            for (int o = 0; o < 6; ++o) {
                float v = share[o * 16];
#pragma unroll
                for (int w = 1; w < 4; ++w) v += share[w * (kShare / 4) + o * 16];
                vsum[o] = v;
            }
            const int cell = tid;
#pragma unroll
            for (int o = 0; o < 6; ++o) {
                const float v = fmaxf(vsum[o] + hb[o], 0.0f);
                if (dst) dst[(o < 4 ? o * S : nd.feat_val_off + (o - 4) * S) + cell] = v;
                if (deferred && o >= 4) {
                    vdst[(o - 4) * S + cell] = v;
                } else if (dst16) {
                    const int k = (o < 4 ? o : o - 4) * S + cell;
                    const int step = (o < 4 ? 0 : nd.groups_act) + (k >> 4);
                    const float z = v * act3;
                    const _Float16 zh = (_Float16)z;
                    if constexpr (!BITS) zmax = fmaxf(zmax, z);
                    _Float16 *q = dst16 + (size_t)step * 1024 + (k & 15);
                    q[0] = zh;
                    q[512] = (_Float16)(z - (float)zh);
                }
            }
        }
    }
    NET_TICK(7);
    __syncthreads();   // the shares are read: the next board's conv1 may overwrite them
    NET_TICK(8);
    if constexpr (RES) {
        // ---- the rest of the simulation, by the same workgroup (k_tree_step_def's body: rz_tree.h): the value head's first layer
        // by K-quarters from the row in LDS, then wave 0 -- the game's wave -- finishes the value, reserves the prior block, backs
        // up and selects the next leaf, which comes back through LDS
        const int game = blockIdx.x;
        if (res.vh.groups == 128) rzt::value_quarter_lds<16>(res.vh, res_vrow, lane, wave, res_part);
        else rzt::value_quarter_lds<8>(res.vh, res_vrow, lane, wave, res_part);
        NET_TICK(16);
        if (wave == 0) rzt::expand_backup_body<float, false, false, false, true>(res.E, nullptr, nullptr, game, lane, rz_raw_heads(), 0, res.vh, res_part);
        else __syncthreads();   // (the barrier inside the body, where the quarters meet)
        __syncthreads();        // the tree's updates before the selection's loads
        NET_TICK(17);
        const bool more = sim + 1 < res_n;
        if (wave == 0 && more) rzt::select_body<false>(res.E, nullptr, game, lane, 0, res_leaf);
        __syncthreads();
        NET_TICK(18);
        if (more) {   // the planes of the next leaf, from LDS: what load_bits forms from the leaf arrays
            planes_from_lds(tid);
            // conv1's weight fragments again (6 KB, L2-resident; their latency passes under the barrier below): carried in
            // registers ACROSS the tree code above they cost the resident kernels a spill that was reloaded in every simulation
            asm volatile("" ::: "memory");
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int p_ = 0; p_ < 2; ++p_) a1[ky][p_] = __builtin_bit_cast(sp::f16x8, nd.s1[(ky * 2 + p_) * 64 + lane]);
            store_obs();
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
    if constexpr (!BITS)
        if (!(zmax <= 65504.0f)) atomicOr(flags, (unsigned)RZ_NET_FLAG_F16_RANGE);
    if (TRACE && tid0 == 0 && (int)blockIdx.x < n_boards)
        rz_trace_write(later.trace, RZ_TRACE_TRUNK, later.slot_of ? later.slot_of[blockIdx.x] : 0, blockIdx.x, trace_t0);
}

template <int NT, bool BITS, bool TRACE = false, bool F8 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(200))) void k_trunk_rows(NetDev nd, const float *__restrict__ obs, LeafBits leaves,
                                                    float *__restrict__ feat, _Float16 *__restrict__ feat16,
                                                    int n_boards, unsigned *__restrict__ flags, DeferredOut later) {
    trunk_rows_body<NT, BITS, TRACE, false, F8>(nd, obs, leaves, feat, feat16, n_boards, flags, later, ResArgs<false>{});
}

template <int NT, bool F8 = false>
__global__ __launch_bounds__(256) void k_trunk_rows_res(NetDev nd, LeafBits leaves, _Float16 *__restrict__ feat16, int n_boards,
                                                        unsigned *__restrict__ flags, DeferredOut later, ResArgs<true> res) {
    trunk_rows_body<NT, true, false, true, F8>(nd, nullptr, leaves, nullptr, feat16, n_boards, flags, later, res);
}

}  // namespace
