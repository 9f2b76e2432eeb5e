// rz_net_f32.h -- the kernels of rz_net.hip on the f32-input MFMA (v_mfma_f32_16x16x4_f32, bit-for-bit a k-ordered fmaf chain): the
// direct trunk k_trunk and its fragment helpers, the Winograd F(4x4,3x3) trunk k_trunk_wino_f4 (namespace f4) and the FC GEMM
// k_heads_gemm (k_heads_finish, which every FC route ends with, is in rz_net_heads.h).
#pragma once

#include <hip/hip_runtime.h>

#include <utility>

#include "rz_net_dev.h"

namespace {

// Operand fragments of one input-channel group (4 channels x 9 taps) for a wave that owns TM
// output-channel tiles and NR board rows: TM x 3 packed weight vectors and the (NR+2) x 3
// distinct (row, dx) activation fragments that the 9 taps x NR rows reuse.
template <int TM, int NR>
struct Frags {
    f32x4 a[TM][3];
    float b[NR + 2][3];
};

template <int PL, int TM, int NR, int STEPS>
__device__ __forceinline__ void load_frags(Frags<TM, NR> &f, const float *__restrict__ base,
                                           const f32x4 *__restrict__ wbase, int s) {
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int tg = 0; tg < 3; ++tg) f.a[m][tg] = wbase[((size_t)(m * STEPS + s) * 3 + tg) * 64];
    const float *p = base + (4 * s) * PL;
#pragma unroll
    for (int ro = 0; ro < NR + 2; ++ro)
#pragma unroll
        for (int dxi = 0; dxi < 3; ++dxi) f.b[ro][dxi] = p[ro * kRowW + dxi];
}

template <int TM, int NR>
__device__ __forceinline__ void mfma_group(const Frags<TM, NR> &f, f32x4 (&acc)[TM][8]) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int dyi = tap / 3, dxi = tap % 3;
#pragma unroll
        for (int m = 0; m < TM; ++m) {
            const float av = f.a[m][tap / 4][tap % 4];
#pragma unroll
            for (int t = 0; t < NR; ++t)
                acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, f.b[t + dyi][dxi], acc[m][t], 0, 0, 0);
        }
    }
}

// acc[m][t] += W(tile tile0+m) x in(rows row0+t) over all CIN input channels and the 9 taps.
// Software pipelined: the fragments of channel group s+1 are fetched (weights: 16-byte loads
// from L2, activations: ds_read_b32) while the 9*TM*NR MFMAs of group s issue.
template <int PL, int CIN, int TM, int NR>
__device__ __forceinline__ void conv_accumulate(const float *__restrict__ in, const f32x4 *__restrict__ wp,
                                                int tile0, int row0, int lane, f32x4 (&acc)[TM][8]) {
    constexpr int kSteps = CIN / 4;
    const int x = lane & 15, kq = lane >> 4;
    const float *base = in + kq * PL + row0 * kRowW + x;  // in[(4s+kq)][row0 + ro][x + dxi]
    const f32x4 *wbase = wp + (size_t)tile0 * kSteps * 3 * 64 + lane;
    Frags<TM, NR> f0, f1;
    load_frags<PL, TM, NR, kSteps>(f0, base, wbase, 0);
#pragma unroll 1
    // sched_barrier(0) pins "issue every load of the next group, THEN the MFMAs of this one":
    // left alone, hipcc sinks each load next to its first use and the MFMAs wait on it.
    for (int s = 0; s < kSteps; s += 2) {
        load_frags<PL, TM, NR, kSteps>(f1, base, wbase, s + 1 < kSteps ? s + 1 : kSteps - 1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_group<TM, NR>(f0, acc);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (kSteps > 1) {  // kSteps is 1 (conv1) or even
            load_frags<PL, TM, NR, kSteps>(f0, base, wbase, s + 2 < kSteps ? s + 2 : kSteps - 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_group<TM, NR>(f1, acc);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <int PL, int CIN, int TM>
__device__ __forceinline__ void conv_rows(const float *__restrict__ in, const f32x4 *__restrict__ wp, int tile0,
                                          int row0, int n_rows, int lane, f32x4 (&acc)[TM][8]) {
    if (n_rows == 7) conv_accumulate<PL, CIN, TM, 7>(in, wp, tile0, row0, lane, acc);
    else conv_accumulate<PL, CIN, TM, 8>(in, wp, tile0, row0, lane, acc);
}

// out[cout][y+1][x+1] = relu(acc + bias[cout]) for the lane's 4 channels of every tile/row.
template <int PL, int TM>
__device__ __forceinline__ void store_relu(float *__restrict__ out, const float *__restrict__ bias, int tile0,
                                           int row0, int lane, int BH, int BW, const f32x4 (&acc)[TM][8],
                                           int n_rows = 8) {
    const int x = lane & 15, q = lane >> 4;
    if (x >= BW) return;
#pragma unroll
    for (int m = 0; m < TM; ++m) {
        const int c0 = (tile0 + m) * 16 + 4 * q;
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + c0);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int y = row0 + t;
            if (y >= BH || t >= n_rows) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                out[(c0 + j) * PL + (y + 1) * kRowW + (x + 1)] = fmaxf(acc[m][t][j] + bv[j], 0.0f);
        }
    }
}

template <int TM>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[TM][8]) {
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// helpers shared by the Winograd F(4x4,3x3) trunk
typedef const __attribute__((address_space(3))) float *lds_cptr;
typedef int i32x4 __attribute__((ext_vector_type(4)));

// U fragment load: buffer addressing = scalar resource + the lane's 32-bit offset + a scalar byte
// offset, so the address of every load of the stream costs SALU only.
__device__ __forceinline__ f32x4 load_u(__amdgpu_buffer_rsrc_t rsrc, int lane_off, int uniform_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_off, uniform_off, 0));
}

// =====================================================================================================
// Winograd F(4x4,3x3) trunk (RZ_NET_WINOGRAD_F4): 36 element-wise products per 4x4 output tile instead of
// 144 multiply-adds -- 4x fewer MFMAs than the direct form, 1.78x fewer than F(2x2,3x3).  fp32
// throughout; the larger transform constants cost about one decimal digit (|error| ~1e-6 on the conv3
// activations against fp64, ~5e-7 on the log-probabilities: tests/test_gpu_parity.py).
//   * the MFMA N dimension is the WHOLE board: 16 tiles of 4x4 outputs (lane & 15 = 4*ty + tx); K = input
//     channels (4 per step, lane >> 4); M = 16 output channels;
//   * 4 waves per workgroup, one per SIMD (up to 512 registers): a wave owns TM output-channel tiles (conv3: 2,
//     conv2: 1) and ALL 36 components, taken in 3 passes over the channel groups, two transform rows (12
//     components) per pass -- {1,2}, {3,4}, {0,5} -- so 12*TM accumulators are live, and each pass folds
//     its rows into the 4x4 outputs (the output transform A^T M A is linear in M);
//   * per channel group a lane reads its 6x6 input patch rows from the halo planes (4 rows for the
//     first two passes, 6 for the last), forms the 12 transformed values (row stage then column stage,
//     52..64 fused multiply-adds) and issues 12*TM MFMAs against U fragments streamed from L2 with buffer
//     loads; the software pipeline of wino_block is kept: the transform of group g+1, the LDS reads of
//     g+2 and the U loads of g+3 are threaded between the MFMAs of group g.
namespace f4 {

// Everything below is indexed by template parameters and expanded with fold expressions (not loops the
// unroller may decline to unroll: the op lists are long), so every register-array index is a constant.

template <int P> struct Pass {  // pass P handles transform rows i' = a, b
    static constexpr int a = (P == 0) ? 1 : (P == 1) ? 3 : 0;
    static constexpr int b = (P == 0) ? 2 : (P == 1) ? 4 : 5;
    static constexpr int first = (P == 2) ? 0 : 1;   // patch rows it reads: 1..4, or all six for rows 0 / 5
    static constexpr int count = (P == 2) ? 6 : 4;
    static constexpr int n_ld = 3 * count;           // ds_read2 per group
    static constexpr int row_ops = (P == 2) ? 4 : 3; // row-stage instructions per patch column
    static constexpr int n_xf = 6 * row_ops + 14;    // transform instructions per group (packed: 2 floats each)
};

// LDS read O of a group of pass P: patch row first + O / 3, column pair O % 3
template <int P, int O>
__device__ __forceinline__ void ld_op(float (&d)[6][6], lds_cptr q) {
    constexpr int row = Pass<P>::first + O / 3, c = 2 * (O % 3);
    d[row][c] = q[row * kRowW + c];
    d[row][c + 1] = q[row * kRowW + c + 1];
}

// Transform instruction O of a group of pass P; every case is ONE instruction, most of them PACKED fp32
// (v_pk_add_f32 / v_pk_fma_f32 on register pairs, with half selects / negations as operand modifiers):
// the two transform rows a, b of the pass go through identical arithmetic, so the pair (row a, row b) is
// the natural vector.  Row stage, column by column: t[c] = (rows a, b of B^T d)[c]; then the column stage
// v[j'] = (t B)[j'] on those pairs,
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1].
template <int P, int O>
__device__ __forceinline__ void xf_op(const float (&d)[6][6], f32x2 (&w)[2], f32x2 (&t)[6], f32x2 (&u)[8], f32x2 (&v)[6]) {
    constexpr int kRowOps = Pass<P>::row_ops;
    if constexpr (O < 6 * kRowOps) {
        constexpr int c = O / kRowOps, k = O % kRowOps;
        if constexpr (P == 0) {  // rows 1, 2: -4 (d1 + d2) + (d3 + d4) ; 4 (d1 - d2) - (d3 - d4)
            if constexpr (k == 0) w[0] = f32x2{d[1][c], d[1][c]} + f32x2{d[2][c], -d[2][c]};
            else if constexpr (k == 1) w[1] = f32x2{d[4][c], d[4][c]} + f32x2{d[3][c], -d[3][c]};
            else t[c] = __builtin_elementwise_fma(f32x2{-4.0f, 4.0f}, w[0], w[1]);
        } else if constexpr (P == 1) {  // rows 3, 4: +-2 (d3 - d1) + (d4 - d2)
            if constexpr (k == 0) w[0].x = d[3][c] - d[1][c];
            else if constexpr (k == 1) w[0].y = d[4][c] - d[2][c];
            else t[c] = __builtin_elementwise_fma(f32x2{2.0f, -2.0f}, f32x2{w[0].x, w[0].x}, f32x2{w[0].y, w[0].y});
        } else {  // rows 0, 5: 4 d0 - 5 d2 + d4 ; 4 d1 - 5 d3 + d5
            if constexpr (k == 0) w[0].x = fmaf(-5.0f, d[2][c], d[4][c]);
            else if constexpr (k == 1) t[c].x = fmaf(4.0f, d[0][c], w[0].x);
            else if constexpr (k == 2) w[0].y = fmaf(-5.0f, d[3][c], d[5][c]);
            else t[c].y = fmaf(4.0f, d[1][c], w[0].y);
        }
    } else {
        constexpr int k = O - 6 * kRowOps;
        const f32x2 c4 = {4.0f, 4.0f}, c2 = {2.0f, 2.0f}, c5 = {-5.0f, -5.0f};
        if constexpr (k == 0) u[0] = t[1] + t[2];
        else if constexpr (k == 1) u[1] = t[3] + t[4];
        else if constexpr (k == 2) u[2] = t[1] - t[2];
        else if constexpr (k == 3) u[3] = t[3] - t[4];
        else if constexpr (k == 4) v[1] = __builtin_elementwise_fma(-c4, u[0], u[1]);
        else if constexpr (k == 5) v[2] = __builtin_elementwise_fma(c4, u[2], -u[3]);
        else if constexpr (k == 6) u[4] = t[3] - t[1];
        else if constexpr (k == 7) u[5] = t[4] - t[2];
        else if constexpr (k == 8) v[3] = __builtin_elementwise_fma(c2, u[4], u[5]);
        else if constexpr (k == 9) v[4] = __builtin_elementwise_fma(-c2, u[4], u[5]);
        else if constexpr (k == 10) u[6] = __builtin_elementwise_fma(c5, t[2], t[4]);
        else if constexpr (k == 11) v[0] = __builtin_elementwise_fma(c4, t[0], u[6]);
        else if constexpr (k == 12) u[7] = __builtin_elementwise_fma(c5, t[3], t[5]);
        else v[5] = __builtin_elementwise_fma(c4, t[1], u[7]);
    }
}
template <int P, int BASE, int... Os>
__device__ __forceinline__ void xf_ops(std::integer_sequence<int, Os...>, const float (&d)[6][6], f32x2 (&w)[2],
                                       f32x2 (&t)[6], f32x2 (&u)[8], f32x2 (&v)[6]) {
    (xf_op<P, BASE + Os>(d, w, t, u, v), ...);
}
template <int P, int BASE, int... Os>
__device__ __forceinline__ void ld_ops(std::integer_sequence<int, Os...>, float (&d)[6][6], lds_cptr q) {
    (ld_op<P, BASE + Os>(d, q), ...);
}

// Slot I of the MFMA block of one channel group: MFMA I (component k = I / TM = rr*6 + j', tile m = I % TM) and its
// slice of the next groups' work: first third of the slots = LDS reads of the group two ahead (pass LP) into
// d_ld and the U loads two groups ahead; the other two thirds = transform of the next group (pass XP), whose
// patch rows d_xf were fetched during the PREVIOUS block (the patch buffer is double buffered: with one wave
// per SIMD nothing else covers the LDS latency), into v_nxt.
template <int TM, int XP, int LP, int I>
__device__ __forceinline__ void slot(f32x4 (&acc)[TM][12], const f32x4 (&a_cur)[TM][3], const f32x2 (&v_cur)[6],
                                     f32x2 (&v_nxt)[6], const float (&d_xf)[6][6], float (&d_ld)[6][6], f32x2 (&w)[2],
                                     f32x2 (&t)[6], f32x2 (&u)[8], lds_cptr q_ld, f32x4 (&a_ld)[TM][3],
                                     __amdgpu_buffer_rsrc_t u_rsrc, int u_off, int u_lane, int u_stride) {
    constexpr int NS = 12 * TM, LD_SLOTS = NS / 3, XF_SLOTS = NS - LD_SLOTS;
    constexpr int kXf = Pass<XP>::n_xf, kLd = Pass<LP>::n_ld;
    constexpr int XF_PER = (kXf + XF_SLOTS - 1) / XF_SLOTS, LD_PER = (kLd + LD_SLOTS - 1) / LD_SLOTS;
    constexpr int k = I / TM, m = I % TM;
    // In-place accumulation on accumulation registers, written as inline assembly: with more than 256
    // registers per wave the compiler otherwise stages every accumulator through a[0:3] and copies it to
    // and from ordinary registers around each MFMA (8 extra instructions per MFMA).  No hazard handling is
    // lost: consecutive MFMAs use different accumulators (the same one recurs 12*TM MFMAs later) and the
    // operands were produced in the previous block; the fold waits explicitly.
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0"
                 : "+a"(acc[m][k])
                 : "v"(a_cur[m][k >> 2][k & 3]), "v"(v_cur[k % 6][k / 6]));
    if constexpr (I < LD_SLOTS) {
        constexpr int lo = I * LD_PER, hi = (lo + LD_PER < kLd) ? lo + LD_PER : kLd;
        if constexpr (hi > lo) ld_ops<LP, lo>(std::make_integer_sequence<int, hi - lo>{}, d_ld, q_ld);
        if constexpr (I < 3) {
#pragma unroll
            for (int m2 = 0; m2 < TM; ++m2) a_ld[m2][I] = load_u(u_rsrc, u_lane, u_off + m2 * u_stride + I * 1024);
        }
    } else {
        constexpr int j = I - LD_SLOTS;
        constexpr int lo = j * XF_PER, hi = (lo + XF_PER < kXf) ? lo + XF_PER : kXf;
        if constexpr (hi > lo) xf_ops<XP, lo>(std::make_integer_sequence<int, hi - lo>{}, d_xf, w, t, u, v_nxt);
    }
    __builtin_amdgcn_sched_barrier(0);
}
template <int TM, int XP, int LP, int... Is>
__device__ __forceinline__ void block(std::integer_sequence<int, Is...>, f32x4 (&acc)[TM][12], const f32x4 (&a_cur)[TM][3],
                                      const f32x2 (&v_cur)[6], f32x2 (&v_nxt)[6], const float (&d_xf)[6][6],
                                      float (&d_ld)[6][6], lds_cptr q_ld, f32x4 (&a_ld)[TM][3],
                                      __amdgpu_buffer_rsrc_t u_rsrc, int u_off, int u_lane, int u_stride) {
    f32x2 w[2], t[6], u[8];
    (slot<TM, XP, LP, Is>(acc, a_cur, v_cur, v_nxt, d_xf, d_ld, w, t, u, q_ld, a_ld, u_rsrc, u_off, u_lane, u_stride), ...);
}

// output transform of one transform row: w[q] = sum_j' A^T[q][j'] M[j'],  A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0;
// 0 1 1 4 4 0; 0 1 -1 8 -8 1]
__device__ __forceinline__ void out_row(const f32x4 *M, f32x4 (&w)[4]) {
    const f32x4 s12 = M[1] + M[2], d12 = M[1] - M[2], s34 = M[3] + M[4], d34 = M[3] - M[4];
    w[0] = M[0] + s12 + s34;
    w[1] = d12 + 2.0f * d34;
    w[2] = s12 + 4.0f * s34;
    w[3] = d12 + 8.0f * d34 + M[5];
}

template <int CIN, int TM>
__device__ __forceinline__ void preload_u(const f32x4 *__restrict__ up, int tile0, int lane, f32x4 (&a)[4][TM][3]) {
    constexpr int kSteps = CIN / 4, kG = 3 * 1024, kUStride = 3 * kSteps * kG;
    const __amdgpu_buffer_rsrc_t u_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<f32x4 *>(up), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                a[g][m][j] = load_u(u_rsrc, lane * 16, tile0 * kUStride + m * kUStride + g * kG + j * 1024);
}

// One pass (transform rows Pass<P>::a, b) over the kSteps channel groups.  Linear group index g = P*kSteps + s;
// block g multiplies group g, transforms g+1, reads the patch of g+2 and loads the U fragments of g+2 -- at the end
// of the pass those belong to pass P+1 (after the last pass the indices are clamped: fetched again, unused).
template <int PL, int CIN, int TM, int P>
__device__ __forceinline__ void pass(lds_cptr base, __amdgpu_buffer_rsrc_t u_rsrc, int ubase, int u_lane,
                                     f32x4 (&a)[4][TM][3], float (&d)[2][6][6], f32x2 (&vb)[2][6], f32x4 (&Y)[TM][16]) {
    constexpr int kSteps = CIN / 4, kGroups = 3 * kSteps, kG = 3 * 1024, kUStride = 3 * kSteps * kG;
    constexpr int NP = P < 2 ? P + 1 : 2;
    constexpr auto seq = std::make_integer_sequence<int, 12 * TM>{};
    f32x4 acc[TM][12];
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int k = 0; k < 12; ++k) acc[m][k] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the compiler cannot see that the assembly below is an MFMA reading these registers as its C operand:
    // ALL clearing writes are forced to precede this point (every accumulator is an operand) and the required
    // distance to the first MFMA is kept by hand
    if constexpr (TM == 1) asm volatile("s_nop 15" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[0][4]), "+a"(acc[0][5]), "+a"(acc[0][6]), "+a"(acc[0][7]), "+a"(acc[0][8]), "+a"(acc[0][9]), "+a"(acc[0][10]), "+a"(acc[0][11]));
    else asm volatile("s_nop 15" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[0][4]), "+a"(acc[0][5]), "+a"(acc[0][6]), "+a"(acc[0][7]), "+a"(acc[0][8]), "+a"(acc[0][9]), "+a"(acc[0][10]), "+a"(acc[0][11]), "+a"(acc[1][0]), "+a"(acc[1][1]), "+a"(acc[1][2]), "+a"(acc[1][3]), "+a"(acc[1][4]), "+a"(acc[1][5]), "+a"(acc[1][6]), "+a"(acc[1][7]), "+a"(acc[1][8]), "+a"(acc[1][9]), "+a"(acc[1][10]), "+a"(acc[1][11]));
    auto patch = [&](int g2) {  // LDS base of group g2's patch, opaque so that the reads use immediate offsets
        lds_cptr q = base + (4 * (g2 % kSteps)) * PL;
        asm volatile("" : "+v"(q));
        return q;
    };
#pragma unroll 1
    for (int s0 = 0; s0 < kSteps - 4; s0 += 4) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int g2 = P * kSteps + s0 + r + 2;
            block<TM, P, P>(seq, acc, a[r], vb[r & 1], vb[(r + 1) & 1], d[(r + 1) & 1], d[r & 1], patch(g2), a[(r + 2) & 3],
                            u_rsrc, ubase + g2 * kG, u_lane, kUStride);
        }
    }
    {   // last four groups of the pass
        constexpr int g0 = P * kSteps + kSteps - 4;
        constexpr int c2 = (g0 + 4 < kGroups) ? g0 + 4 : kGroups - 1, c3 = (g0 + 5 < kGroups) ? g0 + 5 : kGroups - 1;
        block<TM, P, P>(seq, acc, a[0], vb[0], vb[1], d[1], d[0], patch(g0 + 2), a[2], u_rsrc, ubase + (g0 + 2) * kG, u_lane,
                        kUStride);
        block<TM, P, P>(seq, acc, a[1], vb[1], vb[0], d[0], d[1], patch(g0 + 3), a[3], u_rsrc, ubase + (g0 + 3) * kG, u_lane,
                        kUStride);
        block<TM, P, NP>(seq, acc, a[2], vb[0], vb[1], d[1], d[0], patch(c2), a[0], u_rsrc, ubase + c2 * kG, u_lane, kUStride);
        block<TM, NP, NP>(seq, acc, a[3], vb[1], vb[0], d[0], d[1], patch(c3), a[1], u_rsrc, ubase + c3 * kG, u_lane, kUStride);
    }
    // the last MFMAs (8 passes = 32 cycles) must have left the matrix pipe before the fold reads them
    // (every accumulator is an operand, so no read of one can be moved above the wait)
    if constexpr (TM == 1) asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[0][4]), "+a"(acc[0][5]), "+a"(acc[0][6]), "+a"(acc[0][7]), "+a"(acc[0][8]), "+a"(acc[0][9]), "+a"(acc[0][10]), "+a"(acc[0][11]));
    else asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[0][4]), "+a"(acc[0][5]), "+a"(acc[0][6]), "+a"(acc[0][7]), "+a"(acc[0][8]), "+a"(acc[0][9]), "+a"(acc[0][10]), "+a"(acc[0][11]), "+a"(acc[1][0]), "+a"(acc[1][1]), "+a"(acc[1][2]), "+a"(acc[1][3]), "+a"(acc[1][4]), "+a"(acc[1][5]), "+a"(acc[1][6]), "+a"(acc[1][7]), "+a"(acc[1][8]), "+a"(acc[1][9]), "+a"(acc[1][10]), "+a"(acc[1][11]));
    // fold: Y[p][q] (+)= A^T[p][i'] w_i'[q]; columns of A^T: i'=1: 1 1 1 1, 2: 1 -1 1 -1, 3: 1 2 4 8,
    // 4: 1 -2 4 -8, 0: 1 0 0 0, 5: 0 0 0 1.  Pass 0 writes Y for the first time.
#pragma unroll
    for (int m = 0; m < TM; ++m) {
        f32x4 wa[4], wb[4];
        out_row(&acc[m][0], wa);
        out_row(&acc[m][6], wb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (P == 0) {
                const f32x4 sum = wa[q] + wb[q], dif = wa[q] - wb[q];
                Y[m][0 + q] = sum;
                Y[m][4 + q] = dif;
                Y[m][8 + q] = sum;
                Y[m][12 + q] = dif;
            } else if constexpr (P == 1) {
                const f32x4 sum = wa[q] + wb[q], dif = wa[q] - wb[q];
                Y[m][0 + q] += sum;
                Y[m][4 + q] += 2.0f * dif;
                Y[m][8 + q] += 4.0f * sum;
                Y[m][12 + q] += 8.0f * dif;
            } else {
                Y[m][0 + q] += wa[q];
                Y[m][12 + q] += wb[q];
            }
        }
    }
}

// Y[m][p*4 + q] = conv output (no bias) of output-channel tile tile0 + m at board row 4*ty + p, column 4*tx + q
// (ty = (lane >> 2) & 3, tx = lane & 3) for the lane's 4 channels.
template <int PL, int CIN, int TM>
__device__ __forceinline__ void conv(const float *__restrict__ in, const f32x4 *__restrict__ up, int tile0, int lane,
                                     f32x4 (&a)[4][TM][3], f32x4 (&Y)[TM][16]) {
    constexpr int kSteps = CIN / 4, kG = 3 * 1024, kUStride = 3 * kSteps * kG;
    const int kq = lane >> 4, ty = (lane >> 2) & 3, tx = lane & 3;
    // top-left of the lane's 6x6 patch in halo coordinates: row 4*ty, column 4*tx, plane kq of the group
    const lds_cptr base = (lds_cptr)(in + kq * PL + (4 * ty) * kRowW + 4 * tx);
    const __amdgpu_buffer_rsrc_t u_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<f32x4 *>(up), 0, 0x7fffffff, 0x00020000);
    const int ubase = tile0 * kUStride, u_lane = lane * 16;
    float d[2][6][6];  // patch rows, double buffered: a group's rows are read one block before they are transformed
    f32x2 vb[2][6];    // transformed fragment, double buffered: vb[.][j'] = (row a, row b) of column j'
    {   // pipeline prologue: group 0 transformed, patch rows of group 1 in flight
        f32x2 w[2], t[6], u[8];
        ld_ops<0, 0>(std::make_integer_sequence<int, Pass<0>::n_ld>{}, d[0], base);
        ld_ops<0, 0>(std::make_integer_sequence<int, Pass<0>::n_ld>{}, d[1], base + 4 * PL);
        xf_ops<0, 0>(std::make_integer_sequence<int, Pass<0>::n_xf>{}, d[0], w, t, u, vb[0]);
        __builtin_amdgcn_sched_barrier(0);
    }
    pass<PL, CIN, TM, 0>(base, u_rsrc, ubase, u_lane, a, d, vb, Y);
    pass<PL, CIN, TM, 1>(base, u_rsrc, ubase, u_lane, a, d, vb, Y);
    pass<PL, CIN, TM, 2>(base, u_rsrc, ubase, u_lane, a, d, vb, Y);
}

}  // namespace f4

// W waves per workgroup: wave w owns the 8 / W output-channel tiles {w*8/W ..} of conv3 for the whole board;
// conv2 (4 tiles) runs on waves 0..3.
//   W = 4 (default): two tiles per wave, one wave per SIMD with up to 512 registers.  A wave does not overlap
//     its own MFMAs with its own vector work (measured: time = MFMA + VALU), so the transform is exposed --
//     but it is done once per SIMD.
//   W = 8: one tile per wave, two waves per SIMD (<= 256 registers each, spills) that do overlap -- but every
//     wave forms the transformed input of the whole board itself, and the doubled vector work makes it 40 %
//     slower than W = 4 (kept selectable as RZ_NET_WINOGRAD_F4_8W).
// Persistent workgroups, LDS layout, conv1, observation prefetch and the feature epilogue as in k_trunk_wino.
template <int W>
__global__ __launch_bounds__(64 * W) void k_trunk_wino_f4(NetDev nd, const float *__restrict__ obs,
                                                          float *__restrict__ feat, int n_boards) {
    constexpr int PL = kPlaneWino;
    constexpr int kLdsFloats = kPlanes * PL;
    constexpr int kThreads = 64 * W;
    constexpr int TM3 = 8 / W;
    constexpr int kPartialFloats = 4 * 6 * 256;
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats + kPartialFloats];
    float *in0 = lds;
    float *c1 = in0 + kPlanesIn * PL;
    float *c2 = c1 + kPlanesC1 * PL;
    float *partial = c2 + kPlanesC2 * PL;  // [wave][o][y][x]
    const int tid0 = threadIdx.x;
    const int BH = nd.BH, BW = nd.BW, S = nd.S;
    {
        f32x4 *z = reinterpret_cast<f32x4 *>(lds);
        for (int i = tid0; i < kLdsFloats / 4; i += kThreads) z[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
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
    // element tid + k*kThreads of a board's observation planes / head features -> where it lives in LDS /
    // in the feature row: the same for every board, so the integer divisions are done once per thread
    int obs_off[kObsPer];
#pragma unroll
    for (int k = 0; k < kObsPer; ++k) {
        const int i = tid0 + k * kThreads;
        const int c = i / S, r = i - c * S, y = r / BW, x = r - y * BW;
        obs_off[k] = i < 4 * S ? c * PL + (y + 1) * kRowW + (x + 1) : -1;
    }
    constexpr int kFeatPer = (6 * RZ_MAX_BOARD_SIZE * RZ_MAX_BOARD_SIZE + kThreads - 1) / kThreads;
    int feat_src[kFeatPer], feat_dst[kFeatPer];
    float feat_bias[kFeatPer];
#pragma unroll
    for (int k = 0; k < kFeatPer; ++k) {
        const int i = tid0 + k * kThreads;
        const int o = i / S, r = i - o * S, y = r / BW, x = r - y * BW;
        feat_src[k] = (o * 16 + y) * 16 + x;
        feat_dst[k] = i < 6 * S ? (i < 4 * S ? i : i - 4 * S + nd.feat_val_off) : -1;
        feat_bias[k] = i < 6 * S ? nd.bh[o] : 0.0f;
    }
    auto store_obs = [&](int) {
#pragma unroll
        for (int k = 0; k < kObsPer; ++k)
            if (obs_off[k] >= 0) in0[obs_off[k]] = ob[k];
    };
    __syncthreads();
    if ((int)blockIdx.x < n_boards) {
        load_obs(blockIdx.x, tid0);
        store_obs(tid0);
    }
    __syncthreads();
    for (int board = blockIdx.x; board < n_boards; board += gridDim.x) {
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int next_board = board + (int)gridDim.x;
    {   // conv1: 4 -> 32 direct: output tile (wave & 1), board rows (32 / W) * (wave >> 1) ..
        constexpr int kRowsPer = 32 / W;
        const int tile = wave & 1, row0 = kRowsPer * (wave >> 1);
        if (row0 < BH) {
            f32x4 acc[1][8];
            zero_acc<1>(acc);
            if (kRowsPer == 4) conv_accumulate<PL, 4, 1, 4>(in0, nd.w1, tile, row0, lane, acc);
            else conv_rows<PL, 4, 1>(in0, nd.w1, tile, row0, (BH - row0 == 7) ? 7 : 8, lane, acc);
            store_relu<PL, 1>(c1, nd.b1, tile, row0, lane, BH, BW, acc, kRowsPer);
        }
    }
    __syncthreads();
    if (next_board < n_boards) load_obs(next_board, tid);
    const int q = lane >> 4, ty = (lane >> 2) & 3, tx = lane & 3;
    if (wave < 4) {  // conv2: 32 -> 64, one output-channel tile per wave (waves 0..3)
        f32x4 a2[4][1][3];
        f32x4 Y[1][16];
        f4::preload_u<32, 1>(nd.u2f, wave, lane, a2);
        f4::conv<PL, 32, 1>(c1, nd.u2f, wave, lane, a2, Y);
        const int c0 = wave * 16 + 4 * q;
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(nd.b2 + c0);
#pragma unroll
        for (int pq = 0; pq < 16; ++pq) {
            const int y = 4 * ty + (pq >> 2), x = 4 * tx + (pq & 3);
            if (y < BH && x < BW) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    c2[(c0 + j) * PL + (y + 1) * kRowW + (x + 1)] = fmaxf(Y[0][pq][j] + bv[j], 0.0f);
            }
        }
    }
    if (next_board < n_boards) store_obs(tid);
    __syncthreads();
    {   // conv3: 64 -> 128, TM3 tiles per wave; the ReLU'd output feeds the two 1x1 head convolutions
        // head partial sums, packed in pairs of outputs (o, o+1): index pos*3 + o/2, pos = p*4 + q
        f32x2 vals2[48];
#pragma unroll
        for (int i = 0; i < 48; ++i) vals2[i] = f32x2{0.0f, 0.0f};
        {
            f32x4 Y[TM3][16];
            f32x4 a3[4][TM3][3];
            f4::preload_u<64, TM3>(nd.u3f, TM3 * wave, lane, a3);
            f4::conv<PL, 64, TM3>(c2, nd.u3f, TM3 * wave, lane, a3, Y);
#pragma unroll
            for (int m = 0; m < TM3; ++m) {
                const int c0 = (TM3 * wave + m) * 16 + 4 * q;
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(nd.b3 + c0);
                f32x4 wv[6];
#pragma unroll
                for (int o = 0; o < 6; ++o) wv[o] = *reinterpret_cast<const f32x4 *>(nd.wh + o * 128 + c0);
#pragma unroll
                for (int pq = 0; pq < 16; ++pq)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float hv = fmaxf(Y[m][pq][j] + bv[j], 0.0f);
#pragma unroll
                        for (int o2 = 0; o2 < 3; ++o2)  // one v_pk_fma_f32 per pair of head outputs
                            vals2[pq * 3 + o2] = __builtin_elementwise_fma(f32x2{wv[2 * o2][j], wv[2 * o2 + 1][j]},
                                                                           f32x2{hv, hv}, vals2[pq * 3 + o2]);
                    }
            }
        }
        float vals[96];
#pragma unroll
        for (int i = 0; i < 96; ++i) vals[i] = vals2[i >> 1][i & 1];
        float sums[24];
        f4::reduce_scatter_96(vals, sums);
        // partial sums of the waves: [wave & 3][o][y][x]; with 8 waves, wave w + 4 stores first and wave w adds
        // its own on top (fixed order: the result does not depend on timing)
        const int off = (q & 1) * 48 + (q >> 1) * 24;
        if (W == 4 || wave >= 4) {
#pragma unroll
            for (int i = 0; i < 24; ++i) {
                const int vi = off + i, pq = vi / 6, o = vi - 6 * pq;
                const int y = 4 * ty + (pq >> 2), x = 4 * tx + (pq & 3);
                partial[(((wave & 3) * 6 + o) * 16 + y) * 16 + x] = sums[i];
            }
        }
        if (W == 8) {
            __syncthreads();
            if (wave < 4) {
#pragma unroll
                for (int i = 0; i < 24; ++i) {
                    const int vi = off + i, pq = vi / 6, o = vi - 6 * pq;
                    const int y = 4 * ty + (pq >> 2), x = 4 * tx + (pq & 3);
                    partial[((wave * 6 + o) * 16 + y) * 16 + x] += sums[i];
                }
            }
        }
    }
    __syncthreads();
    {
        float *dst = feat + (size_t)board * nd.feat_ld;
#pragma unroll
        for (int k = 0; k < kFeatPer; ++k) {
            if (feat_dst[k] < 0) continue;
            float v = feat_bias[k];
#pragma unroll
            for (int g = 0; g < 4; ++g) v += partial[g * 6 * 256 + feat_src[k]];
            dst[feat_dst[k]] = fmaxf(v, 0.0f);
        }
    }
    }  // boards
}

// Direct path: wave w = 4*rh + q4 owns output-channel quarter q4 (the two waves of a quarter share
// a SIMD, waves are dealt to SIMDs cyclically) and row half rh (rows 0-7 / 8-15; on a 15x15 board
// the second half computes 7 rows, so every SIMD carries exactly 15 row-units of each layer).
__global__ __launch_bounds__(kTrunkThreads) void k_trunk(NetDev nd, const float *__restrict__ obs,
                                                         float *__restrict__ feat, int n_boards) {
    constexpr int PL = kPlaneDirect;
    constexpr int kLdsFloats = kPlanes * PL;  // 131.25 KiB
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    float *in0 = lds;
    float *c1 = in0 + kPlanesIn * PL;
    float *c2 = c1 + kPlanesC1 * PL;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q4 = wave & 3, rh = wave >> 2;
    const int BH = nd.BH, BW = nd.BW, S = nd.S;
    const int board = blockIdx.x;
    if (board >= n_boards) return;
    const int row0 = 8 * rh;
    const int n_rows = (BH - row0 == 7) ? 7 : 8;
    const bool busy = row0 < BH;  // a wave whose rows are all outside the board only hits barriers

    // zero the halo planes (interiors are overwritten below), then stage the observation
    {
        f32x4 *z = reinterpret_cast<f32x4 *>(lds);
        for (int i = tid; i < kLdsFloats / 4; i += kTrunkThreads) z[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    {
        const float *src = obs + (size_t)board * 4 * S;
        for (int i = tid; i < 4 * S; i += kTrunkThreads) {
            const int c = i / S, r = i - c * S, y = r / BW, x = r - y * BW;
            in0[c * PL + (y + 1) * kRowW + (x + 1)] = src[i];
        }
    }
    __syncthreads();

    if (busy && q4 < 2) {   // conv1: 4 -> 32 = two 16-channel tiles
        f32x4 acc[1][8];
        zero_acc<1>(acc);
        conv_rows<PL, 4, 1>(in0, nd.w1, q4, row0, n_rows, lane, acc);
        store_relu<PL, 1>(c1, nd.b1, q4, row0, lane, BH, BW, acc);
    }
    __syncthreads();
    if (busy) {   // conv2: 32 -> 64 = one tile per quarter
        f32x4 acc[1][8];
        zero_acc<1>(acc);
        conv_rows<PL, 32, 1>(c1, nd.w2, q4, row0, n_rows, lane, acc);
        store_relu<PL, 1>(c2, nd.b2, q4, row0, lane, BH, BW, acc);
    }
    __syncthreads();
    // conv3: 64 -> 128 (two tiles per quarter), kept in registers and fed to the 1x1 head convs
    float part[8][6];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int o = 0; o < 6; ++o) part[t][o] = 0.0f;
    if (busy) {
        const int q = lane >> 4;
        f32x4 acc[2][8];
        zero_acc<2>(acc);
        conv_rows<PL, 64, 2>(c2, nd.w3, 2 * q4, row0, n_rows, lane, acc);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int c0 = (2 * q4 + m) * 16 + 4 * q;
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(nd.b3 + c0);
            f32x4 wv[6];
#pragma unroll
            for (int o = 0; o < 6; ++o) wv[o] = *reinterpret_cast<const f32x4 *>(nd.wh + o * 128 + c0);
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float hv = fmaxf(acc[m][t][j] + bv[j], 0.0f);
#pragma unroll
                    for (int o = 0; o < 6; ++o) part[t][o] = fmaf(wv[o][j], hv, part[t][o]);
                }
        }
    }
    // sum over the 4 channel sub-groups held by lanes x, x+16, x+32, x+48
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int o = 0; o < 6; ++o) {
            float v = part[t][o];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            part[t][o] = v;
        }
    float *partial = c1;  // [q4][o][y][x]: c1 is free now
    if (lane < 16) {
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int o = 0; o < 6; ++o) partial[((q4 * 6 + o) * 16 + (row0 + t)) * 16 + lane] = part[t][o];
    }
    __syncthreads();
    {
        float *dst = feat + (size_t)board * nd.feat_ld;
        for (int i = tid; i < 6 * S; i += kTrunkThreads) {
            const int o = i / S, r = i - o * S, y = r / BW, x = r - y * BW;
            float v = nd.bh[o];
#pragma unroll
            for (int k = 0; k < 4; ++k) v += partial[((k * 6 + o) * 16 + y) * 16 + x];
            dst[i < 4 * S ? i : i - 4 * S + nd.feat_val_off] = fmaxf(v, 0.0f);
        }
    }
}

// ------------------------------------------------------------------ heads (FC layers)
// k_heads_gemm: the two first FC layers as ONE fp32-MFMA GEMM: M = boards, N = outputs (policy
// logits padded to a multiple of 32, then the 64 hidden units of the value head), K = 4S (policy) /
// 2S (value), both padded to multiples of 16.  One workgroup per (32 boards) x (32 outputs); its 4
// waves split K and each accumulates the whole 2 x 2 block of 16 x 16 tiles over its slice, so a
// fragment pair feeds four independent MFMA chains.  Operands stream straight from L2 in their
// natural row-major layouts: lane (row r, quarter q) loads 16 bytes = k 16g + 4q .. + 3 of its row,
// the 4 values being the lane's operand of the 4 MFMA steps of group g (the order in which K is
// consumed is free as long as both operands agree).  A ring of kHeadDepth groups is kept in flight.
// The 4 partial blocks are summed through LDS.  k_heads_finish: log_softmax / fc2 + tanh.
constexpr int kHeadDepth = 4;
constexpr int kHeadWaves = 4;  // K split

__global__ __launch_bounds__(64 * kHeadWaves) void k_heads_gemm(NetDev nd, const float *__restrict__ feat,
                                                    float *__restrict__ raw, float *__restrict__ hid,
                                                    int n_boards) {
    __shared__ f32x4 part[kHeadWaves][4][64];
    __builtin_amdgcn_s_setprio(3);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * 32;
    const int n_act_tiles = nd.Npad / 32;
    const int ot = blockIdx.y;
    const bool is_act = ot < n_act_tiles;
    const int m = lane & 15, kq = lane >> 4;
    const int groups = is_act ? nd.groups_act : nd.groups_val;
    const int g0 = wave * groups / kHeadWaves, g1 = (wave + 1) * groups / kHeadWaves;
    const size_t ldw = (size_t)16 * groups, lda = (size_t)nd.feat_ld;
    const int n0 = 32 * (is_act ? ot : ot - n_act_tiles);
    const float *w = (is_act ? nd.fc_act_w : nd.fc_val1_w) + (size_t)(n0 + m) * ldw + 4 * kq;
    const float *a = feat + (size_t)(b0 + m) * lda + (is_act ? 0 : nd.feat_val_off) + 4 * kq;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ra[kHeadDepth][2], rw[kHeadDepth][2];
#pragma unroll
    for (int d = 0; d < kHeadDepth; ++d) {
        const int g = g0 + d;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ra[d][i] = f32x4{0.f, 0.f, 0.f, 0.f};
            rw[d][i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (g < g1) {
                ra[d][i] = *reinterpret_cast<const f32x4 *>(a + (size_t)(16 * i) * lda + 16 * g);
                rw[d][i] = *reinterpret_cast<const f32x4 *>(w + (size_t)(16 * i) * ldw + 16 * g);
            }
        }
    }
    for (int g = g0; g < g1; g += kHeadDepth) {
#pragma unroll
        for (int d = 0; d < kHeadDepth; ++d) {
            if (g + d >= g1) break;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[d][i][u], rw[d][j][u], acc[i][j], 0, 0, 0);
            const int gn = g + d + kHeadDepth;
            if (gn < g1) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    ra[d][i] = *reinterpret_cast<const f32x4 *>(a + (size_t)(16 * i) * lda + 16 * gn);
                    rw[d][i] = *reinterpret_cast<const f32x4 *>(w + (size_t)(16 * i) * ldw + 16 * gn);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) part[wave][2 * i + j][lane] = acc[i][j];
    __syncthreads();
    if (wave >= 4) return;
    // wave t finishes tile t = 2 i + j.  D: column = output (lane & 15), rows = boards 4 * (lane >> 4) + e
    const int ti = wave >> 1, tj = wave & 1;
    f32x4 v = part[0][wave][lane];
#pragma unroll
    for (int k = 1; k < kHeadWaves; ++k) {
        const f32x4 p = part[k][wave][lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += p[e];
    }
    const int col = n0 + 16 * tj + m;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int b = b0 + 16 * ti + 4 * kq + e;
        if (b >= n_boards) continue;
        if (is_act) raw[(size_t)b * nd.Npad + col] = v[e] + nd.fc_act_b[col];
        else hid[(size_t)b * 64 + col] = fmaxf(v[e] + nd.fc_val1_b[col], 0.0f);
    }
}

}  // namespace
