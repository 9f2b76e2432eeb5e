// rz_delta.h -- receptive-field ("delta") leaf evaluation for boards of 11 .. 16 rows and columns, on the records and the arithmetic of
// k_trunk_rows (rz_net_rows.h, namespace rt), cell by cell; rz_net.hip includes it with the other kernel families' headers.
//
// Why.  The reference's search (alphazero_mcts.py:42-71 under node.py:32-42's UCT rule) is near breadth-first: at 15 x 15 / 800
// simulations a leaf is the root position plus ONE or TWO stones (mean depth 1.74).  PolicyValueNet.forward
// (policy_value_net.py:34-52) is three zero-padded 3 x 3 convolutions and two 1 x 1 head convolutions, so a changed input cell moves
// conv1's output only in the 3 x 3 window around it, conv2's in the 5 x 5, conv3's and the head features in the 7 x 7 window.  Per
// game and move the trunk is therefore evaluated ONCE on two pseudo-positions of the root ("bases": the root's stones seen by the
// side to move / by the other side, no last-move plane, the stone-count plane of that parity) with conv1's and conv2's outputs and the
// six head-feature planes kept in HBM (BaseCache); a leaf then recomputes only the cells inside the windows of the cells where its
// planes differ from the base of its parity (the added stones; the last move is one of them).
//
// Same bits.  An MFMA column (a cell) never mixes with another column, an accumulator sees the products of its cell in the order
// (tap column, channel chunk) -> kernel row -> (hi x hi, hi x lo, lo x hi) of rt::slot_r, the epilogues are the element-wise code of
// trunk_rows_body, the 1 x 1 head sums keep its tree ((lane groups 0 + 1) + (2 + 3), then the waves in wave order): every value a
// leaf's window holds is what k_trunk_rows computes for that cell, bit for bit (tests/test_delta_trunk.py); a cell outside the
// windows takes the base's value, which is k_trunk_rows' as well.  The one formal difference: k_trunk_rows never multiplies the zero
// ring above / below the board, here an off-board tap meets an all-zero record (acc + 0 = acc).
//
// One kernel, three uses (DeltaArgs::mode).  A workgroup owns a leaf.  The cells are not board rows but LISTS: thread = cell finds its
// distance to the changed cells, ballots compact the cells of every layer's window into tiles of 16 (conv2, conv3) or 32 (conv1) MFMA
// columns, a map [halo position] -> LDS record gives every tap its operand (records of cells outside a layer's window are copied from
// the base, off-board taps read the zero record).  LDS: 77 KB -- TWO workgroups per CU, so one leaf's gathers and vector phases run
// under the other's MFMAs.  A leaf whose windows exceed the budget (more than kMaxD changed cells: deep paths late in a game; or a
// base that is not a subset of the leaf) is evaluated by the same code WITHOUT a base, in four passes over the board's quadrants
// (each pass: conv3 on <= 8 x 8 cells, conv2 on the 9 x 9 and conv1 on the 10 x 10 around them) -- no second kernel, no host decision.
// mode 1 builds the bases that way and writes the cache.
// (the prologue of a pass has ONE barrier: every wave ballots the membership of all four 64-cell blocks, so ranks and totals are in
// its registers, and a thread requests the base records it holds as soon as it knows it holds them -- one fetch, stored in the same
// phase; profiles/r07/ab_prologue.txt; k_delta_res: pass -1's sets come from the selecting wave instead, leaf_windows --
// profiles/r08/ab_windows.txt)

#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rlzero_hip.h"
#include "rz_gather.h"
#include "rz_net_dev.h"
#include "rz_net_rows.h"
#include "rz_net_split.h"
#include "rz_trace.h"
#include "rz_tree.h"
#include "rz_window.h"

// (issue priorities of the resident search's phases, s_setprio: its serial tree phase -- one wave, ~20 k cycles a simulation -- ahead of
// the OTHER game's trunk waves on the same SIMDs: +2.5 % on the whole line, profiles/r06/ab_prio.txt; PRO: the trunk's prologue likewise)
#ifndef RZ_DELTA_TREE_PRIO
#define RZ_DELTA_TREE_PRIO 1
#endif
#ifndef RZ_DELTA_PRO_PRIO
#define RZ_DELTA_PRO_PRIO 0
#endif
// (k_delta_res: wave 1 scores the root's siblings for the next selection while wave 0 backs the simulation up -- rzt::root_prescan;
// 0: the selection scans the root itself, as before -- profiles/r09/ab_prescan.txt)
#ifndef RZ_DELTA_PRESCAN
#define RZ_DELTA_PRESCAN 1
#endif
// (k_delta_res: wave 0 asks for the tree phase's loads one phase early -- rz_tree.h's fetch steps.  Bit 0: the backup's leaf state in
// front of the value layer, its path's records behind wave 0's own quarter of it; bit 1: the selection's root state behind the backup,
// in front of the barrier that orders the backup's stores.  3 is what ships and what the tests run; 0 and 1 exist for the A / B builds
// of profiles/r14/ab_early_loads.txt alone: every load where its body has it, the backup's fetch steps without the selection's)
#ifndef RZ_DELTA_EARLY
#define RZ_DELTA_EARLY 3
#endif

namespace {

namespace dl {

using sp::f16x4;
using sp::f16x8;
typedef const __attribute__((address_space(3))) f16x8 *lds_frag;
typedef const __attribute__((address_space(3))) uint32_t *lds_u32;
typedef __attribute__((address_space(3))) f16x4 *lds_h4;
typedef __attribute__((address_space(3))) f32x4 *lds_v4;

constexpr int kC1Slots = 128, kC2Slots = 164;   // records of conv1's / conv2's output a pass may hold
constexpr int kT1 = 4, kT2 = 8, kT3 = 8;        // tiles per pass: conv1 (32 cells each), conv2 / conv3 (16 cells each)
constexpr int kMaxD = 4;                        // changed cells a delta pass handles
constexpr int P1 = rt::Geo<32>::pos_bytes, P2 = rt::Geo<64>::pos_bytes;   // 160 / 288: k_trunk_rows' records
constexpr int kGrid = kRowW * kRowW;            // halo positions (18 x 18), position of cell (y, x) = (y + 1) * 18 + x + 1
constexpr int kShareFloats = kT3 * 4 * 96;      // the waves' shares of the head sums: [tile][wave][output][column]
constexpr int kHeadW = 128 * 6 * 4 + 128 * 4 + 32;   // the 1 x 1 head convolutions' weights [128][6], conv3's biases [128], the head biases [6 + 2], staged once
// (the planes: the hi pieces only -- the lo pieces of 0 / 1 planes are zero and conv1 skips their products)
constexpr int kOffC1 = sp::kInPieceBytes, kOffC2 = kOffC1 + kC1Slots * P1, kOffZero = kOffC2 + kC2Slots * P2, kOffHead = kOffZero + P2,
              kOffMap1 = kOffHead + kHeadW, kOffMap2 = kOffMap1 + kGrid * 4, kOffList = kOffMap2 + kGrid * 4,
              kLdsBytes = kOffList + 3 * 128 * 2;
static_assert(kShareFloats * 4 <= kC1Slots * P1, "the shares lie inside conv1's records (dead behind conv2)");
// the resident search's hand-over from the selection to the next leaf's prologue (leaf_windows): the four window sets of pass -1
// (radius 1 .. 4) as 4 x 4 words, their words' popcounts, the verdict (use_delta | parity << 1 | nD << 8)
constexpr int kWinSets = rzw::kRadii * rzw::kWords, kWinLds = kWinSets * 8 + kWinSets * 4 + 16;
static_assert(2 * (kLdsBytes + 512 * 4 + 4 * 64 * 4 + 80 + kWinLds + (int)sizeof(rzt::RootPre) + 512) <= 160 * 1024,
              "two workgroups per CU, also of the resident search (value row, K-quarter sums, leaf, window sets, root pre-scan)");
static_assert(kOffC1 % 16 == 0 && kOffZero % 16 == 0 && kOffHead % 16 == 0 && kOffMap1 % 16 == 0, "alignment");

// The base cache: per game a header (the stones the two bases were computed from) and per (game, parity) the records.
constexpr int kCells = RZ_MAX_BOARD_SIZE * RZ_MAX_BOARD_SIZE;
struct BaseHdr {
    uint64_t stones[2 * RZ_BOARD_WORDS];
    int32_t to_move, valid, pad[2];
};
constexpr size_t kBaseC2 = (size_t)kCells * 128, kBaseV = kBaseC2 + (size_t)kCells * 256, kBaseBytes = kBaseV + (size_t)6 * kCells * 4;

struct DeltaArgs {
    BaseHdr *hdr;            // [games]
    char *recs;              // [games][2 parities][kBaseBytes]: conv1 records [cell][hi 32 | lo 32] f16, conv2 records [cell][hi 64 | lo 64],
                             // head features [6][kCells] f32 (behind their ReLU)
    const uint8_t *active;   // mode 0: games whose flag is 0 are skipped (NULL: none is)
    float *feat32;           // the features as f32 [board][6 S] (tests; NULL otherwise)
    unsigned *stats;         // [8] counters (NULL: none): delta leaves, leaves without a base, conv3 tiles, changed cells, conv2 tiles, root scans
                             // answered from the pre-scan (k_delta_res), and of workgroup 0 of the LAST resident launch: shader-clock
                             // cycles >> 8, ticks of the constant 100 MHz clock
    int mode;                // 0: the leaves of `leaves` against the cache; 1: build the cache from the ROOT positions in `leaves`
                             // (board = 2 game + parity); 2: the leaves without a base (the four-pass route alone: a checker)
    int bw_rcp;              // ceil(65536 / width): cell / width = (cell * bw_rcp) >> 16 for cell < 4096
    const uint64_t *win;     // k_delta_res: the window table of the net's board (rz_window.h; NULL elsewhere)
};

__device__ __forceinline__ uint32_t lds_addr(const void *p) {
    return (uint32_t)(uintptr_t)((const __attribute__((address_space(3))) char *)p);
}

// ---- the convolutions at tiles of gathered cells.  pos19[t] = the lane's cell of tile t as halo position - 19 (every tap's map entry
// then lies at a non-negative offset); rec[t][dy] = the LDS record of tile t's tap (dy, current tap column) + the lane's k block.
// Per accumulator the order of rt::slot_r: (tap column, chunk) -> kernel row -> hi x hi, hi x lo, lo x hi.  The work of a step (tap
// column, chunk, kernel row) is cut into UNITS of at most three tiles: a unit's fragments are read from LDS while the unit before it
// multiplies (two sets of registers), and inside a unit the products go combo -> tile -> M-tile, so that an accumulator meets its next
// product 2 x (tiles of the unit) MFMAs later.
constexpr int unit_tiles(int nt) { return nt <= 3 ? nt : (nt + 1) / 2; }
constexpr int units_of(int nt) { return (nt + unit_tiles(nt) - 1) / unit_tiles(nt); }

template <int CIN, int NT, int UT>
__device__ __forceinline__ void read_unit(f16x8 (&b)[UT][2], const uint32_t (&rec)[NT][3], int h, int dy, int c) {
#pragma unroll
    for (int i = 0; i < UT; ++i) {
        const int t = h * UT + i;
        if (t < NT) {
            const uint32_t r = rec[t][dy] + (uint32_t)(c * 64);
            b[i][0] = *(lds_frag)(uintptr_t)r;
            b[i][1] = *(lds_frag)(uintptr_t)(r + CIN * 2);
        }
    }
}
template <int TM, int NT, int UT>
__device__ __forceinline__ void mfma_unit(f32x4 (&acc)[TM][NT], const f16x8 (&a)[TM][2], const f16x8 (&b)[UT][2], int h) {
#pragma unroll
    for (int combo = 0; combo < 3; ++combo)
#pragma unroll
        for (int i = 0; i < UT; ++i) {
            const int t = h * UT + i;
            if (t < NT) {
#pragma unroll
                for (int m = 0; m < TM; ++m)
                    acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[m][combo == 2], b[i][combo == 1], acc[m][t], 0, 0, 0);
            }
        }
}
template <int NT>
__device__ __forceinline__ void lookup(uint32_t (&rec)[NT][3], lds_u32 map, const int (&pos19)[NT], int dx, int g) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) rec[t][dy] = map[pos19[t] + dx + dy * kRowW] + (uint32_t)(g * 16);
}

// conv2 (32 -> 64): the wave's 16 output channels at NT <= 4 tiles; ALL its weight fragments (9 taps x hi / lo: 72 registers) are in
// registers.  A step = (tap column, kernel row) is one unit.
template <int NT>
__device__ __forceinline__ void conv2_g(lds_u32 map, const int (&pos19)[NT], int lane, const f16x8 (&a2)[9][1][2], f32x4 (&acc)[1][NT]) {
    static_assert(NT <= 4, "one unit per step");
    const int g = lane >> 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int AHEAD = NT <= 2 ? 2 : 1;   // units read ahead: a unit of one or two tiles (3 - 6 MFMAs) is shorter than an LDS round trip
    uint32_t rec[3][NT][3];
    f16x8 b[AHEAD + 1][NT][2];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) lookup<NT>(rec[dx], map, pos19, dx, g);
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) read_unit<32, NT, NT>(b[u], rec[u / 3], 0, u % 3, 0);
#pragma unroll
    for (int u = 0; u < 9; ++u) {   // u = 3 dx + dy
        const int dx = u / 3, dy = u % 3;
        if (u + AHEAD < 9) read_unit<32, NT, NT>(b[(u + AHEAD) % (AHEAD + 1)], rec[(u + AHEAD) / 3], 0, (u + AHEAD) % 3, 0);
        mfma_unit<1, NT, NT>(acc, a2[dy * 3 + dx], b[u % (AHEAD + 1)], 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// conv3 (64 -> 128): the wave's 32 output channels (two M-tiles) at NT <= 6 tiles.  A step (tap column, chunk, kernel row) needs four
// weight fragments; they come through a ring of R steps, requested R - 1 steps ahead: R = 6 where a step is short (up to four tiles:
// 24 MFMAs a step do not cover an L2 round trip two steps ahead), R = 3 above.  The first R - 1 steps are requested BEFORE the barrier
// behind conv2, which the waves meet in here (SYNC; the ring as a kernel-scope array handed through the barrier and the switch over the
// tile count cost 200 - 400 spilled registers).  The tap-column loop is rolled: 6 steps a turn.
#ifndef RZ_DELTA_RING6_UPTO
#define RZ_DELTA_RING6_UPTO 2
#endif
constexpr int ring3(int nt) { return nt <= RZ_DELTA_RING6_UPTO ? 6 : 3; }
__device__ __forceinline__ void load_a3(f16x8 (&a)[2][2], __amdgpu_buffer_rsrc_t w_rsrc, int lane, int dx, int j) {
    using G = rt::Geo<64>;
    const int c = j / 3, dy = j % 3;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int p = 0; p < 2; ++p)
            a[m][p] = sp::load_w(w_rsrc, lane * 16, dx * (G::chunks * 2048) + ((m * G::steps + dy * 3 * G::chunks + c) * 2 + p) * 1024);
}
template <int NT>
__device__ __forceinline__ void conv3_g(lds_u32 map, const uint16_t *list3, const void *wts, int lane, bool sync, f32x4 (&acc)[2][NT]) {
    static_assert(NT <= 6, "two units per step");
    constexpr int R = ring3(NT), H = units_of(NT);
    const int n = lane & 15, g = lane >> 4;
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(wts), 0, 0x7fffffff, 0x00020000);
    f16x8 a3[R][2][2];
#pragma unroll
    for (int j = 0; j < R - 1; ++j) load_a3(a3[j], w_rsrc, lane, 0, j);
    if (sync) __syncthreads();   // conv2's records are complete (the barrier behind conv2, met behind the first requests)
    int pos19[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) pos19[t] = (int)list3[16 * t + n] - 19;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint32_t rec[NT][3], recn[NT][3];
    // units read ahead: a unit of one or two tiles (6 - 12 MFMAs) is shorter than an LDS round trip under load
#ifndef RZ_DELTA_AHEAD3_SMALL
#define RZ_DELTA_AHEAD3_SMALL 1
#endif
    constexpr int UT = unit_tiles(NT), AH = UT <= 2 ? RZ_DELTA_AHEAD3_SMALL : 1, NB = AH + 1;
    static_assert((6 * H) % NB == 0 && AH <= H * 6, "a unit's registers are a constant of the unrolled body");
    f16x8 b[NB][UT][2];
    lookup<NT>(rec, map, pos19, 0, g);
#pragma unroll
    for (int u = 0; u < AH; ++u) read_unit<64, NT, UT>(b[u], rec, u % H, (u / H) % 3, u / H / 3);
#pragma unroll 1
    for (int dx = 0; dx < 3; ++dx) {
        lookup<NT>(recn, map, pos19, dx < 2 ? dx + 1 : 2, g);   // the next tap column's records (past the last: unused)
#pragma unroll
        for (int u = 0; u < 6 * H; ++u) {   // unit u = step (u / H) x tiles of group (u % H); 6 H is a multiple of NB: a unit's registers are constants
            const int j = u / H, h = u % H;
            if (h == 0) {   // the fragments of step j + R - 1 (past the last tap column: a reload of the last one's, never used)
                const int jj = j + R - 1, dx2 = jj < 6 ? dx : (dx < 2 ? dx + 1 : 2);
                load_a3(a3[jj % R], w_rsrc, lane, dx2, jj % 6);
            }
            {
                const int v = u + AH;   // the unit read now (past this tap column's last: the next column's first)
                if (v < 6 * H) read_unit<64, NT, UT>(b[v % NB], rec, v % H, (v / H) % 3, v / H / 3);
                else read_unit<64, NT, UT>(b[v % NB], recn, (v - 6 * H) % H, ((v - 6 * H) / H) % 3, (v - 6 * H) / H / 3);
            }
            mfma_unit<2, NT, UT>(acc, a3[j % R], b[u % NB], h);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) rec[t][dy] = recn[t][dy];
    }
}

// the lane's head values [tile][output] of T tiles (T = 4: 24 values, T = 8: 48) -> those of the T / 4 tiles its lane group is left with,
// summed over the four lane groups in f4::reduce_scatter_96's order: (group 0 + group 1) + (group 2 + group 3).  Group g keeps tiles
// (T / 2) (g & 1) + (T / 4) (g >> 1) + ...  O = outputs per tile (6: all; 4 / 2: the policy / the value planes alone, each value through the same swaps
// and sums)
template <int T, int O = 6>
__device__ __forceinline__ void reduce_scatter(const float (&vals)[O * T], float (&out)[O * T / 4]) {
    float r1[O * T / 2];
#pragma unroll
    for (int i = 0; i < O * T / 2; ++i) {
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(vals[i]), __float_as_uint(vals[O * T / 2 + i]), false, false);
        r1[i] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
#pragma unroll
    for (int i = 0; i < O * T / 4; ++i) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r1[i]), __float_as_uint(r1[O * T / 4 + i]), false, false);
        out[i] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
}

// conv2 of NT <= 4 tiles -> the cells' conv2 records (bias, ReLU, hi + lo pieces: trunk_rows_body's epilogue); n2 = cells of these tiles
template <int NT>
__device__ __forceinline__ void conv2_tiles(lds_u32 map1, lds_u32 map2, const uint16_t *list2, int n2, int lane, int wave, const f16x8 (&a2)[9][1][2],
                                            f32x4 bias2, float k2) {
    const int n = lane & 15, g = lane >> 4;
    int pos19[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) pos19[t] = (int)list2[16 * t + n] - 19;
    f32x4 acc[1][NT];
    conv2_g<NT>(map1, pos19, lane, a2, acc);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (16 * t + n < n2) {
            const uint32_t rec = map2[pos19[t] + kRowW + 1] + (uint32_t)((16 * wave + 4 * g) * 2);
            float z[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = fmaxf(fmaf(acc[0][t][j], k2, bias2[j]), 0.0f);
            f16x4 hi, lo;
            sp::split4(z, hi, lo);
            *(lds_h4)(uintptr_t)rec = hi;
            *(lds_h4)(uintptr_t)(rec + 128) = lo;
        }
    }
}

// conv3 of NT <= 6 tiles + the two 1 x 1 head convolutions -> the wave's shares of the six head sums of these tiles (shares: the first
// tile's).  headw (LDS): [128][6] weights, [128] biases.  Outputs OLO .. OHI - 1 alone (even bounds: 0 .. 3 the policy planes, 4 / 5 the
// value planes): the others' products, swaps and shares do not exist, the ones kept go through the operations they go through among all six.
template <int NT, int OLO = 0, int OHI = 6>
__device__ __forceinline__ void conv3_tiles(lds_u32 map2, const uint16_t *list3, const void *wts, int lane, int wave, bool sync,
                                            const char *headw, float k3, float *shares) {
    constexpr int T = NT <= 4 ? 4 : 8, O = OHI - OLO;
    static_assert(OLO % 2 == 0 && OHI % 2 == 0 && 0 <= OLO && OLO < OHI && OHI <= 6, "pairs of outputs");
    const int n = lane & 15, g = lane >> 4;
    float vals[O * T];
    {
        f32x4 acc[2][NT];
        conv3_g<NT>(map2, list3, wts, lane, sync, acc);
        // the lane's 8 channels of conv3 (32 wave + 16 m + 4 g + j) meet 6 outputs each (trunk_rows_body: hwr, b3r)
        f32x4 hwr[2][6], b3r[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int c0 = 32 * wave + 16 * m + 4 * g;
#pragma unroll
            for (int i = 0; i < 6; ++i) hwr[m][i] = *reinterpret_cast<const f32x4 *>(headw + (c0 * 6 + 4 * i) * 4);
            b3r[m] = *reinterpret_cast<const f32x4 *>(headw + 128 * 6 * 4 + c0 * 4);
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            f32x2 v2[3] = {f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}};
            if (t < NT) {
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float hv = fmaxf(fmaf(acc[m][t < NT ? t : 0][j], k3, b3r[m][j]), 0.0f);
#pragma unroll
                        for (int o2 = OLO / 2; o2 < OHI / 2; ++o2) {
                            const int e = 6 * j + 2 * o2;
                            v2[o2] = __builtin_elementwise_fma(f32x2{hwr[m][e >> 2][e & 3], hwr[m][e >> 2][(e & 3) + 1]}, f32x2{hv, hv}, v2[o2]);
                        }
                    }
            }
#pragma unroll
            for (int o = OLO; o < OHI; ++o) vals[t * O + o - OLO] = v2[o >> 1][o & 1];
        }
    }
    float mine[O * T / 4];
    reduce_scatter<T, O>(vals, mine);
    const int t0 = (T / 2) * (g & 1) + (T / 4) * (g >> 1);
#pragma unroll
    for (int i = 0; i < O * T / 4; ++i)
        if (t0 + i / O < NT) shares[((t0 + i / O) * 4 + wave) * 96 + (OLO + i % O) * 16 + n] = mine[i];
}

// ---- what the pass loop of a leaf needs (one struct so that the two kernels below share the loop)
struct Leaf {
    f16x4 cell_planes;        // the four planes of this thread's cell (delta_passes<true>: not read, the planes are formed from leaf_lds)
    const uint64_t *leaf_lds; // delta_passes<true>: the leaf in LDS (select_body's lds_leaf layout: stones [8], side to move, last cell)
    const char *base;         // the base of the leaf's parity (mode 1: the base being built)
    int dys[kMaxD], dxs[kMaxD];   // the changed cells (-100: none)
    _Float16 *dst16;          // the policy pieces' place in the store (NULL: none)
    float *vdst;              // the value head's input row (global memory, or LDS in the resident search)
    float *dst32;             // f32 features (tests; NULL otherwise)
    const uint64_t *sets;     // delta_passes<true>: pass -1's window sets, handed over in LDS (leaf_windows)
    uint16_t *gtab;           // delta_passes<true>: THIS wave's table of the base records it copies (rz_gather.h: rzg::Split<3>::kTabEntries entries of LDS)
    bool deferred, store_head;
};
struct Layers {
    float k1, k2, k3, act1, act2, act3;
    const char *t2p, *t3p;
};
#ifdef RZ_NET_PROFILE
struct Prof { long long acc[24], t; };
#else
struct Prof {};
#endif

// once per launch: every map entry -> the zero record, every list entry -> a valid position (cell 0)
__device__ __forceinline__ void init_maps(char *lds, int tid) {
    uint32_t *map1 = reinterpret_cast<uint32_t *>(lds + kOffMap1);
    const uint32_t zaddr = lds_addr(lds + kOffZero);
    for (int i = tid; i < 2 * kGrid; i += 256) map1[i] = zaddr;    // (map1 and map2 are contiguous)
    if (tid < 3 * 128 / 2) reinterpret_cast<uint32_t *>(lds + kOffList)[tid] = 19u | (19u << 16);
}

// Chebyshev distance of cell (cy, cx) to the changed cells (pass -1) / to quadrant `pass` of the board
__device__ __forceinline__ int cell_dist(int cy, int cx, int pass, const int (&dys)[kMaxD], const int (&dxs)[kMaxD], int BH, int BW) {
    int dist = 1000;
    if (pass < 0) {
#pragma unroll
        for (int i = 0; i < kMaxD; ++i) {
            const int ady = cy > dys[i] ? cy - dys[i] : dys[i] - cy, adx = cx > dxs[i] ? cx - dxs[i] : dxs[i] - cx;
            const int d = ady > adx ? ady : adx;
            dist = d < dist ? d : dist;
        }
    } else {
        const int y0 = 8 * (pass >> 1), x0 = 8 * (pass & 1);
        const int y1 = (y0 + 8 < BH ? y0 + 8 : BH) - 1, x1 = (x0 + 8 < BW ? x0 + 8 : BW) - 1;   // (inclusive)
        const int ddy = cy < y0 ? y0 - cy : (cy > y1 ? cy - y1 : 0), ddx = cx < x0 ? x0 - cx : (cx > x1 ? cx - x1 : 0);
        dist = ddy > ddx ? ddy : ddx;
    }
    return dist;
}

// 16 bytes of a base's records (offset >= kBaseBytes: zeros, no memory access -- the buffer's range check)
constexpr int kOutside = 1 << 30;
__device__ __forceinline__ f32x4 load_rec(__amdgpu_buffer_rsrc_t rsrc, int off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
}

__device__ __forceinline__ uint64_t uni64(uint64_t v) {
    return ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

// set bits of a word (the same in every lane) below this lane's bit: rzg::below(word, lane)
__device__ __forceinline__ int lane_below(uint64_t word) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word, 0u));
}
static_assert(rzg::kC1Max == kC1Slots && rzg::kC2Max == kC2Slots && rzg::kC1Bytes * kCells == (int)kBaseC2 && rzg::kOutside == kOutside,
              "rz_gather.h's records are the base's and the budget is this file's");
static_assert(rzg::kC1Bytes <= P1 && rzg::kC2Bytes <= P2, "a record fits its LDS slot");

__device__ __forceinline__ f16x4 planes_of(const uint64_t (&ls)[8], int tid, int tm_eff, bool has_last, int lc, int par_count);

// the leaf the selection left in LDS (wave-uniform values)
__device__ __forceinline__ void leaf_from_lds(const uint64_t *leaf_lds, uint64_t (&ls)[8], int &tm, int &lc, int &nst) {
    nst = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        ls[q] = uni64(leaf_lds[q]);
        nst += __popcll(ls[q]);
    }
    tm = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int *>(leaf_lds + 2 * RZ_BOARD_WORDS)[0]);
    lc = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int *>(leaf_lds + 2 * RZ_BOARD_WORDS)[1]);
}

// conv1 (4 -> 32) of tile `tile` of list1 (32 cells) by one wave: trunk_rows_body's conv1 with the lane's cell taken from the list
__device__ __forceinline__ void conv1_tile(int tile, int total, int lane, const char *in0, const uint16_t *list1, const uint32_t *map1,
                                           const sp::f16x8 (&a1)[3][2], const f32x4 (&bias1)[4], float k1, float act1) {
    const int n32 = lane & 31, h = lane >> 5, idx = 32 * tile + n32;
    const int pos = list1[idx];
    const int py = (pos * 3641) >> 16, px = pos - py * kRowW;   // halo row / column (board row py - 1, column px - 1)
    typedef const __attribute__((address_space(3))) f16x4 *lds_half;
    const lds_half q = (lds_half)(in0 + ((py - 1) * sp::kInCols + (px - 1) + 2 * h) * 8);
    sp::f16x8 b1[3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int o = ky * sp::kInCols;
        const f16x4 lo4 = q[o], hi4 = q[o + 1];
        b1[ky] = __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    sp::f32x16 acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[r] = 0.0f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int combo = 0; combo < 3; combo += 2)   // (the lo pieces of 0 / 1 planes are zero: no hi x lo product)
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[ky][combo == 2], b1[ky], acc1, 0, 0, 0);
    if (idx < total) {
        const uint32_t rec = map1[pos] + (uint32_t)(4 * h * 2);
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            float z[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = fmaxf(fmaf(acc1[4 * gg + j], k1, bias1[gg][j] * act1), 0.0f);
            f16x4 hi, lo;
            sp::split4(z, hi, lo);
            *(lds_h4)(uintptr_t)(rec + 8 * gg * 2) = hi;
            *(lds_h4)(uintptr_t)(rec + 8 * gg * 2 + 64) = lo;
        }
    }
}

// The passes of one leaf: -1 = against the base (use_delta), 0 .. 3 = the board's quadrants without one.  -> tiles computed: conv3 | conv2 << 16.
// SETS (k_delta_res): pass -1 takes its cell sets, ranks and totals from leaf.sets (leaf_windows) instead of the distances and ballots.
// OLO, OHI: the head planes this leaf is evaluated for (conv3_tiles; the base's values of the others are not requested either) -- all six,
// the value planes alone (the search of policy on demand: 4, 6) or the policy planes alone (its flush, k_trunk_policy_rows: 0, 4).
template <bool SETS, int OLO = 0, int OHI = 6>
__device__ __forceinline__ int delta_passes(const NetDev &nd, const DeltaArgs &da, char *lds, int tid0, int wave, const Leaf &leaf, const Layers &ly,
                                            f32x4 headv, bool &use_delta, Prof &prof) {
    char *in0 = lds, *c1 = lds + kOffC1, *c2 = lds + kOffC2, *zrec = lds + kOffZero, *headw = lds + kOffHead;
    uint32_t *map1 = reinterpret_cast<uint32_t *>(lds + kOffMap1), *map2 = reinterpret_cast<uint32_t *>(lds + kOffMap2);
    uint16_t *list1 = reinterpret_cast<uint16_t *>(lds + kOffList), *list2 = list1 + 128, *list3 = list2 + 128;
    float *shares = reinterpret_cast<float *>(c1);
    const int mode = da.mode, BH = nd.BH, BW = nd.BW, S = nd.S;
    const float k1 = ly.k1, k2 = ly.k2, k3 = ly.k3, act1 = ly.act1, act2 = ly.act2, act3 = ly.act3;
    const char *t2p = ly.t2p, *t3p = ly.t3p;
    const char *base = leaf.base;
    const int (&dys)[kMaxD] = leaf.dys, (&dxs)[kMaxD] = leaf.dxs;
    _Float16 *dst16 = leaf.dst16;
    float *vdst = leaf.vdst, *dst32 = leaf.dst32;
    const bool deferred = leaf.deferred, store_head = leaf.store_head;
    const uint32_t zaddr = lds_addr(zrec);
    int n_conv3_tiles = 0, n_conv2_tiles = 0;
#ifdef RZ_NET_PROFILE
    long long (&prof_acc)[24] = prof.acc, &prof_t = prof.t;
#endif
    for (int pass = use_delta ? -1 : 0; pass < 4; ++pass) {
        // (the thread's number is opaque per pass: hipcc otherwise hoists every lane-dependent address of the pass -- of all its
        // instantiations -- out of this loop and spills them: trunk_rows_body's board loop does the same)
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, g = lane >> 4;
        const int cy = (tid * da.bw_rcp) >> 16, cx = tid - cy * BW;
        const bool is_cell = tid < S;
        const int mypos = is_cell ? (cy + 1) * kRowW + cx + 1 : 0;
        if (RZ_DELTA_PRO_PRIO) __builtin_amdgcn_s_setprio(RZ_DELTA_PRO_PRIO);
        // sets: 0 = conv1 computes, 1 = conv2 computes, 2 = conv3 computes, 3 = conv1 records held, 4 = conv2 records held
        const int th[5] = {pass < 0 ? 1 : 2, pass < 0 ? 2 : 1, pass < 0 ? 3 : 0, pass < 0 ? 3 : 2, pass < 0 ? 4 : 1};
        bool f[5];
        uint64_t own[5];   // (SETS, pass -1: set k = the window of radius th[k] handed over by the selection; the wave's word of it)
        const bool handed = SETS && pass < 0;   // (uniform)
        int rank[5], tot[5];
        if (handed) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                own[k] = uni64(leaf.sets[4 * (th[k] - 1) + wave]);
                f[k] = (own[k] >> lane) & 1ull;   // (cells past the board: no bit)
            }
            // ranks and totals: the handed-over words' popcounts (before the requests: conv1's weights depend on its total)
            const int *cnt = reinterpret_cast<const int *>(leaf.sets + kWinSets);
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                int before = 0, all = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int c = __builtin_amdgcn_readfirstlane(cnt[4 * (th[k] - 1) + w]);
                    all += c;
                    before += w < wave ? c : 0;
                }
                rank[k] = before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(own[k] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)own[k], 0u));
                tot[k] = all;
            }
        } else {
            // ---- the distance of this thread's cell to the changed cells (delta) / to the pass's quadrant
            const int dist = cell_dist(cy, cx, pass, dys, dxs, BH, BW);
#pragma unroll
            for (int k = 0; k < 5; ++k) f[k] = is_cell && dist <= th[k];
        }
        // the records conv2 / conv3 read but this leaf does not recompute come from the base: requested NOW, straight into the
        // registers they are stored from (no barrier lies between).  Every load is issued by every thread --
        // a load under a branch makes hipcc wait for every outstanding load first --; a thread that holds no such record reads
        // past the end of a buffer resource instead, which returns zeros without touching memory.
        // SETS (k_delta_res): the same bytes record by record (rz_gather.h) -- the lanes of a wave-instruction read whole records, 8
        // (conv1) or 16 (conv2) lanes each, so a 128-byte line is touched once.  The gather is the work of waves 1 .. 3 (the three-wave
        // split, gathering wave gw = wave - 1: 6 + 14 requests a wave); wave 0 -- behind the selection's tail when the others are here,
        // and conv1 of pass -1 is its work -- has no table and no gather in that pass.  Table, requests and stores stand in ONE uniform
        // region further down, behind the maps and lists: with the requests up here and the stores down there, a branch around each
        // spilled the requests' registers (profiles/TRIED.md, round 13); inside the region nothing is under a branch of its own.
        const bool g1 = pass < 0 && f[3] && !f[0], g2 = pass < 0 && f[4] && !f[1];
        const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(base), 0, kBaseBytes, 0x00020000);
        f32x4 r1[8], r2[16];
        typedef rzg::Split<SETS ? 3 : 4> GS;
        constexpr int NW = SETS ? 3 : 4;
        if constexpr (!SETS) {
            const int o1 = g1 ? tid * 128 : kOutside, o2 = g2 ? (int)kBaseC2 + tid * 256 : kOutside;
#pragma unroll
            for (int i = 0; i < 8; ++i) r1[i] = load_rec(b_rsrc, o1 + 16 * i);
#pragma unroll
            for (int i = 0; i < 16; ++i) r2[i] = load_rec(b_rsrc, o2 + 16 * i);
        }
        float bv[6];   // ... and, behind them (the copies' waits do not include these), the features of a cell outside conv3's window
        {
            const int ov = pass < 0 && is_cell && !f[2] ? (int)kBaseV + tid * 4 : kOutside;
#pragma unroll
            for (int o = OLO; o < OHI; ++o) bv[o] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(b_rsrc, ov + o * kCells * 4, 0, 0));
        }
        // (conv1's weights and the biases: requested per pass, so that nothing of them is live across conv3)
        // (SETS, pass -1: conv1 is wave 0's, every tile of it; the other waves request them past the end of their buffers)
        sp::f16x8 a1[3][2];
        f32x4 bias1[4];
        if constexpr (SETS) {
            const __amdgpu_buffer_rsrc_t s_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<f32x4 *>(nd.s1), 0, 6 * 64 * 16, 0x00020000);
            const __amdgpu_buffer_rsrc_t o_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(nd.b1), 0, 32 * 4, 0x00020000);
            const bool runs = !handed || wave == 0;   // (uniform)
            const int so = runs ? lane * 16 : kOutside, bo = runs ? 16 * (lane >> 5) : kOutside;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int p_ = 0; p_ < 2; ++p_) a1[ky][p_] = sp::load_w(s_rsrc, so, (ky * 2 + p_) * 1024);
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) bias1[gg] = load_rec(o_rsrc, bo + 32 * gg);
        } else if (32 * wave < 32 * kT1) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int p_ = 0; p_ < 2; ++p_) a1[ky][p_] = __builtin_bit_cast(sp::f16x8, nd.s1[(ky * 2 + p_) * 64 + lane]);
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) bias1[gg] = *reinterpret_cast<const f32x4 *>(nd.b1 + 8 * gg + 4 * (lane >> 5));
        }
        f32x4 bias2 = *reinterpret_cast<const f32x4 *>(nd.b2 + 16 * wave + 4 * g);
        // ranks and totals without a barrier: every wave evaluates the membership of all four 64-cell blocks (its own block's ballots
        // give the ranks inside the wave, the blocks before it the offsets); the same values in every wave, so the budget test is uniform
        if (!handed) {
            int before[5] = {0, 0, 0, 0, 0}, all[5] = {0, 0, 0, 0, 0};
            unsigned long long own[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int cell = 64 * b + lane, by = (cell * da.bw_rcp) >> 16, bx = cell - by * BW;
                const int d = cell_dist(by, bx, pass, dys, dxs, BH, BW);
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const unsigned long long m = __ballot(cell < S && d <= th[k]);
                    const int c = __popcll(m);
                    all[k] += c;
                    before[k] += b < wave ? c : 0;
                    own[k] = b == wave ? m : own[k];
                }
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                rank[k] = before[k] + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(own[k] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)own[k], 0u));
                tot[k] = all[k];
            }
        }
        NET_TICK(1);   // distances, requests, ranks
        if (pass < 0 && (tot[0] > 32 * kT1 || tot[1] > 16 * kT2 || tot[2] > 16 * kT3 || tot[3] > kC1Slots || tot[4] > kC2Slots)) {
            use_delta = false;   // (uniform) the windows exceed the budget: the four passes without a base (nothing is written yet)
            continue;
        }
        // (maps and lists: every map entry is the zero record and every list entry a valid position when a pass begins -- set once per
        // launch, init_maps; a pass puts back what it changed, and a lane past a list's count may read any position: its column is dropped)
        uint32_t rec1 = 0, rec2 = 0;
        if (f[3]) {
            rec1 = lds_addr(c1 + rank[3] * P1);
            map1[mypos] = rec1;
        }
        if (f[4]) {
            rec2 = lds_addr(c2 + rank[4] * P2);
            map2[mypos] = rec2;
        }
        if (f[0]) list1[rank[0]] = (uint16_t)mypos;
        if (f[1]) list2[rank[1]] = (uint16_t)mypos;
        if (f[2]) list3[rank[2]] = (uint16_t)mypos;
        if constexpr (SETS) {
            // (k_delta_res: the leaf is in LDS, and nobody has read it yet; pass -1: wave 0 writes the planes of every cell, below)
            if (!handed && pass <= 0) {
                uint64_t ls[8];
                int tm, lc, nst;
                leaf_from_lds(leaf.leaf_lds, ls, tm, lc, nst);
                const f16x4 planes = planes_of(ls, tid, tm, nst > 0, lc, nst);
                if (is_cell) *reinterpret_cast<f16x4 *>(in0 + ((cy + 1) * sp::kInCols + (cx + 1)) * 8) = planes;
            }
        } else {
            if (pass <= 0 && is_cell) *reinterpret_cast<f16x4 *>(in0 + ((cy + 1) * sp::kInCols + (cx + 1)) * 8) = leaf.cell_planes;
        }
        if (pass <= 0 && store_head && tid < 226) reinterpret_cast<f32x4 *>(headw)[tid] = headv;
        if constexpr (SETS) {
          // ---- the gather (see above): which record a lane group copies comes from the wave's own table -- lane L writes the entries
          // of its held cells L, 64 + L, 128 + L, 192 + L that fall to this wave, the wave reads the entries of its rounds back (its
          // LDS operations complete in order: no barrier) --, then all requests, then all stores: no other work stands
          // between a request and its store any more, these waves wait the latency out (profiles/r13/delta_resident_phases.txt).
          if (!(handed && wave == 0)) {   // (uniform; wave 0 of the handed pass: no table, no gather)
            // (no branch around single requests or stores: the passes without a base -- handed false -- go through the same
            // instructions with no record anywhere, as they went through the cell-by-cell requests)
            f32x4 q1[GS::kC1Rounds], q2[GS::kC2Rounds];
            uint32_t d1[GS::kC1Rounds], d2[GS::kC2Rounds];   // where a round's 16 bytes go (no record: the zeros it was answered, to the zero record)
            uint16_t *tab = leaf.gtab;
            const int gw = wave - 1, gwi = gw < 0 ? 0 : gw;   // (wave 0: no place is its own, and the entries it reads back are nobody's)
            const bool gathers = handed && gw >= 0;           // (uniform)
            // held records / slots in the words before word w, and in all: the popcounts the hand-over stored behind the sets, scalar
            // (W1 <= W3 and W2 <= W4, so a held set's count is a difference)
            const int *wcnt = reinterpret_cast<const int *>(leaf.sets + kWinSets);
            int pn1[rzg::kWords + 1], ps1[rzg::kWords + 1], pn2[rzg::kWords + 1], ps2[rzg::kWords + 1];
            pn1[0] = ps1[0] = pn2[0] = ps2[0] = 0;
#pragma unroll
            for (int w = 0; w < rzg::kWords; ++w) {
                const int k0 = __builtin_amdgcn_readfirstlane(wcnt[4 * 0 + w]), k1_ = __builtin_amdgcn_readfirstlane(wcnt[4 * 1 + w]);
                const int k2_ = __builtin_amdgcn_readfirstlane(wcnt[4 * 2 + w]), k3_ = __builtin_amdgcn_readfirstlane(wcnt[4 * 3 + w]);
                pn1[w + 1] = pn1[w] + k2_ - k0, ps1[w + 1] = ps1[w] + k2_;
                pn2[w + 1] = pn2[w] + k3_ - k1_, ps2[w + 1] = ps2[w] + k3_;
            }
            const int n1 = pn1[rzg::kWords], n2 = pn2[rzg::kWords];
            if (gathers) {
                // (all sixteen words first, in one batch of LDS reads; they stay in vector registers -- the same value in every lane --:
                // nothing here needs them in scalar ones)
                uint64_t ws[rzw::kRadii][rzg::kWords];
#pragma unroll
                for (int r = 0; r < rzw::kRadii; ++r)
#pragma unroll
                    for (int w = 0; w < rzg::kWords; ++w) ws[r][w] = leaf.sets[4 * r + w];
#pragma unroll
                for (int w = 0; w < rzg::kWords; ++w) {
                    const uint64_t h1 = rzg::held(ws[2][w], ws[0][w]), h2 = rzg::held(ws[3][w], ws[1][w]);
                    const int cell = 64 * w + lane;
                    const int p1 = rzg::c1_place<NW>(pn1[w] + lane_below(h1), gw), p2 = rzg::c2_place<NW>(pn2[w] + lane_below(h2), gw);
                    const uint16_t e1 = rzg::entry(cell, ps1[w] + lane_below(ws[2][w])), e2 = rzg::entry(cell, ps2[w] + lane_below(ws[3][w]));
                    if (((h1 >> lane) & 1ull) && p1 >= 0) tab[p1] = e1;
                    if (((h2 >> lane) & 1ull) && p2 >= 0) tab[p2] = e2;
                }
            }
            const uint32_t c1a = lds_addr(c1), c2a = lds_addr(c2);
#pragma unroll
            for (int i = 0; i < GS::kC1Rounds; ++i) {
                const int j = rzg::c1_record<NW>(i, gwi, lane), chunk = rzg::c1_chunk(lane);
                const uint16_t e = tab[rzg::c1_index<NW>(j)];
                const bool has = gathers && rzg::c1_has(j, n1);
                d1[i] = has ? c1a + (uint32_t)rzg::dst(rzg::entry_slot(e), chunk, P1) : zaddr + 16u * (uint32_t)chunk;
                q1[i] = load_rec(b_rsrc, rzg::c1_src(has, rzg::entry_cell(e), chunk));
            }
#pragma unroll
            for (int i = 0; i < GS::kC2Rounds; ++i) {
                const int j = rzg::c2_record<NW>(i, gwi, lane), chunk = rzg::c2_chunk(lane);
                const uint16_t e = tab[rzg::c2_index<NW>(j)];
                const bool has = gathers && rzg::c2_has(j, n2);
                d2[i] = has ? c2a + (uint32_t)rzg::dst(rzg::entry_slot(e), chunk, P2) : zaddr + 16u * (uint32_t)chunk;
                q2[i] = load_rec(b_rsrc, rzg::c2_src(has, rzg::entry_cell(e), chunk, (int)kBaseC2));
            }
#pragma unroll
            for (int i = 0; i < GS::kC1Rounds; ++i) *(lds_v4)(uintptr_t)d1[i] = q1[i];
#pragma unroll
            for (int i = 0; i < GS::kC2Rounds; ++i) *(lds_v4)(uintptr_t)d2[i] = q2[i];
          }
        } else {
            if (g1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) *(lds_v4)(uintptr_t)(rec1 + 16 * i) = r1[i];
            }
            if (g2) {
#pragma unroll
                for (int i = 0; i < 16; ++i) *(lds_v4)(uintptr_t)(rec2 + 16 * i) = r2[i];
            }
        }
        __builtin_amdgcn_sched_barrier(0);   // (the requests below stay behind the stores of the base's records: their 96 registers are free again)
        f16x8 a2[9][1][2];   // conv2's weight fragments: requested here, conv1 -- one wave's work -- covers their latency
        {
            const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(t2p), 0, 0x7fffffff, 0x00020000);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int p = 0; p < 2; ++p) a2[tap][0][p] = sp::load_w(w_rsrc, lane * 16, (tap * 2 + p) * 1024);
        }
        if (handed) {
            // ---- pass -1 of the resident search: conv1 reads the planes alone, so it does not wait for the gather -- wave 0, which comes
            // here last (the selection's tail), does ALL of it in front of the pass's one barrier before conv2: the planes of every cell
            // (lane L: cells L, 64 + L, 128 + L, 192 + L), the list and map entries of W1's cells in every word (the owners write the
            // same values; this wave's LDS operations complete in order, so it reads its own back), then every tile of conv1.
            if (wave == 0) {
                uint64_t ls[8];
                int tm, lc, nst;
                leaf_from_lds(leaf.leaf_lds, ls, tm, lc, nst);
                const int *cnt = reinterpret_cast<const int *>(leaf.sets + kWinSets);
                int b0 = 0, b3 = 0;   // W1's / W3's cells in the words before this one
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int cell = 64 * w + lane, y = (cell * da.bw_rcp) >> 16, x = cell - y * BW;
                    const f16x4 planes = planes_of(ls, cell, tm, nst > 0, lc, nst);
                    if (cell < S) *reinterpret_cast<f16x4 *>(in0 + ((y + 1) * sp::kInCols + (x + 1)) * 8) = planes;
                    const uint64_t w1 = uni64(leaf.sets[4 * 0 + w]), w3 = uni64(leaf.sets[4 * 2 + w]);
                    const int pos = (y + 1) * kRowW + x + 1;
                    if ((w1 >> lane) & 1ull) {
                        list1[b0 + lane_below(w1)] = (uint16_t)pos;
                        map1[pos] = lds_addr(c1 + (b3 + lane_below(w3)) * P1);
                    }
                    b0 += __builtin_amdgcn_readfirstlane(cnt[4 * 0 + w]);
                    b3 += __builtin_amdgcn_readfirstlane(cnt[4 * 2 + w]);
                }
#pragma unroll 1
                for (int tile = 0; 32 * tile < tot[0]; ++tile) conv1_tile(tile, tot[0], lane, in0, list1, map1, a1, bias1, k1, act1);
            }
            NET_TICK(3);   // maps, lists, the base's records (their arrival); wave 0: the planes, conv1
            __syncthreads();
            NET_TICK(4);
        } else {
            NET_TICK(3);   // maps, lists, planes, the base's records (their arrival)
            __syncthreads();
            NET_TICK(4);
            // ---- conv1 (4 -> 32): tile w of 32 cells by wave w
            if (32 * wave < tot[0]) conv1_tile(wave, tot[0], lane, in0, list1, map1, a1, bias1, k1, act1);
            NET_TICK(5);   // conv1
            __syncthreads();
            NET_TICK(6);
        }
        if (mode == 1 && f[0]) {   // the base keeps conv1's records
            f32x4 *dstp = reinterpret_cast<f32x4 *>(const_cast<char *>(base) + (size_t)tid * 128);
#pragma unroll
            for (int i = 0; i < 8; ++i) dstp[i] = *(lds_v4)(uintptr_t)(rec1 + 16 * i);
        }

        if (RZ_DELTA_PRO_PRIO) __builtin_amdgcn_s_setprio(0);   // (the matrix loops: behind the other workgroup's latency chains at issue)
        // ---- conv2 (32 -> 64): wave w = output channels 16 w .. 16 w + 15 at every tile
        const int nt3 = (tot[2] + 15) >> 4;
        {
            const lds_u32 m1 = (lds_u32)map1, m2 = (lds_u32)map2;
            const int nt2 = (tot[1] + 15) >> 4;
            n_conv2_tiles += nt2;
            for (int t0 = 0; t0 < nt2; t0 += 4) {   // groups of up to four tiles (the weights are in registers: a group costs no fetch)
                const uint16_t *l2 = list2 + 16 * t0;
                const int left = tot[1] - 16 * t0;
                switch (nt2 - t0) {
                    case 1: conv2_tiles<1>(m1, m2, l2, left, lane, wave, a2, bias2 * act2, k2); break;
                    case 2: conv2_tiles<2>(m1, m2, l2, left, lane, wave, a2, bias2 * act2, k2); break;
                    case 3: conv2_tiles<3>(m1, m2, l2, left, lane, wave, a2, bias2 * act2, k2); break;
                    default: conv2_tiles<4>(m1, m2, l2, left, lane, wave, a2, bias2 * act2, k2); break;
                }
            }
        }
        NET_TICK(7);   // conv2

        // ---- conv3 (64 -> 128) + the head convolutions: wave w = output channels 32 w .. 32 w + 31 at every tile
        {
            const lds_u32 m2 = (lds_u32)map2;
            n_conv3_tiles += nt3;
            // up to six tiles in one go; seven or eight as four + the rest (the weights are fetched again: rare, big leaves only)
            const int first = nt3 <= 6 ? nt3 : 4;
            switch (first) {
                case 0: __syncthreads(); break;   // (the barrier behind conv2, which the other cases meet inside conv3_g)
                case 1: conv3_tiles<1, OLO, OHI>(m2, list3, t3p, lane, wave, true, headw, k3, shares); break;
                case 2: conv3_tiles<2, OLO, OHI>(m2, list3, t3p, lane, wave, true, headw, k3, shares); break;
                case 3: conv3_tiles<3, OLO, OHI>(m2, list3, t3p, lane, wave, true, headw, k3, shares); break;
                case 4: conv3_tiles<4, OLO, OHI>(m2, list3, t3p, lane, wave, true, headw, k3, shares); break;
                case 5: conv3_tiles<5, OLO, OHI>(m2, list3, t3p, lane, wave, true, headw, k3, shares); break;
                default: conv3_tiles<6, OLO, OHI>(m2, list3, t3p, lane, wave, true, headw, k3, shares); break;
            }
            if (nt3 == 7) conv3_tiles<3, OLO, OHI>(m2, list3 + 64, t3p, lane, wave, false, headw, k3, shares + 4 * 4 * 96);
            else if (nt3 >= 8) conv3_tiles<4, OLO, OHI>(m2, list3 + 64, t3p, lane, wave, false, headw, k3, shares + 4 * 4 * 96);
        }
        NET_TICK(9);   // the barrier behind conv2, conv3 + heads
        __syncthreads();
        NET_TICK(10);
        if (mode == 1 && f[1]) {   // the base keeps conv2's records too
            f32x4 *dstp = reinterpret_cast<f32x4 *>(const_cast<char *>(base) + kBaseC2 + (size_t)tid * 256);
#pragma unroll
            for (int i = 0; i < 16; ++i) dstp[i] = *(lds_v4)(uintptr_t)(rec2 + 16 * i);
        }

        // ---- the features: thread = cell adds the waves' shares in wave order (a cell outside the windows: the base's value)
        if (is_cell && (pass < 0 || f[2])) {
            const float *share = shares + (rank[2] >> 4) * 4 * 96 + (rank[2] & 15);
            float *basev = mode == 1 ? reinterpret_cast<float *>(const_cast<char *>(base) + kBaseV) : nullptr;
#pragma unroll
            for (int o = OLO; o < OHI; ++o) {
                float v;
                if (f[2]) {
                    float s = share[o * 16];
#pragma unroll
                    for (int w = 1; w < 4; ++w) s += share[w * 96 + o * 16];
                    v = fmaxf(s + reinterpret_cast<const float *>(headw + 128 * 7 * 4)[o], 0.0f);
                } else {
                    v = bv[o];
                }
                if (mode == 1) {
                    basev[o * kCells + tid] = v;
                    continue;
                }
                if (dst32) dst32[o * S + tid] = v;
                if (deferred && o >= 4) {
                    vdst[(o - 4) * S + tid] = v;
                } else if (dst16) {
                    const int k = (o < 4 ? o : o - 4) * S + tid;
                    const int step = (o < 4 ? 0 : nd.groups_act) + (k >> 4);
                    const float z = v * act3;
                    const _Float16 zh = (_Float16)z;
                    _Float16 *q = dst16 + (size_t)step * 1024 + (k & 15);
                    q[0] = zh;
                    q[512] = (_Float16)(z - (float)zh);
                }
            }
        }
        if (f[3]) map1[mypos] = zaddr;   // (every wave is behind conv3: nothing reads the maps any more)
        if (f[4]) map2[mypos] = zaddr;
        NET_TICK(11);   // features
        if (pass < 0) break;
        __syncthreads();   // the next pass rewrites maps, lists and records
    }
    return n_conv3_tiles | (n_conv2_tiles << 16);
}

// the four planes of thread `tid`'s cell (load_bits of trunk_rows_body; a base: no last move, the parity's stone count)
__device__ __forceinline__ f16x4 planes_of(const uint64_t (&ls)[8], int tid, int tm_eff, bool has_last, int lc, int par_count) {
    f16x4 cell_planes;
    const int word = (tid >> 6) & 3, bit = tid & 63;
    uint64_t w0 = 0ull, w1 = 0ull;   // (masks, not a select of array elements: rz_tree.h's word_of)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint64_t mk = word == w ? ~0ull : 0ull;
        w0 |= ls[w] & mk;
        w1 |= ls[4 + w] & mk;
    }
    const bool s0 = (w0 >> bit) & 1ull, s1 = (w1 >> bit) & 1ull;
    const bool mine = tm_eff == 0 ? s0 : s1, theirs = tm_eff == 0 ? s1 : s0;
    const _Float16 one = (_Float16)sp::kObsScale, zero = (_Float16)0.0f;
    cell_planes[0] = mine ? one : zero;
    cell_planes[1] = theirs ? one : zero;
    cell_planes[2] = (has_last && tid == lc) ? one : zero;
    cell_planes[3] = (par_count & 1) ? zero : one;
    return cell_planes;
}

// delta or not: the base's stones (rs) must be a subset of the leaf's (ls), colour by colour; the changed cells D = the added stones and
// the last move (any superset of the cells whose planes differ from the base's is correct).  Selects, no branches.  -> use_delta
__device__ __forceinline__ bool changed_cells(const uint64_t (&ls)[8], const uint64_t (&rs)[8], int nst, int tm, int lc, bool has_last, bool base_ok, int h_tm,
                                              int bw_rcp, int BW, int (&dys)[kMaxD], int (&dxs)[kMaxD], int &parity, int &nD) {
    // ---- delta or not (mode 0): the base's stones must be a subset of the leaf's, colour by colour; the changed cells D = the added
    // stones and the last move (any superset of the cells whose planes differ from the base's is correct).  Selects, no branches.
    bool use_delta = false;
    {
        bool sup = true;
        int nroot = 0;
        uint64_t D[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            sup = sup && (rs[q] & ~ls[q]) == 0ull;
            nroot += __popcll(rs[q]);
            D[q & 3] |= rs[q] ^ ls[q];
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) D[w] |= (has_last && lc >= 0 && (lc >> 6) == w) ? 1ull << (lc & 63) : 0ull;
        parity = (nst - nroot) & 1;
        nD = __popcll(D[0]) + __popcll(D[1]) + __popcll(D[2]) + __popcll(D[3]);
        use_delta = base_ok && sup && tm == (h_tm ^ parity) && nD <= kMaxD;
#pragma unroll
        for (int i = 0; i < kMaxD; ++i) {
            const bool z0 = D[0] == 0ull, z1 = D[1] == 0ull, z2 = D[2] == 0ull;
            const int w = !z0 ? 0 : !z1 ? 1 : !z2 ? 2 : 3;
            const uint64_t word = !z0 ? D[0] : !z1 ? D[1] : !z2 ? D[2] : D[3];
            const bool any = word != 0ull;
            const int cell = 64 * w + __builtin_ctzll(word | (1ull << 63));
            const uint64_t rest = word & (word - 1ull);
#pragma unroll
            for (int k = 0; k < 4; ++k) D[k] = k == w ? rest : D[k];
            const int y = (cell * bw_rcp) >> 16;
            dys[i] = any ? y : -100;
            dxs[i] = any ? cell - y * BW : -100;
        }
    }
    return use_delta;
}

template <bool TRACE>
__global__ __launch_bounds__(256, 2) void k_trunk_delta(NetDev nd, LeafBits leaves, _Float16 *__restrict__ feat16, int n_boards,
                                                        DeferredOut later, DeltaArgs da) {
    __shared__ __attribute__((aligned(16))) char lds[kLdsBytes];
    // (the grid is exactly n_boards workgroups.  Everything up to the first use of a loaded value is ONE block of unconditional
    // requests -- kernel arguments, the position, the header, the constants: a conditional load or an early return costs a memory
    // round trip of its own in the chain kernel arguments -> position -> windows -> base records, which is what a leaf waits for)
    const int board = blockIdx.x;
    const int mode = da.mode;
    const int game = mode == 1 ? board >> 1 : board, par_b = mode == 1 ? board & 1 : 0;
    unsigned long long trace_t0 = 0;
    if (TRACE) trace_t0 = rz_trace_now();
    Prof prof;
#ifdef RZ_NET_PROFILE
    for (int i = 0; i < 24; ++i) prof.acc[i] = 0;
    prof.t = __builtin_readcyclecounter();
    const long long prof_k0 = prof.t;
    long long (&prof_acc)[24] = prof.acc, &prof_t = prof.t;
#endif
    const int tid0 = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
    const int BW = nd.BW, S = nd.S;
    Layers ly;
    ly.t2p = reinterpret_cast<const char *>(nd.t2) + (size_t)wave * rt::Geo<32>::steps * 2 * 1024;
    ly.t3p = reinterpret_cast<const char *>(nd.t3) + (size_t)(2 * wave) * rt::Geo<64>::steps * 2 * 1024;
    // the head convolutions' weights: requested now, stored to LDS behind the first barrier
    f32x4 headv = tid0 < 192 ? reinterpret_cast<const f32x4 *>(nd.whp)[tid0] : reinterpret_cast<const f32x4 *>(nd.b3)[(tid0 - 192) & 31];
    {   // (threads 224 / 225: the six head biases, two floats of padding)
        const float *bh = nd.bh + (tid0 == 225 ? 4 : 0);
        const f32x4 hbv = {bh[0], bh[1], tid0 == 225 ? 0.0f : bh[2], tid0 == 225 ? 0.0f : bh[3]};
        headv = (tid0 == 224 || tid0 == 225) ? hbv : headv;
    }
    ly.k1 = nd.s_inv[2], ly.k2 = nd.s_inv[0], ly.k3 = nd.s_inv[1];
    ly.act1 = nd.s_inv[5], ly.act2 = nd.s_inv[6], ly.act3 = nd.s_inv[7];

    // ---- the position (wave-uniform: scalar loads), the header of the game's bases (read in every mode, used in mode 0), the flag
    const uint64_t *sb = leaves.stones + (size_t)game * 8;
    const BaseHdr *hd = da.hdr + game;
    uint64_t ls[8], rs[8];
    int nst = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        ls[q] = sb[q];
        rs[q] = hd->stones[q];
        nst += __popcll(ls[q]);
    }
    const int tm = leaves.to_move[game];
    const int lc_raw = (mode == 1 ? leaves.to_move : leaves.last)[game];   // (mode 1 has no last-move array: any readable word)
    const int lc = mode == 1 ? -1 : lc_raw;
    const int h_tm = hd->to_move, h_valid = hd->valid;
    const int is_active = da.active[game];
    const bool deferred = later.slot_of != nullptr;
    const int slot_ = (deferred ? later.slot_of : leaves.to_move)[deferred ? board : game];
    const int tm_eff = tm ^ par_b;        // mode 1, parity 1: the root seen by the other side, one stone later
    const int par_count = nst + par_b;
    const bool has_last = mode != 1 && nst > 0;

    Leaf leaf;
    int parity = 0, nD = 0;
    bool use_delta = changed_cells(ls, rs, nst, tm, lc, has_last, mode == 0 && h_valid != 0, h_tm, da.bw_rcp, BW, leaf.dys, leaf.dxs, parity, nD);
    leaf.base = da.recs + ((size_t)game * 2 + (mode == 1 ? par_b : parity)) * kBaseBytes;
    leaf.cell_planes = planes_of(ls, tid0, tm_eff, has_last, lc, par_count);

    // ---- where the features go (trunk_rows_body's feature stage)
    leaf.dst16 = nullptr;
    leaf.vdst = nullptr;
    if (mode != 1 && deferred) {
        leaf.dst16 = (feat16 != nullptr && slot_ < later.n_slots) ? feat16 + (size_t)slot_ * later.slot_halfs + (size_t)(board >> 5) * nd.groups_act * 1024 + (board & 31) * 16 : nullptr;
        leaf.vdst = later.valfeat + (size_t)board * later.vf_ld;
    }
    if (mode != 1 && !deferred && feat16 != nullptr)   // rz_net_delta_trunk_engine: the FC GEMM's own tiles (policy and value K-steps), as trunk_rows_body writes them
        leaf.dst16 = feat16 + ((size_t)(board >> 5) * (nd.groups_act + nd.groups_val) * 1024 + (board & 31) * 16);
    leaf.dst32 = (mode != 1 && da.feat32 != nullptr) ? da.feat32 + (size_t)board * 6 * S : nullptr;
    leaf.sets = nullptr, leaf.gtab = nullptr, leaf.leaf_lds = nullptr;
    leaf.deferred = deferred;
    leaf.store_head = true;

    {   // once per leaf: the planes' halo, the zero record; the planes themselves and the head weights behind the first barrier
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 *z = reinterpret_cast<f32x4 *>(lds);
        for (int i = tid0; i < sp::kInPieceBytes / 16; i += 256) z[i] = zero;
        if (tid0 < P2 / 16) reinterpret_cast<f32x4 *>(lds + kOffZero)[tid0] = zero;
        init_maps(lds, tid0);
    }
    if (mode == 0 && is_active == 0) return;   // (uniform; before any barrier; behind the stores above so that the flag's load is
                                               // one of the batch, not a round trip of its own at the top)
    __syncthreads();   // the zeroed halo and the default maps before the first pass writes its cells into them
    NET_TICK(0);   // requests, scalars, header, planes, zeroing
    const int n_tiles = delta_passes<false>(nd, da, lds, tid0, wave, leaf, ly, headv, use_delta, prof);
    const int n_conv3_tiles = n_tiles & 0xffff;

    if (mode == 1 && par_b == 0 && tid0 == 0) {   // the header of this game's bases (the launch behind this one reads it)
        BaseHdr *h = da.hdr + game;
#pragma unroll
        for (int q = 0; q < 8; ++q) h->stones[q] = sb[q];
        h->to_move = tm;
        h->valid = 1;
    }
    if (da.stats != nullptr && tid0 == 0 && mode != 1) {
        atomicAdd(da.stats + (use_delta ? 0 : 1), 1u);
        atomicAdd(da.stats + 2, (unsigned)n_conv3_tiles);
        atomicAdd(da.stats + 3, (unsigned)nD);
        atomicAdd(da.stats + 4, (unsigned)(n_tiles >> 16));
    }
#ifdef RZ_NET_PROFILE
    if (blockIdx.x == 0 && tid0 == 0) {
        for (int i = 0; i < 24; ++i) net_prof[i] = prof_acc[i];
        net_prof[23] = __builtin_readcyclecounter() - prof_k0;
        net_prof[22] = n_conv3_tiles;
    }
#endif
    if (TRACE && tid0 == 0) rz_trace_write(later.trace, RZ_TRACE_TRUNK, deferred ? slot_ : 0, board, trace_t0);
}

// The hand-over of k_delta_res: wave 0, behind a selection (the leaf in LDS: select_body's lds_leaf), sets the next leaf against the root
// -- changed_cells' verdict -- and, for pass -1, the cells within Chebyshev distance 1 .. 4 of its changed cells: per radius the union
// of the window table's rows of the (at most kMaxD) changed cells.  Lane 16 i + 4 (r - 1) + w reads word w of the radius-r row of
// changed cell i, two lane swaps OR the four cells' rows.  -> ws: [kWinSets] words, [kWinSets] their popcounts, the verdict.
// (the lane's word of its changed cell's rows, zero without one -> the sets, the popcounts, the verdict)
__device__ __forceinline__ void windows_store(uint64_t row, bool use_delta, int parity, int nD, int lane, uint64_t *ws) {
    unsigned lo = (unsigned)row, hi = (unsigned)(row >> 32);
    {   // (a swap leaves the lane's own value and its partner's: the OR does not care which is which)
        const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        lo = a[0] | a[1];
        hi = b[0] | b[1];
    }
    {
        const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        lo = a[0] | a[1];
        hi = b[0] | b[1];
    }
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    int *cnt = reinterpret_cast<int *>(ws + kWinSets);
    if (lane < kWinSets) {
        ws[lane] = v;
        cnt[lane] = __popcll(v);
    }
    if (lane == 0) cnt[kWinSets] = (use_delta ? 1 : 0) | (parity << 1) | (nD << 8);
}
__device__ __forceinline__ void leaf_windows(const uint64_t *leaf_lds, const uint64_t (&rs)[8], bool base_ok, int h_tm, const DeltaArgs &da, int BW,
                                             int lane, uint64_t *ws) {
    uint64_t ls[8];
    int nst = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        ls[q] = uni64(leaf_lds[q]);
        nst += __popcll(ls[q]);
    }
    const int tm = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int *>(leaf_lds + 2 * RZ_BOARD_WORDS)[0]);
    const int lc = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int *>(leaf_lds + 2 * RZ_BOARD_WORDS)[1]);
    int dys[kMaxD], dxs[kMaxD], parity = 0, nD = 0;
    const bool use_delta = changed_cells(ls, rs, nst, tm, lc, nst > 0, base_ok, h_tm, da.bw_rcp, BW, dys, dxs, parity, nD);
    const int i = lane >> 4;
    int dy = dys[0], dx = dxs[0];
#pragma unroll
    for (int j = 1; j < kMaxD; ++j) {
        dy = i == j ? dys[j] : dy;
        dx = i == j ? dxs[j] : dx;
    }
    const bool any = dy >= 0;   // (no such cell: -100)
    const uint64_t row = da.win[(any ? dy * BW + dx : 0) * kWinSets + (lane & (kWinSets - 1))];
    windows_store(any ? row : 0ull, use_delta, parity, nD, lane, ws);
}

// select_body's hook in k_delta_res: the root pre-scan's hand-over (rz_tree.h: RootPre) and, in the profile build, the selection's
// own phases (RZ_SEL_TICKS: bit i = tick i is taken -- a tick costs ~400 cycles itself, so the rows come from builds with different
// placements; a tick that is off leaves its cycles to the next one)
#if defined(RZ_NET_PROFILE) && !defined(RZ_SEL_TICKS)
#define RZ_SEL_TICKS 0
#endif
// expand_backup_from's ticks in k_delta_res (the profile build with -DRZ_BKP_TICKS=1; RZ_SEL_TICKS 0 or 1 beside it: the rows take the
// slots of the selection's ticks 1 .. 3): net_prof[8] the backup's fetches issued (behind the value layer's quarter), [13] join ->
// leaf value, [14] the expansion's bookkeeping; [17] is then the backup's stores and the barrier behind them; [22] wave 1's conv2
#if defined(RZ_NET_PROFILE) && !defined(RZ_BKP_TICKS)
#define RZ_BKP_TICKS 0
#endif
#ifdef RZ_NET_PROFILE
static_assert(!(RZ_BKP_TICKS && (RZ_SEL_TICKS & 14)), "the backup's rows stand in the slots of the selection's ticks 1 .. 3");
struct ResTick {
    static constexpr bool kOn = true;
    Prof *prof;
    __device__ __forceinline__ void tick(int i, int arrived) {
        if (RZ_BKP_TICKS) {
            asm volatile("" ::"v"(arrived));
            __builtin_amdgcn_sched_barrier(0);
            const long long now = __builtin_readcyclecounter();
            prof->acc[13 + i] += now - prof->t;
            prof->t = now;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};
#else
typedef rzt::NoTick ResTick;
#endif
struct ResHook {
    static constexpr bool kOn = true;
    rzt::RootPre *pre;
    // the leaf's changed cells against the root as the selection walks: the path's cells (depth >= 1), the root's last move (depth 0).
    // Lane 16 i + 4 (r - 1) + w asks for word w of the radius-r row of changed cell i the moment that cell is chosen -- leaf_windows'
    // lane layout --, so the rows arrive under the rest of the level, the terminal test and the leaf's stores.  (every level issues its
    // load: past kMaxD cells no lane keeps it, and a load under a branch would wait for the loads before it)
    const uint64_t *win;
    int depth;
    bool any0;
    uint64_t row;
    __device__ __forceinline__ void root_cell(int last, int stones, int lane) {
        any0 = stones > 0 && last >= 0 && last < kCells;
        row = win[(any0 ? last : 0) * kWinSets + (lane & (kWinSets - 1))];
    }
    __device__ __forceinline__ void cell(int level, int c, int lane) {
        const uint64_t v = win[c * kWinSets + (lane & (kWinSets - 1))];
        row = (lane >> 4) == level ? v : row;
    }
    // Behind the descent (select_body calls it once, whichever way the descent ended): the leaf to LDS, the hand-over of its windows --
    // the rows were requested during the descent, and the verdict is changed_cells' without the leaf: against a base that is the root
    // (base_ok) the changed cells are the path's cells -- the last move is one of them -- or, at depth 0, the root's last move (none on an
    // empty board); parity = depth & 1; more than kMaxD cells or no base: no delta -- and, inside the simulation loop (release), the
    // barrier waves 1 - 3 wait at: they start the next leaf's prologue while this wave finishes the selection (the stash, the terminal
    // test, the leaf's stores to global memory: nothing of it is read before expand_backup_body, one trunk later, by this wave).
    // (release: only for a game whose `active` flag the kernel has tested -- select_body returns in front of this call for an inactive
    // game, and the other waves would wait at the barrier for ever; k_delta_res returns on such a game before its first barrier)
    uint64_t *leaf_lds, *ws;
    bool base_ok, release;
    __device__ __forceinline__ void leaf(const uint64_t (&st)[2][rzt::kWords], int to_move, int last, int d, int lane) {
        depth = d;
        rzt::store_board<rzt::kWords>(leaf_lds, 0, st, lane);
        if (lane == 0) {
            reinterpret_cast<int *>(leaf_lds + 2 * rzt::kWords)[0] = to_move;
            reinterpret_cast<int *>(leaf_lds + 2 * rzt::kWords)[1] = last;
        }
        const bool mine = d == 0 ? (lane < 16 && any0) : (lane >> 4) < d;
        const int nD = d == 0 ? (any0 ? 1 : 0) : d;
        windows_store(mine ? row : 0ull, base_ok && nD <= kMaxD, d & 1, nD, lane, ws);
        if (release) __syncthreads();
#ifdef RZ_NET_PROFILE
        {   // -> net_prof[18]: the selection up to the release
            __builtin_amdgcn_sched_barrier(0);
            const long long now = __builtin_readcyclecounter();
            prof->acc[18] += now - prof->t;
            prof->t = now;
            __builtin_amdgcn_sched_barrier(0);
        }
#endif
    }
#ifdef RZ_NET_PROFILE
    Prof *prof;
    __device__ __forceinline__ void tick(int i, int arrived) {   // -> net_prof[2, 8, 13, 14, 15]
        if ((RZ_SEL_TICKS >> i) & 1) {
            asm volatile("" ::"v"(arrived));
            const int slot = i == 0 ? 2 : i == 1 ? 8 : 12 + i;
            __builtin_amdgcn_sched_barrier(0);
            const long long now = __builtin_readcyclecounter();
            prof->acc[slot] += now - prof->t;
            prof->t = now;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#else
    __device__ __forceinline__ void tick(int, int) {}
#endif
};

// RESIDENT SEARCH with receptive-field evaluation (rz_net_search_resident on boards of 11 .. 16 rows and columns once the base cache
// exists): k_trunk_rows_res's loop -- leaf -> trunk -> value head -> expand / backup -> next selection, n_sims times in ONE launch, one
// workgroup per game, the leaf handed over through LDS, the tree code the engine's own (rz_tree.h) -- with the delta passes as the
// trunk.  82 KB of LDS and 256 registers: TWO games per CU, so the serial tree walk of one game (one wave, ~6 us a simulation) runs
// under the other game's matrix work, and a batch of 2 x CUs games (the 512 per GPU of BASELINE.json configs[3]) is ONE launch per
// search on one stream: no lanes, no hardware-queue layout, no kernel boundary inside a search.  The bases of the roots are built
// by the launch before this one (rz_net_search_resident); the header is compared with the root once per search.
// POL = false (policy on demand, rz_net_search_resident_values): a simulation needs the two value planes only, and under the reference's
// selection rule nothing a search reads depends on a prior -- the four policy planes of a leaf are neither computed nor stored here;
// k_trunk_policy_rows forms them at the flush, for the records the flush lists.
constexpr int kResVrow = 512;
template <bool POL>
__global__ __launch_bounds__(256, 2) void k_delta_res(NetDev nd, _Float16 *__restrict__ store16, DeferredOut later, DeltaArgs da, ResArgs<true> res) {
    __shared__ __attribute__((aligned(16))) char lds[kLdsBytes];
    __shared__ float res_vrow[kResVrow];
    __shared__ float res_part[rzt::kDefWaves][rzt::kWave];
    static_assert(rzg::Split<3>::kTabEntries == 14 * 4 + 6 * 8 && rzg::Split<3>::kTabEntries <= 128 && rzg::Split<3>::kTabEntries * 2 <= rzt::kWave * 4,
                  "a gathering wave's table (104 entries) lies in its 128-entry row of the K-quarter sums");
    __shared__ __attribute__((aligned(16))) uint64_t res_leaf[2 * RZ_BOARD_WORDS + 2];
    __shared__ __attribute__((aligned(16))) uint64_t res_win[kWinLds / 8];   // leaf_windows' hand-over
    __shared__ __attribute__((aligned(16))) rzt::RootPre res_pre;            // the root pre-scan's (select_body -> wave 1 -> select_body)
    // (rz_set_playouts' order: the games with the most simulations in the first round of a grid of more than two games per CU)
    const int game = res.order != nullptr ? res.order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)game >= (unsigned)res.E.n_games || res.E.active[game] == 0) return;   // (uniform: before any barrier; an order's entry out of range: no game)
    const int n_sims = res_sims(res, game);   // the GAME's simulations (uniform: a scalar register)
    const unsigned long long clk0 = __builtin_readcyclecounter(), rt0 = __builtin_amdgcn_s_memrealtime();
    const int tid0 = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
    const int BW = nd.BW;
    Prof prof;
#ifdef RZ_NET_PROFILE
    for (int i = 0; i < 24; ++i) prof.acc[i] = 0;
    prof.t = __builtin_readcyclecounter();
    const long long prof_k0 = prof.t;
    long long (&prof_acc)[24] = prof.acc, &prof_t = prof.t;
#endif
    Layers ly;
    ly.t2p = reinterpret_cast<const char *>(nd.t2) + (size_t)wave * rt::Geo<32>::steps * 2 * 1024;
    ly.t3p = reinterpret_cast<const char *>(nd.t3) + (size_t)(2 * wave) * rt::Geo<64>::steps * 2 * 1024;
    f32x4 headv = tid0 < 192 ? reinterpret_cast<const f32x4 *>(nd.whp)[tid0] : reinterpret_cast<const f32x4 *>(nd.b3)[(tid0 - 192) & 31];
    {
        const float *bh = nd.bh + (tid0 == 225 ? 4 : 0);
        const f32x4 hbv = {bh[0], bh[1], tid0 == 225 ? 0.0f : bh[2], tid0 == 225 ? 0.0f : bh[3]};
        headv = (tid0 == 224 || tid0 == 225) ? hbv : headv;
    }
    ly.k1 = nd.s_inv[2], ly.k2 = nd.s_inv[0], ly.k3 = nd.s_inv[1];
    ly.act1 = nd.s_inv[5], ly.act2 = nd.s_inv[6], ly.act3 = nd.s_inv[7];
    const int slot0 = res.E.pend[game];
    // the root (it does not move inside a search) against the header of the game's bases: once
    uint64_t rs[8];
    bool base_ok = da.hdr[game].valid != 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        rs[q] = res.E.root_stones[(size_t)game * 8 + q];
        base_ok = base_ok && da.hdr[game].stones[q] == rs[q];
    }
    const int h_tm = res.E.root_to_move[game];
    base_ok = base_ok && da.hdr[game].to_move == h_tm;
    {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 *z = reinterpret_cast<f32x4 *>(lds);
        for (int i = tid0; i < sp::kInPieceBytes / 16; i += 256) z[i] = zero;
        if (tid0 < P2 / 16) reinterpret_cast<f32x4 *>(lds + kOffZero)[tid0] = zero;
        init_maps(lds, tid0);
        for (int i = tid0; i < kResVrow; i += 256) res_vrow[i] = 0.0f;
    }
    if (tid0 == 0) res_pre.scan = res_pre.valid = res_pre.answered = 0;   // (no stash yet: a select_first == 0 launch's first selection was not made here)
    ResHook hook;
    hook.pre = &res_pre;
    hook.win = da.win;
    hook.depth = 0;
    hook.any0 = false;
    hook.row = 0ull;
    hook.leaf_lds = res_leaf;
    hook.ws = res_win;
    hook.base_ok = base_ok;
    hook.release = false;   // (the first selection: every wave meets the barrier behind it)
#ifdef RZ_NET_PROFILE
    hook.prof = &prof;
    long long pre_cycles = 0, pre_wait = 0;   // wave 1: the pre-scan, the barrier behind it (= its slack under expand + backup)
#endif
    if (res.select_first == 0 && tid0 == 0) {   // the first leaf was selected by rz_select_step: from the engine's leaf arrays
#pragma unroll
        for (int q = 0; q < 8; ++q) res_leaf[q] = res.E.leaf_stones[(size_t)game * 8 + q];
        reinterpret_cast<int *>(res_leaf + 2 * RZ_BOARD_WORDS)[0] = res.E.leaf_to_move[game];
        reinterpret_cast<int *>(res_leaf + 2 * RZ_BOARD_WORDS)[1] = res.E.leaf_last[game];
    }
    __syncthreads();
    if (wave == 0) {
        // AlphaZeroMCTS._playout's select loop for the first simulation of the search (rz_select_step's work), or its leaf from
        // rz_select_step; either way the hand-over of the first leaf's windows
        const int lane0 = tid0 & 63;
        if (res.select_first != 0) {
            rzt::select_body<false, rzt::kWords, ResHook>(res.E, nullptr, game, lane0, 0, res_leaf, &hook);   // (the hand-over: hook.leaf)
        } else {
            leaf_windows(res_leaf, rs, base_ok, h_tm, da, BW, lane0, res_win);
        }
    }
    __syncthreads();
    int tiles_total = 0, tiles2_total = 0, deltas = 0, cells_total = 0;
    for (int sim = 0; sim < n_sims; ++sim) {
        // (the thread's number is opaque per simulation: hipcc otherwise hoists the tree code's lane-dependent addresses out of this
        // loop and spills them)
        int tid_s = tid0;
        asm volatile("" : "+v"(tid_s));
        // ---- the verdict and the window sets of pass -1 from the selection's hand-over (ResHook::leaf, leaf_windows).  The leaf itself
        // (LDS: res_leaf) is read where its planes are formed: by wave 0 in pass -1, by every thread in the passes without a base.
        // Waves 1 .. 3 are here as soon as the leaf's cell is chosen -- wave 0 follows behind the selection's tail and meets them at the
        // barrier before conv2.
        const int verdict = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int *>(res_win + kWinSets)[kWinSets]);
        bool use_delta = (verdict & 1) != 0;
        const int parity = (verdict >> 1) & 1, nD = verdict >> 8;
        Leaf leaf;
        leaf.sets = res_win;
        leaf.gtab = reinterpret_cast<uint16_t *>(res_part[wave]);   // (the K-quarter sums: dead from the selection to the value layer)
#pragma unroll
        for (int i = 0; i < kMaxD; ++i) leaf.dys[i] = leaf.dxs[i] = -100;   // (pass -1 reads the sets; the passes without a base, no cells)
        leaf.base = da.recs + ((size_t)game * 2 + parity) * kBaseBytes;
        leaf.leaf_lds = res_leaf;
        // the game's slot advances by one per simulation (expand_backup_body<DEF>); the value inputs stay in LDS
        leaf.dst16 = POL && slot0 + sim < later.n_slots ? store16 + (size_t)(slot0 + sim) * later.slot_halfs + (size_t)(game >> 5) * nd.groups_act * 1024 + (game & 31) * 16 : nullptr;
        leaf.vdst = res_vrow;
        leaf.dst32 = nullptr;
        leaf.deferred = true;
        leaf.store_head = sim == 0;
        NET_TICK(0);
        const int n_tiles = delta_passes<true, POL ? 0 : 4, 6>(nd, da, lds, tid_s, wave, leaf, ly, headv, use_delta, prof);
        tiles_total += n_tiles & 0xffff;
        tiles2_total += n_tiles >> 16;
        deltas += use_delta ? 1 : 0;
        cells_total += nD;
        __syncthreads();   // the value head's inputs are complete; the shares are read
        NET_TICK(12);
        // ---- the rest of the simulation, by the same workgroup (k_tree_step_def's body: rz_tree.h), as in trunk_rows_body
        const int lane = tid_s & 63;
        if (RZ_DELTA_TREE_PRIO) __builtin_amdgcn_s_setprio(RZ_DELTA_TREE_PRIO);   // (the serial part of a simulation: ahead of the other game's trunk waves at issue)
        const bool more = sim + 1 < n_sims;
        const auto value_quarter = [&]() {
            if (res.vh.groups == 128) rzt::value_quarter_lds<16>(res.vh, res_vrow, lane, wave, res_part);
            else rzt::value_quarter_lds<8>(res.vh, res_vrow, lane, wave, res_part);
        };
        constexpr bool kBackupDeferred = true;   // expand_backup's DEF in BOTH calls below (what the early root fetch relies on)
        if (wave == 0) {
            // Wave 0, the game's: its quarter of the value layer, expand + backup, the next selection -- ONE region, so that what is asked
            // for a phase early and its uses stand together.  RZ_DELTA_EARLY: the backup's leaf state (written by this wave's selection a
            // trunk ago) is requested in front of the quarter and arrives under the quarter's weight loads; the records of the path's
            // nodes are requested behind the quarter and travel under the join, the hidden sum, tanh and the expansion's bookkeeping.
            if (RZ_DELTA_EARLY & 1) {
                const rzt::BackupLeaf bl = rzt::backup_leaf_fetch<false, true>(res.E, game, lane);
                value_quarter();
                NET_TICK(16);
                const rzt::PathRecs recs = rzt::backup_path_fetch(res.E, game, lane, bl);
#ifdef RZ_NET_PROFILE
                if (RZ_BKP_TICKS) NET_TICK(8);   // the path's records requested (not their arrival)
                ResTick btick;
                btick.prof = &prof;
                ResTick *tk = &btick;
#else
                ResTick *tk = nullptr;
#endif
                rzt::expand_backup_from<float, false, false, false, kBackupDeferred, rzt::kWords, rzt::PathRecs, ResTick>(res.E, nullptr, nullptr, game, lane, bl, recs,
                                                                                                               rz_raw_heads(), 0, res.vh, res_part, tk);
            } else {
                value_quarter();
                NET_TICK(16);
                rzt::expand_backup_body<float, false, false, false, kBackupDeferred>(res.E, nullptr, nullptr, game, lane, rz_raw_heads(), 0, res.vh, res_part);
            }
            // The next selection.  Its hook meets the RELEASE barrier the moment the leaf's cell is chosen, the leaf and its window sets in LDS
            // (ResHook::leaf); waves 1 .. 3 wait for nothing else and go on to the next leaf's prologue, wave 0 finishes the selection
            // beside them.  (res_leaf / res_win: written before the release, rewritten by the next selection, at least three barriers on;
            // res_pre: the tail's stash is read by wave 1 behind the barrier inside expand_backup_body; the gather tables: rows 1 .. 3 of
            // res_part, which the tail does not touch.)  The last simulation: no selection, no barrier, for anyone.
            if (more) {
                hook.depth = 0, hook.any0 = false, hook.row = 0ull;   // (nothing of the last selection's is kept)
                hook.release = true;
                // (the lane number opaque once more: what the selection derives from it is not worked out at the top of the simulation
                // and kept -- spilled -- across the trunk)
                int lane_t = lane;
                asm volatile("" : "+v"(lane_t));
                if (RZ_DELTA_EARLY & 2) {
                    // (top[g] in particular: the backup in front of this fetch is the one with deferred priors, whose expansion is never
                    // dense -- `dense = !DEF && ...` in expand_backup_from --, so only this wave's own selection tail stores to it)
                    static_assert(kBackupDeferred, "the root fetch in front of the barrier: no dense expansion may move top[g] behind it");
                    // the selection's root state -- arena, top, root position, window: words neither the backup with deferred priors nor
                    // the pre-scan stores to (top[g]: only this wave's own selection tail) -- requested in front of the barrier: it
                    // travels with the backup's store acknowledgements.  Behind the barrier stay what the backup and wave 1 write: the
                    // stash (LDS), the root's record and child r's.
                    const rzt::SelectRoot root = rzt::select_root_fetch<rzt::kWords>(res.E, game, lane_t);
                    __syncthreads();   // the tree's updates before the selection's record loads; the pre-scan's answer
                    NET_TICK(17);
                    rzt::select_body_from<false, rzt::kWords, ResHook>(res.E, nullptr, game, lane_t, root, 0, res_leaf, &hook);
                } else {
                    __syncthreads();   // the tree's updates before the selection's loads; the pre-scan's answer
                    NET_TICK(17);
                    rzt::select_body<false, rzt::kWords, ResHook>(res.E, nullptr, game, lane_t, 0, res_leaf, &hook);
                }
                NET_TICK(15);   // wave 0: the selection's tail, behind the release
            } else {
                __syncthreads();
                NET_TICK(17);
            }
        } else {
            value_quarter();
            NET_TICK(16);
            __syncthreads();   // (the barrier inside the body, where the quarters meet)
            // wave 1, idle until the next barrier: the root's siblings for the next selection (it reads the tree, it writes LDS)
            if (RZ_DELTA_PRESCAN && wave == 1 && more) {
#ifdef RZ_NET_PROFILE
                const long long t0 = __builtin_readcyclecounter();
#endif
                rzt::root_prescan<rzt::kWords>(res.E, game, lane, &res_pre);
#ifdef RZ_NET_PROFILE
                __builtin_amdgcn_s_waitcnt(0);
                const long long t1 = __builtin_readcyclecounter();
                pre_cycles += t1 - t0;
                pre_wait -= t1;
#endif
            }
            __syncthreads();        // (wave 0: behind the backup) the pre-scan's answer
#ifdef RZ_NET_PROFILE
            if (RZ_DELTA_PRESCAN && wave == 1 && more) pre_wait += __builtin_readcyclecounter();
#endif
            NET_TICK(17);
            if (more) {
                __syncthreads();   // the release
                NET_TICK(18);
            }
        }
        if (RZ_DELTA_TREE_PRIO) __builtin_amdgcn_s_setprio(0);
    }
    if (da.stats != nullptr && tid0 == 0) {
        atomicAdd(da.stats + 0, (unsigned)deltas);
        atomicAdd(da.stats + 1, (unsigned)(n_sims - deltas));
        atomicAdd(da.stats + 2, (unsigned)tiles_total);
        atomicAdd(da.stats + 3, (unsigned)cells_total);
        atomicAdd(da.stats + 4, (unsigned)tiles2_total);
        atomicAdd(da.stats + 5, (unsigned)res_pre.answered);
        if (game == 0) {   // the clock this search ran at: cycles / (ticks x 10 ns)
            da.stats[6] = (unsigned)((__builtin_readcyclecounter() - clk0) >> 8);
            da.stats[7] = (unsigned)(__builtin_amdgcn_s_memrealtime() - rt0);
        }
    }
#ifdef RZ_NET_PROFILE
    if (blockIdx.x == 0 && tid0 == 0) {
        for (int i = 0; i < 24; ++i)
            if (i != 19 && i != 20 && i != 21 && !(RZ_BKP_TICKS && i == 22)) net_prof[i] = prof_acc[i];
        net_prof[23] = __builtin_readcyclecounter() - prof_k0;
        if (!RZ_BKP_TICKS) net_prof[22] = tiles_total;
    }
    if (blockIdx.x == 0 && tid0 == 64) {   // wave 1's first lane: the pre-scan and the wait behind it
        if (RZ_BKP_TICKS) net_prof[22] = prof_acc[7];   // (its conv2, in the place of the tile count)
        net_prof[19] = pre_cycles;
        net_prof[20] = pre_wait;
        net_prof[21] = prof_acc[0] + prof_acc[1] + prof_acc[3];   // ... from the release to the barrier before conv2 (its arrival there)
    }
#endif
}

// POLICY ON DEMAND, the flush's side: the four policy planes of the LISTED records of a search made by k_delta_res<false>, written to the
// record's own place in the feature store (slot rows[i] / n_games, the game's tile and column: where k_delta_res<true> writes them
// during the search), so that k_heads_rows and k_deferred_priors_rows run behind it unchanged.  A record holds the leaf (stones, side to
// move, last move: rzt::pend_lw); the leaf is evaluated as k_trunk_delta evaluates one -- changed_cells against the header of the game's
// bases, delta_passes<false> -- for outputs 0 .. 3: the same code on the same leaf against the same base, hence the same bits.  A stale
// or missing base, or more than kMaxD changed cells: the four passes without a base.  Fixed grid (two workgroups per CU), the count is
// the device's.  It counts nothing in da.stats: those are the leaves of searches.
struct PolicyRows {
    const int32_t *rows, *count;   // the records (slot * n_games + game), their number
    const uint64_t *stones;        // [record][2][RZ_BOARD_WORDS]
    const int32_t *lw;             // [record] rzt::pend_lw_pack(side to move, last move)
    int n_games, n_slots;
    long long slot_halfs;          // halves per slot of the store
};
__global__ __launch_bounds__(256, 2) void k_trunk_policy_rows(NetDev nd, _Float16 *__restrict__ store16, DeltaArgs da, PolicyRows pr) {
    __shared__ __attribute__((aligned(16))) char lds[kLdsBytes];
    const int tid0 = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
    const int BW = nd.BW;
    Prof prof;
#ifdef RZ_NET_PROFILE
    for (int i = 0; i < 24; ++i) prof.acc[i] = 0;
    prof.t = __builtin_readcyclecounter();
#endif
    Layers ly;
    ly.t2p = reinterpret_cast<const char *>(nd.t2) + (size_t)wave * rt::Geo<32>::steps * 2 * 1024;
    ly.t3p = reinterpret_cast<const char *>(nd.t3) + (size_t)(2 * wave) * rt::Geo<64>::steps * 2 * 1024;
    f32x4 headv = tid0 < 192 ? reinterpret_cast<const f32x4 *>(nd.whp)[tid0] : reinterpret_cast<const f32x4 *>(nd.b3)[(tid0 - 192) & 31];
    {
        const float *bh = nd.bh + (tid0 == 225 ? 4 : 0);
        const f32x4 hbv = {bh[0], bh[1], tid0 == 225 ? 0.0f : bh[2], tid0 == 225 ? 0.0f : bh[3]};
        headv = (tid0 == 224 || tid0 == 225) ? hbv : headv;
    }
    ly.k1 = nd.s_inv[2], ly.k2 = nd.s_inv[0], ly.k3 = nd.s_inv[1];
    ly.act1 = nd.s_inv[5], ly.act2 = nd.s_inv[6], ly.act3 = nd.s_inv[7];
    const int n_rows = pr.count[0];
    {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 *z = reinterpret_cast<f32x4 *>(lds);
        for (int i = tid0; i < sp::kInPieceBytes / 16; i += 256) z[i] = zero;
        if (tid0 < P2 / 16) reinterpret_cast<f32x4 *>(lds + kOffZero)[tid0] = zero;
        init_maps(lds, tid0);
    }
    __syncthreads();
    bool first = true;
    for (int i = blockIdx.x; i < n_rows; i += gridDim.x) {
        // (the thread's number is opaque per row, as per pass and per simulation: hipcc otherwise hoists the lane-dependent addresses)
        int tid_r = tid0;
        asm volatile("" : "+v"(tid_r));
        // ---- the record (wave-uniform), the header of its game's bases: one block of unconditional requests
        const int rec = pr.rows[i];
        const int game = rec % pr.n_games, slot = rec / pr.n_games;
        const uint64_t *sb = pr.stones + (size_t)rec * 8;
        const BaseHdr *hd = da.hdr + game;
        uint64_t ls[8], rs[8];
        int nst = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            ls[q] = sb[q];
            rs[q] = hd->stones[q];
            nst += __popcll(ls[q]);
        }
        const int lw = pr.lw[rec];
        const int h_tm = hd->to_move, h_valid = hd->valid;
        const int tm = rzt::pend_lw_to_move(lw), lc = rzt::pend_lw_last(lw);
        const bool has_last = nst > 0;
        if ((unsigned)slot >= (unsigned)pr.n_slots) continue;   // (uniform; a record beyond the store has no features: never listed)
        Leaf leaf;
        int parity = 0, nD = 0;
        bool use_delta = changed_cells(ls, rs, nst, tm, lc, has_last, h_valid != 0, h_tm, da.bw_rcp, BW, leaf.dys, leaf.dxs, parity, nD);
        leaf.base = da.recs + ((size_t)game * 2 + parity) * kBaseBytes;
        leaf.cell_planes = planes_of(ls, tid_r, tm, has_last, lc, nst);
        leaf.dst16 = store16 + (size_t)slot * pr.slot_halfs + (size_t)(game >> 5) * nd.groups_act * 1024 + (game & 31) * 16;
        leaf.vdst = nullptr;
        leaf.dst32 = nullptr;
        leaf.sets = nullptr, leaf.gtab = nullptr, leaf.leaf_lds = nullptr;
        leaf.deferred = false;
        leaf.store_head = first;
        first = false;
        (void)delta_passes<false, 0, 4>(nd, da, lds, tid_r, wave, leaf, ly, headv, use_delta, prof);
        __syncthreads();   // the next row rewrites planes, maps, lists and records
    }
}

}  // namespace dl

}  // namespace
