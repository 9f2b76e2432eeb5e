// rz_net_dev.h -- what every kernel family of rz_net.hip takes: the vector types, the halo planes' constants, the records a launch
// hands to a kernel (NetDev, LeafBits, ResArgs, DeferredOut) and the profile build's NET_TICK.  No kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rlzero_hip.h"
#include "rz_tree.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kRowW = 18;     // halo row width (x = -1 .. 16)
// halo rows: 18 (y = -1 .. 16), 18*18 = 324 floats per plane before padding
// plane stride (floats): 18*18 = 324 padded.  Direct kernel: 336 = 16 mod 32, so the 4 channel
// sub-groups of a fragment read hit disjoint banks.  Winograd kernel: 337 (odd) -- see wino_conv.
constexpr int kPlaneDirect = 336, kPlaneWino = 337;
constexpr int kPlanesIn = 4, kPlanesC1 = 32, kPlanesC2 = 64, kPlanes = kPlanesIn + kPlanesC1 + kPlanesC2;
constexpr int kTrunkThreads = 512;

struct NetDev {
    const f32x4 *w1, *w2, *w3;   // packed [tile][cin_step][3][64 lanes] x 4 taps
    const f32x4 *u2f, *u3f;      // F(4x4,3x3): [tile][pass][cin_step][3][64 lanes] x 4 components (pack_wino_f4)
    const f32x4 *s1;             // conv1 for k_trunk_split: [kernel row][hi | lo][64 lanes] x 8 f16 (pack_split1)
    const f32x4 *s2, *s3;        // split f16 weights: [32-channel tile][tap][16-channel chunk][hi | lo][64 lanes] x 8 f16
    const f32x4 *t2, *t3;        // the same for k_trunk_rows: [16-channel tile][tap][32-channel chunk][hi | lo][64 lanes] x 8 f16 (pack_rows)
    const f32x4 *t3f;            // conv3 for the FP8 cross terms (RZ_NET_SPLIT_F16_FP8): [16-channel tile][tap][part][half][64 lanes] x 16 bytes
                                 // (pack_rows_f8: part 0 = the hi f16 pieces of the tap's two chunks, part 1 = e4m3 bytes [lo 2^5 | hi 2^-6])
    const float *s_inv;          // [8] in device memory (a captured launch must see a reload's values), with a1, a2, a3 =
                                 // the activation scales of conv1's / conv2's outputs and of the head features (powers of
                                 // two from rz_net_load's activation bounds), sw* the weight scales:
                                 // [0] a2 / (a1 sw2), [1] 1 / (a2 sw3), [2] a1 / (16 sw1), [3] 1 / (a3 sw_act_fc1),
                                 // [4] 1 / (a3 sw_val_fc1), [5] a1, [6] a2, [7] a3
    const f32x4 *fs_act, *fs_val;  // split f16 FC weights: [32-output tile][K-step of 16][hi | lo][64 lanes] x 8 f16 (+ a zero step)
    const float *b1, *b2, *b3;   // conv biases
    const float *wh;             // [6][128]: act_conv1 (4 rows) then val_conv1 (2 rows)
    const float *whp;            // the same, [128][6] (k_trunk_split)
    const float *bh;             // [6]
    const float *fc_act_w;       // act_fc1.weight [out][in], zero padded to [Npad][16*groups_act]
    const float *fc_act_b;       // [Npad]
    const float *fc_val1_w;      // val_fc1.weight [out][in], zero padded to [64][16*groups_val]
    const float *fc_val1_b;      // [64]
    const float *fc_val2_w;      // [64]
    const float *fc_val2_b;      // [1]
    // head features of a board: policy inputs at [0, 4S), value inputs at [feat_val_off, +2S) of a row of
    // feat_ld floats.  A caller's buffer is the natural [board][6S]; the internal one pads both ranges
    // to multiples of 16 (zero filled) so the FC GEMM reads aligned 16-byte fragments.
    int feat_ld, feat_val_off;
    int BH, BW, S, A, Npad, groups_act, groups_val;  // A policy outputs (Npad: padded to 32); groups_*: K / 16
    // k_trunk_split: an N-tile (32 MFMA columns) = tile_rows board rows x tile_cols columns, position n of a tile =
    // (n / tile_cols, n % tile_cols) with n / tile_cols = (n * tile_rcp) >> 16; (2, 16) for boards that need 5 .. 8
    // tiles, (32 / width, width) when 4 tiles of that shape cover the board (9x9: 3 x 9, Connect4: 4 x 7)
    int tile_rows, tile_cols, tile_rcp;
};

// The leaf positions themselves (rz_net_trunk_leaves): bitboards [board][2 colours][4 words], side to move and last
// cell, exactly what the tree kernels keep per leaf.  The trunk then builds the four observation planes of
// GomokuEnv.current_state (gomoku_env.py:95-114) itself -- thread t = cell t: stones of the side to move, of the other
// side, the last move (if any stone is on the board), ones if the stone count is even -- so the tree kernel need not
// write, and this kernel need not read, 16 S bytes of 0.0 / 1.0 floats per leaf.
struct LeafBits {
    const uint64_t *stones;
    const int32_t *to_move;
    const int32_t *last;
};

// Development aid (not built by default): -DRZ_NET_PROFILE accumulates the shader-clock cycles wave 0 of workgroup 0 spends in
// each phase of a board in k_trunk_split into net_prof[] (rz_net_debug_profile).
#ifdef RZ_NET_PROFILE
__device__ long long net_prof[24];   // [16 .. 19]: the resident search's tree phases (value head, expand / backup, selection, planes)
#define NET_TICK(i) do { __builtin_amdgcn_sched_barrier(0); const long long now_ = __builtin_readcyclecounter(); prof_acc[i] += now_ - prof_t; prof_t = now_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define NET_TICK(i)
#endif

// RESIDENT SEARCH (RES instantiations of the trunk kernels; rz_net_search_resident).  For a batch of at most one game per CU the whole
// chain of a search lives in ONE workgroup per game and ONE launch: trunk -> value head -> expand / backup -> next selection, n_sims
// times, the leaf handed from the tree code to the trunk through LDS, the value head's inputs never leaving the CU, the trunk's
// prologue (weights into registers, LDS zeroing) paid once per launch instead of once per simulation, no kernel boundary inside a
// search.  The tree code is the engine's own (rz_tree.h: the bodies of k_tree_step_def), the policy features go to the deferred
// store like in the two-launch step, so trees, priors and values are those of that route bit for bit.
#ifndef RZ_SPLIT_TREE_PRIO
#define RZ_SPLIT_TREE_PRIO 1   // k_trunk_split<RES> on the compact grid (two games per CU): issue priority of the tree phase
#endif
template <bool RES> struct ResArgs {};
template <> struct ResArgs<true> {
    rzt::Dev E;          // the engine's device view (rz_device_view)
    rz_value_head vh;    // valfeat unused: the inputs stay in LDS
    int n_sims;          // simulations of this launch: n_sims x (trunk, expand / backup), a selection between two of them
    int select_first;    // != 0: the launch begins with the selection of the first leaf itself (no rz_select_step before it)
    // rz_set_playouts (NULL: every game runs n_sims): game g runs min(sims_of[g], n_sims) simulations -- n_sims stays the launch's
    // maximum, the store slots pend[g] .. pend[g] + n_sims - 1 stay reserved for it; `order` (k_delta_res only, NULL: identity):
    // workgroup b searches game order[b]
    const int32_t *sims_of;
    const int32_t *order;
};
// the simulations of `game`'s workgroup: one load from a uniform address, once per workgroup
__device__ __forceinline__ int res_sims(const ResArgs<false> &, int) { return 0; }
__device__ __forceinline__ int res_sims(const ResArgs<true> &r, int game) {
    if (r.sims_of == nullptr) return r.n_sims;
    const int n = __builtin_amdgcn_readfirstlane(r.sims_of[game]);
    return n < r.n_sims ? n : r.n_sims;
}

// Deferred priors (rz_value_head, include/rlzero_hip.h): where a board's features go when no FC GEMM follows the trunk -- the policy
// pieces into slot slot_of[board] of a store of `slot_halfs` f16 values per slot (tiles of groups_act K-steps), the value head's
// inputs as f32 rows of vf_ld floats.  slot_of == nullptr: the ordinary route.
struct DeferredOut {
    const int32_t *slot_of;
    long long slot_halfs;
    float *valfeat;
    int vf_ld;
    unsigned long long *trace;   // rz_trace.h (NULL: none)
    int n_slots;                 // slots of the store: a leaf whose slot lies beyond it is NOT stored (the tree step flags the game)
};

// The lane reduction of the head sums, shared by the Winograd trunk (rz_net_f32.h, the rest of namespace f4), the row trunk and
// the delta kernels, which keep its order of additions.
namespace f4 {
// Sum `vals` over the 4 lanes {n, n+16, n+32, n+48}: every lane ends with 24 of the 96 sums,
// out[i] = sum of vals[(q & 1) * 48 + (q >> 1) * 24 + i], q = lane >> 4.
__device__ __forceinline__ void reduce_scatter_96(const float (&vals)[96], float (&out)[24]) {
    float r1[48];
#pragma unroll
    for (int i = 0; i < 48; ++i) {
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(vals[i]), __float_as_uint(vals[48 + i]),
                                                         false, false);
        r1[i] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
#pragma unroll
    for (int i = 0; i < 24; ++i) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r1[i]), __float_as_uint(r1[24 + i]),
                                                         false, false);
        out[i] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
}
}  // namespace f4

}  // namespace
