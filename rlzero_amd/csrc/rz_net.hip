// rz_net.hip -- fused forward of the AlphaZero policy-value network on MI355X (gfx950), f32 results.
//
// Replaces PolicyValueNet.forward (rlzero/games/gomoku/policy_value_net.py:34-52) for the
// batch of MCTS leaves: the one dense contraction of the path (42.8 MFLOP per
// 15x15 position, MFMA-bound).  The default trunk carries f32 operands as hi + lo f16 pairs on the f16 matrix
// pipe (three MFMAs per product, f32 accumulation: as accurate as the exact-f32 kernel) and so does the FC GEMM
// behind it; the other trunks and their FC GEMM use v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain (tolerance vs
// the reference's CPU output: 1e-4).
//
// This file is the host side of ONE translation unit: the kernels lie in headers beside it, one per family, each of which compiles
// alone (tests/test_csrc_headers.py) and describes its kernels and their design where they are defined.  One workgroup owns a board;
// its activations never leave the CU.
//   rz_net_dev.h     what every family takes: the vector types, NetDev, LeafBits, ResArgs, DeferredOut, NET_TICK (-DRZ_NET_PROFILE)
//   rz_net_rows.h    k_trunk_rows<NT> (default, boards of 11 .. 16 rows and columns): conv1..conv3 as direct convolutions on the f16
//                    matrix pipe, every f32 operand a hi + lo pair of f16 values: v_mfma_f32_16x16x32_f16, one N-tile per board row,
//                    the four waves split the OUTPUT CHANNELS; k_trunk_rows_res<NT>: the same body as a resident search; namespace rt
//   rz_delta.h       k_trunk_delta, k_delta_res, k_trunk_policy_rows: k_trunk_rows' arithmetic on the cells a leaf changes (namespace dl)
//   rz_net_split.h   k_trunk_split<TN, MS> (smaller boards; the checker of k_trunk_rows): the same arithmetic on v_mfma_f32_32x32x16_f16
//                    tiles of whole rows, the waves split the rows; optionally the FC layers of its own board behind it
//                    (RZ_NET_HEADS_IN_TRUNK) and the resident search (under PUCT both at once: rz_net_search_resident_puct); namespace sp,
//                    whose types and conversions every f16 kernel uses
//   rz_net_heads.h   k_heads_split, k_heads_rows, k_heads_part: the first FC layers of both heads on the f16 pipe (hi + lo pairs), fed
//                    by the f16 feature pieces the trunks above write in MFMA fragment order; k_heads_finish: log_softmax and tanh
//   rz_net_f32.h     the f32-input MFMA: k_trunk (direct implicit GEMM, bit-for-bit a k-ordered fmaf chain), k_trunk_wino_f4<4>
//                    (conv2 / conv3 as Winograd F(4x4,3x3), namespace f4), k_heads_gemm (the FC layers in 32 x 32 output blocks)
// The launch_* functions below are the only place that names template instantiations.
//
// Host side (from `struct rz_net` on): the C ABI's entry points.  What rz_net_load computes before it uploads -- the fragment layouts
// the kernels above read, the weight and activation scales, the e4m3 bytes -- is rz_pack.h (no HIP, tested on the CPU:
// tests/test_net_pack.py); the records handed to the kernels (value head, store, delta arguments) are each built by one helper
// beside net_ready, and every device buffer is a DevBuf the net owns.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

#include "rlzero_hip.h"
#include "rz_host.h"
#include "rz_pack.h"
#include "rz_trace.h"
#include "rz_tree.h"
#include "rz_gather.h"
#include "rz_window.h"

// (this order is the order of the kernels in the code object)
#include "rz_net_dev.h"
#include "rz_net_split.h"
#include "rz_net_rows.h"
#include "rz_delta.h"
#include "rz_net_f32.h"
#include "rz_net_heads.h"

struct rz_net {
    int board_size = 0, device = 0;
    bool loaded = false;
    bool split_ok = true;        // rz_net_load found finite activation bounds: the split-f16 trunk cannot overflow
    float range_info[8] = {0};   // rz_net_range_info
    int algo = RZ_NET_SPLIT_F16;
    bool fp8_cross = false;      // RZ_NET_SPLIT_F16_FP8: algo stays RZ_NET_SPLIT_F16, conv3's cross terms run on the FP8 pipe (position-fed launches)
    int n_cus = 256;
    int max_wgs = 0;  // rz_net_set_max_workgroups: 0 = one persistent trunk workgroup per CU
    // small boards: k_trunk_split on the compact LDS grid, two workgroups per CU, for launches of more boards than HALF the CUs -- more
    // boards than CUs run in one round instead of two, and of two lanes with up to a CU's worth of boards each both trunks are on the
    // chip together (Connect4 512 games on two lanes 21.1 -> 21.8 M, 6 x 6 +7 %; four lanes of 128 boards: 3 % slower, hence the half).
    // RZ_NET_COMPACT=0: never, 2: whenever the geometry allows
    bool compact_grid = true;
    bool compact_always = false;
    NetDev dev;
    std::vector<DevBuf<char>> allocs;   // the parameter buffers, in rz_net_load's order
    size_t upload_cursor = 0;
    DevBuf<float> d_feat, d_raw, d_hid;
    DevBuf<_Float16> d_feat16;     // the features as hi + lo f16 pieces in fragment order (k_trunk_split -> k_heads_split)
    bool feat16_valid = false;     // the last trunk launch into the internal buffer wrote d_feat16
    bool feat32_valid = false;     // ... wrote d_feat (the split-f16 trunk skips it when the GEMM reads the f16 pieces)
    int heads_algo = RZ_NET_HEADS_AUTO;
    int raw_parts = 1;           // what the last launch_heads_gemm left in d_raw / d_hid: 1 = final, 4 = K-quarter sums
    bool raw_from_trunk = false; // the last trunk launch ran the FC layers itself (k_trunk_split, FC_HERE): d_raw / d_hid are final
    size_t raw_part_floats = 0, hid_part_floats = 0;  // stride between the parts
    DevBuf<unsigned> d_flags;
    long long feat_boards = 0;
    size_t feat_floats = 0;
    // deferred priors (rz_net_deferred_reserve): the policy-feature store, the logits of a flush, the value head's inputs
    DevBuf<_Float16> d_store16;
    DevBuf<float> d_store_raw, d_valfeat;
    const float *d_w1t = nullptr;        // val_fc1.weight as [groups][64][4] (rz_value_head; one of `allocs`)
    int vf_groups = 0;                    // K / 4 of the value head's first layer, padded to a multiple of 4
    int store_slots = 0, store_tiles = 0; // slots x 32-board tiles per slot
    unsigned long long *d_trace = nullptr; // rz_net_trace_attach
    long long store_boards = 0;
    // receptive-field leaf evaluation (rz_delta.h; rz_net_delta_*): the base cache of `base_games` games
    DevBuf<dl::BaseHdr> d_base_hdr;
    DevBuf<char> d_base_recs;
    DevBuf<unsigned> d_delta_stats;
    DevBuf<uint8_t> d_base_ones;      // [base_games] of 1: the `active` flags of a caller that has none
    DevBuf<uint64_t> d_win;           // the window table of the net's board (rz_window.h; the board is fixed per net): k_delta_res
    int base_games = 0;
    bool delta_resident = true;       // rz_net_delta_resident: rz_net_search_resident runs k_delta_res where the cache allows
};

namespace {

// Parameter buffers are allocated by the first rz_net_load and REUSED by later ones (same shapes, same
// order), so device pointers captured in hipGraphs stay valid across weight updates.
template <typename T>
int net_upload(rz_net *net, const float *host, size_t count, const T **out) {
    const size_t bytes = count * sizeof(float);
    if (net->upload_cursor < net->allocs.size()) {
        if (net->allocs[net->upload_cursor].bytes != bytes) return rz_fail(RZ_ERR_ARG, "parameter size changed between loads");
    } else {
        DevBuf<char> fresh;
        if (!fresh.alloc(bytes)) return rz_fail(RZ_ERR_OOM, "hipMalloc failed (net)");
        net->allocs.push_back(std::move(fresh));
    }
    void *p = net->allocs[net->upload_cursor].p;
    net->upload_cursor += 1;
    if (hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return rz_fail(RZ_ERR_HIP, "hipMemcpy failed (net)");
    *out = (const T *)p;
    return RZ_OK;
}

int net_ready(rz_net *net, int32_t n) {
    if (!net) return rz_fail(RZ_ERR_ARG, "net handle is NULL");
    if (!net->loaded) return rz_fail(RZ_ERR_ARG, "rz_net_load has not been called");
    if (n < 0) return rz_fail(RZ_ERR_ARG, "negative batch");
    return rz_on_device(net->device);
}

// ---- the records the entry points hand to the kernels and to the engine, each built in one place

// the engine's device view, and the net ready for a batch of its games
int engine_view(rz_net *net, rz_engine *engine, rzt::Dev *dev) {
    RZ_TRY(rz_device_view(engine, dev, (int64_t)sizeof(*dev)));
    return net_ready(net, dev->n_games);
}

int same_board(const rz_net *net, const rzt::Dev &dev, bool actions_too) {
    if (dev.BH != net->dev.BH || dev.BW != net->dev.BW || (actions_too && dev.A != net->dev.A))
        return rz_fail(RZ_ERR_ARG, "engine and network disagree on the board");
    return RZ_OK;
}

// what the tree step of the deferred route needs of the value head (rows: the inputs in d_valfeat; the resident search keeps them in LDS)
rz_value_head value_head_of(const rz_net *net, bool rows = true) {
    return rz_value_head{rows ? net->d_valfeat.p : nullptr, net->d_w1t, net->dev.fc_val1_b, net->dev.fc_val2_w, net->dev.fc_val2_b,
                         net->vf_groups * 4, net->vf_groups};
}

// f16 values per slot of the policy-feature store: store_tiles tiles of groups_act K-steps of 32 boards x 16 x (hi | lo)
long long store_stride(const rz_net *net) { return (long long)net->store_tiles * net->dev.groups_act * 1024; }

// the features of a launch go to the store's slot slot_of[board] (value_rows: and the value head's inputs to d_valfeat, the schedule
// trace attached) / to where the ordinary route puts them
DeferredOut store_out(const rz_net *net, const int32_t *slot_of, bool value_rows) {
    return DeferredOut{slot_of, store_stride(net), value_rows ? net->d_valfeat.p : nullptr, value_rows ? net->vf_groups * 4 : 0,
                       value_rows ? net->d_trace : nullptr, net->store_slots};
}
DeferredOut no_store() { return DeferredOut{nullptr, 0, nullptr, 0, nullptr, 0}; }

// active == NULL: every game is; count: the delta counters
dl::DeltaArgs delta_args(const rz_net *net, const uint8_t *active, float *feat32, bool count, int mode, const uint64_t *win = nullptr) {
    return dl::DeltaArgs{net->d_base_hdr, net->d_base_recs, active ? active : net->d_base_ones.p, feat32, count ? net->d_delta_stats.p : nullptr,
                         mode, (65536 + net->dev.BW - 1) / net->dev.BW, win};
}

// the NetDev of a GEMM over the store's tiles, which hold the policy K-steps only; n_groups: groups of 128 policy outputs
int policy_store_dev(const rz_net *net, NetDev *nd, int *n_groups) {
    *nd = net->dev;
    nd->groups_val = 0;
    *n_groups = (nd->Npad / 32 + 3) / 4;
    if (*n_groups > 2) return rz_fail(RZ_ERR_INTERNAL, "more than 256 policy outputs");
    return RZ_OK;
}

// the internal feature buffer uses the padded layout of the FC GEMM (NetDev::feat_ld)
void use_internal_feat_layout(rz_net *net) {
    net->dev.feat_ld = 16 * (net->dev.groups_act + net->dev.groups_val);
    net->dev.feat_val_off = 16 * net->dev.groups_act;
}

}  // namespace

template <int NT>
static void launch_trunk_rows(bool bits, dim3 grid, hipStream_t stream, const NetDev &nd, const float *d_obs, LeafBits leaves, float *f32,
                              _Float16 *f16, int n_boards, unsigned *flags, DeferredOut later = no_store(),
                              bool fp8 = false) {
    if (fp8 && bits) {   // (the schedule trace reads the default arithmetic's kernel)
        k_trunk_rows<NT, true, false, true><<<grid, dim3(256), 0, stream>>>(nd, d_obs, leaves, f32, f16, n_boards, flags, later);
        return;
    }
    if constexpr (NT == 15) {
        if (bits && later.trace) {
            k_trunk_rows<NT, true, true><<<grid, dim3(256), 0, stream>>>(nd, d_obs, leaves, f32, f16, n_boards, flags, later);
            return;
        }
    }
    if (bits) k_trunk_rows<NT, true><<<grid, dim3(256), 0, stream>>>(nd, d_obs, leaves, f32, f16, n_boards, flags, later);
    else k_trunk_rows<NT, false><<<grid, dim3(256), 0, stream>>>(nd, d_obs, leaves, f32, f16, n_boards, flags, later);
}

template <int NT>
static void launch_search_rows(dim3 grid, hipStream_t stream, const NetDev &nd, LeafBits leaves, _Float16 *store, int n_games, unsigned *flags,
                               DeferredOut later, const ResArgs<true> &res, bool fp8) {
    if (fp8) k_trunk_rows_res<NT, true><<<grid, dim3(256), 0, stream>>>(nd, leaves, store, n_games, flags, later, res);
    else k_trunk_rows_res<NT><<<grid, dim3(256), 0, stream>>>(nd, leaves, store, n_games, flags, later, res);
}

// f(std::integral_constant<int, rows>): the row-tile kernels are instantiated per board height (rows_kernel_covers)
template <typename F>
static void with_board_rows(int rows, F &&f) {
    switch (rows) {
        case 11: f(std::integral_constant<int, 11>{}); break;
        case 12: f(std::integral_constant<int, 12>{}); break;
        case 13: f(std::integral_constant<int, 13>{}); break;
        case 14: f(std::integral_constant<int, 14>{}); break;
        case 15: f(std::integral_constant<int, 15>{}); break;
        default: f(std::integral_constant<int, 16>{}); break;
    }
}

// How k_trunk_split covers a board (trunk_class()).  ``ms``: waves that share an N-tile's output channels -- 4: one tile; 2: two tiles x two
// channel halves; 3: 9x9, three tiles + the fourth wave on a quarter of conv3's channels; 1: four tiles, one per wave; 0: two tiles per wave.
// ``compact``: at most two tiles that fit the 9 x 15 LDS grid (67-69 KB: two workgroups per CU), unless RZ_NET_COMPACT=0.
struct TrunkClass { int ms; bool compact; };

// THE launch of k_trunk_split: every instantiation is named here and nowhere else (RES: the resident search's, which has none for ms = 0).
// ``compact``: the caller's decision, from TrunkClass::compact and its own run-time conditions.
template <bool RES>
static void launch_trunk_split(int ms, bool compact, dim3 grid, hipStream_t st, const NetDev &nd, const float *obs, LeafBits leaves, float *f32,
                               _Float16 *f16, int n_boards, unsigned *flags, float *raw, float *hid, const DeferredOut &later, const ResArgs<RES> &res) {
    const dim3 wg(256);
    if (compact && ms == 4) k_trunk_split<1, 4, RES, 9, 15><<<grid, wg, 0, st>>>(nd, obs, leaves, f32, f16, n_boards, flags, raw, hid, later, res);
    else if (compact) k_trunk_split<1, 2, RES, 9, 15><<<grid, wg, 0, st>>>(nd, obs, leaves, f32, f16, n_boards, flags, raw, hid, later, res);
    else if (ms == 4) k_trunk_split<1, 4, RES><<<grid, wg, 0, st>>>(nd, obs, leaves, f32, f16, n_boards, flags, raw, hid, later, res);
    else if (ms == 2) k_trunk_split<1, 2, RES><<<grid, wg, 0, st>>>(nd, obs, leaves, f32, f16, n_boards, flags, raw, hid, later, res);
    else if (ms == 3) k_trunk_split<1, 3, RES><<<grid, wg, 0, st>>>(nd, obs, leaves, f32, f16, n_boards, flags, raw, hid, later, res);
    else if (RES || ms == 1) k_trunk_split<1, 1, RES><<<grid, wg, 0, st>>>(nd, obs, leaves, f32, f16, n_boards, flags, raw, hid, later, res);
    else if constexpr (!RES) k_trunk_split<2, 1, RES><<<grid, wg, 0, st>>>(nd, obs, leaves, f32, f16, n_boards, flags, nullptr, nullptr, later, res);
}

// ... and of its PUCT instantiations (rz_net_search_resident_puct: RES + FC_HERE on the 18 x 18 grid, one per way of covering a board of
// up to 10 rows; ms = 0 has none).  raw / hid: one row per game.
static void launch_search_split_puct(int ms, dim3 grid, hipStream_t st, const NetDev &nd, LeafBits leaves, int n_games, unsigned *flags, float *raw,
                                     float *hid, const ResArgs<true> &res) {
    const dim3 wg(256);
    const DeferredOut none = no_store();
    if (ms == 4) k_trunk_split<1, 4, true, kRowW, 18, true><<<grid, wg, 0, st>>>(nd, nullptr, leaves, nullptr, nullptr, n_games, flags, raw, hid, none, res);
    else if (ms == 2) k_trunk_split<1, 2, true, kRowW, 18, true><<<grid, wg, 0, st>>>(nd, nullptr, leaves, nullptr, nullptr, n_games, flags, raw, hid, none, res);
    else if (ms == 3) k_trunk_split<1, 3, true, kRowW, 18, true><<<grid, wg, 0, st>>>(nd, nullptr, leaves, nullptr, nullptr, n_games, flags, raw, hid, none, res);
    else k_trunk_split<1, 1, true, kRowW, 18, true><<<grid, wg, 0, st>>>(nd, nullptr, leaves, nullptr, nullptr, n_games, flags, raw, hid, none, res);
}

extern "C" {

int rz_net_create(int32_t height, int32_t width, int32_t n_actions, int32_t device, rz_net **out) {
    if (out == nullptr) return rz_fail(RZ_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (height < 1 || height > RZ_MAX_BOARD_SIZE || width < 1 || width > RZ_MAX_BOARD_SIZE)
        return rz_fail(RZ_ERR_ARG, "board dimensions out of range");
    if (n_actions < 1 || n_actions > RZ_MAX_BOARD_SIZE * RZ_MAX_BOARD_SIZE)
        return rz_fail(RZ_ERR_ARG, "n_actions out of range");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
        return rz_fail(RZ_ERR_ARG, "bad device ordinal");
    rz_net *net = new (std::nothrow) rz_net();
    if (!net) return rz_fail(RZ_ERR_OOM, "host allocation failed");
    net->board_size = height;
    net->device = device;
    if (const char *v = getenv("RZ_NET_COMPACT")) {
        net->compact_grid = v[0] != '0';
        net->compact_always = v[0] == '2';
    }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            net->n_cus = prop.multiProcessorCount;
    }
    if (hipSetDevice(device) != hipSuccess || !net->d_flags.alloc(sizeof(unsigned)) || !net->d_flags.fill(0)) {
        delete net;
        return rz_fail(RZ_ERR_OOM, "hipMalloc failed (net flags)");
    }
    memset(&net->dev, 0, sizeof(net->dev));
    net->dev.BH = height;
    net->dev.BW = width;
    net->dev.S = height * width;
    net->dev.A = n_actions;
    {
        NetDev &D = net->dev;
        D.Npad = (D.A + 31) / 32 * 32;
        D.groups_act = (4 * D.S + 15) / 16;
        D.groups_val = (2 * D.S + 15) / 16;
        // N-tile geometry of k_trunk_split: rows x width tiles if four of them cover the board, else 2 x 16
        const int rows = 32 / D.BW < 16 ? 32 / D.BW : 16;  // rows + 2 halo rows stay inside the 18-row grid
        if (rows >= 1 && (D.BH + rows - 1) / rows <= 4) {
            D.tile_rows = rows;
            D.tile_cols = D.BW;
        } else {
            D.tile_rows = 2;
            D.tile_cols = 16;
        }
        D.tile_rcp = (65536 + D.tile_cols - 1) / D.tile_cols;  // (n * rcp) >> 16 == n / cols for n < 32
    }
    *out = net;
    return RZ_OK;
}

int rz_net_destroy(rz_net *net) {
    if (!net) return RZ_OK;
    (void)hipSetDevice(net->device);
    (void)hipDeviceSynchronize();
    delete net;
    return RZ_OK;
}

int rz_net_error_flags(rz_net *net, uint32_t *h_flags) {
    if (!net || !h_flags) return rz_fail(RZ_ERR_ARG, "NULL argument");
    if (hipSetDevice(net->device) != hipSuccess) return rz_fail(RZ_ERR_HIP, "hipSetDevice failed");
    unsigned v = 0;
    if (hipMemcpy(&v, net->d_flags, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "hipMemcpy failed (net flags)");
    if (v != 0 && hipMemset(net->d_flags, 0, sizeof(unsigned)) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "hipMemset failed (net flags)");
    *h_flags = v;
    return RZ_OK;
}

int rz_net_load(rz_net *net, const float *const *h_params, int32_t n_params) {
    if (!net || !h_params) return rz_fail(RZ_ERR_ARG, "NULL argument");
    if (n_params != 16) return rz_fail(RZ_ERR_ARG, "expected the 16 tensors of PolicyValueNet.state_dict()");
    for (int i = 0; i < 16; ++i)
        if (!h_params[i]) return rz_fail(RZ_ERR_ARG, "a parameter pointer is NULL");
    if (hipSetDevice(net->device) != hipSuccess) return rz_fail(RZ_ERR_HIP, "hipSetDevice failed");
    (void)hipDeviceSynchronize();
    net->upload_cursor = 0;
    const int S = net->dev.S;
    NetDev &D = net->dev;
    // the arithmetic is rz_pack.h's; here: the uploads, in an order that must not change (net_upload reuses the buffers of
    // the first load by position)
    const rzp::Prepared P = rzp::prepare(h_params, rzp::Shape{S, D.A, D.Npad, D.groups_act, D.groups_val});
    net->split_ok = P.split_ok;
    net->vf_groups = P.vf_groups;
    memcpy(net->range_info, P.range_info, sizeof(net->range_info));
    int rc = RZ_OK;
    auto up = [&](const std::vector<float> &v, auto **dst) { if (rc == RZ_OK) rc = net_upload(net, v.data(), v.size(), dst); };
    auto up_f = [&](const float *src, size_t count, const float **dst) { if (rc == RZ_OK) rc = net_upload(net, src, count, dst); };
    // order of PolicyValueNet.state_dict(): conv1.w,b conv2.w,b conv3.w,b act_conv1.w,b
    // act_fc1.w,b val_conv1.w,b val_fc1.w,b val_fc2.w,b
    up(P.w1, &D.w1);
    up_f(h_params[1], 32, &D.b1);
    up(P.w2, &D.w2);
    up_f(h_params[3], 64, &D.b2);
    up(P.w3, &D.w3);
    up(P.u2f, &D.u2f);
    up(P.u3f, &D.u3f);
    up(P.s2, &D.s2);
    up(P.s3, &D.s3);
    up(P.t2, &D.t2);
    up(P.t3, &D.t3);
    up(P.t3f, &D.t3f);
    up(P.s1, &D.s1);
    up(P.fs_act, &D.fs_act);
    up(P.fs_val, &D.fs_val);
    up(P.s_inv, &D.s_inv);
    up_f(h_params[5], 128, &D.b3);
    up(P.wh, &D.wh);
    up(P.whp, &D.whp);
    up(P.bh, &D.bh);
    up(P.fc_act_w, &D.fc_act_w);
    up(P.fc_act_b, &D.fc_act_b);
    up(P.fc_val1_w, &D.fc_val1_w);
    up_f(h_params[13], 64, &D.fc_val1_b);
    up_f(h_params[14], 64, &D.fc_val2_w);
    up_f(h_params[15], 1, &D.fc_val2_b);
    up(P.w1t, &net->d_w1t);
    // the receptive-field bases hold activations of the weights they were built with: none survives an upload (a leaf of a game
    // without a valid base takes the route without one until rz_net_delta_bases runs again)
    if (rc == RZ_OK && net->base_games > 0 && !net->d_base_hdr.fill(0))
        rc = rz_fail(RZ_ERR_HIP, "hipMemset failed (base cache)");
    net->loaded = rc == RZ_OK;
    return rc;
}

int rz_net_reserve(rz_net *net, int32_t max_boards) {
    RZ_ENTER(net_ready, net, max_boards);
    if (max_boards <= net->feat_boards) return RZ_OK;
    (void)hipDeviceSynchronize();
    net->d_feat.release();
    net->d_feat16.release();
    net->d_raw.release();
    net->d_hid.release();
    net->feat16_valid = net->feat32_valid = false;
    net->feat_boards = 0;
    // internal features: [boards padded to 32][16 * (groups_act + groups_val)], zero filled once
    const size_t pad_boards = ((size_t)max_boards + 31) / 32 * 32;
    net->feat_floats = pad_boards * 16 * (size_t)(net->dev.groups_act + net->dev.groups_val);
    if (!net->d_feat.alloc(net->feat_floats * sizeof(float)) ||
        !net->d_raw.alloc(4 * (((size_t)max_boards + 63) / 64 * 64) * net->dev.Npad * sizeof(float)) ||
        !net->d_hid.alloc(4 * (((size_t)max_boards + 63) / 64 * 64) * 64 * sizeof(float)))
        return rz_fail(RZ_ERR_OOM, "hipMalloc failed (feature buffers)");
    // padded boards and the K tail must read as finite values (they meet zero weights)
    if (!net->d_feat.fill(0)) return rz_fail(RZ_ERR_HIP, "hipMemset failed (feature buffer)");
    {   // f16 pieces: [boards padded to 64][K-steps][hi | lo][16 x f16]; the K tail and padded boards stay zero
        const size_t bytes = (((size_t)max_boards + 63) / 64 * 64) * (size_t)(net->dev.groups_act + net->dev.groups_val) * 64;
        if (!net->d_feat16.alloc(bytes)) return rz_fail(RZ_ERR_OOM, "hipMalloc failed (f16 feature buffer)");
        if (!net->d_feat16.fill(0)) return rz_fail(RZ_ERR_HIP, "hipMemset failed (f16 feature buffer)");
    }
    net->raw_part_floats = (((size_t)max_boards + 63) / 64 * 64) * net->dev.Npad;  // room for four K-quarter parts
    net->hid_part_floats = (((size_t)max_boards + 63) / 64 * 64) * 64;
    net->feat_boards = max_boards;
    return RZ_OK;
}

// k_trunk_rows is instantiated for boards of 11 .. 16 rows (the 15 x 15 Gomoku board of the BASELINE configuration and its kin:
// the boards k_trunk_split needs more than four tiles for), 11 .. 16 columns wide (narrower ones leave too many of a row tile's
// 16 MFMA columns empty)
static bool rows_kernel_covers(int bh, int bw) { return bh >= 11 && bh <= 16 && bw >= 11 && bw <= 16; }

// The route -- which kernels evaluate a leaf -- as the library decides it for the net it holds: rows_kernel_covers() and the four functions
// below.  rlzero_amd/route.py decides the same for the Python callers BEFORE they call: that module is the one other place that must agree
// with these, and the RZ_ERR_ARG returns of the entry points are the backstop where the two disagree.
static bool split_trunk_ok(const rz_net *net) {   // the split-f16 trunks (both kernels), finite activation bounds: positions, deferred priors
    return (net->algo == RZ_NET_SPLIT_F16 || net->algo == RZ_NET_SPLIT_F16_TILES) && net->split_ok;
}
static bool delta_covers(const rz_net *net) {   // k_trunk_rows' boards, its arithmetic, positions: the receptive-field trunk
    return split_trunk_ok(net) && net->algo == RZ_NET_SPLIT_F16 && !net->fp8_cross && rows_kernel_covers(net->dev.BH, net->dev.BW);
}
static bool compact_grid_covers(const rz_net *net, int tiles) {   // (route.py: compact_grid_board) at most 7 columns, tile rows + halo within 15
    return net->compact_grid && tiles <= 2 && net->dev.BW <= 7 && tiles * net->dev.tile_rows + 2 <= 15;
}
static TrunkClass trunk_class(const rz_net *net) {
    const int tiles = (net->dev.BH + net->dev.tile_rows - 1) / net->dev.tile_rows;
    return TrunkClass{tiles <= 1 ? 4 : tiles <= 2 ? 2 : (tiles == 3 && net->dev.tile_rows == 3) ? 3 : tiles <= 4 ? 1 : 0, compact_grid_covers(net, tiles)};
}

static void launch_trunk(rz_net *net, const float *d_obs, float *d_feat, int32_t n_boards, void *stream,
                         LeafBits leaves = LeafBits{nullptr, nullptr, nullptr}, DeferredOut later = no_store()) {
    const dim3 grid((unsigned)n_boards);
    // the internal buffer uses the padded layout of the FC GEMM, a caller's buffer the natural one
    const bool internal = d_feat == net->d_feat;
    // the split-f16 trunk writes what the FC GEMM behind it reads: the f16 pieces, and the f32 features only for a
    // caller's buffer or when the f32 GEMM is forced
    // a net whose weights give no finite activation bound (rz_net_load) never runs on the f16 pipe
    const bool split_algo = net->algo == RZ_NET_SPLIT_F16 || net->algo == RZ_NET_SPLIT_F16_TILES;
    const int algo = split_trunk_ok(net) ? RZ_NET_SPLIT_F16 : split_algo ? RZ_NET_DIRECT : net->algo;
    const bool split = algo == RZ_NET_SPLIT_F16;
    const bool want_f32 = !split || !internal || net->heads_algo == RZ_NET_HEADS_F32;
    if (internal) {
        net->feat16_valid = split;
        net->feat32_valid = want_f32;
    }
    if (internal) use_internal_feat_layout(net);
    else net->dev.feat_ld = 6 * net->dev.S, net->dev.feat_val_off = 4 * net->dev.S;
    // Winograd kernels are persistent: one workgroup per CU (LDS bound) loops over its boards
    const int wg_cap = net->max_wgs > 0 ? net->max_wgs : net->n_cus;
    const dim3 pgrid((unsigned)(n_boards < wg_cap ? n_boards : wg_cap));
    net->raw_from_trunk = false;
    if (algo == RZ_NET_WINOGRAD_F4)
        k_trunk_wino_f4<4><<<pgrid, dim3(256), 0, (hipStream_t)stream>>>(net->dev, d_obs, d_feat, n_boards);
    else if (algo == RZ_NET_SPLIT_F16)
    {
        _Float16 *f16 = later.slot_of ? net->d_store16 : internal ? net->d_feat16 : nullptr;
        float *f32 = later.slot_of ? nullptr : want_f32 ? d_feat : nullptr;
        if (later.slot_of) net->feat16_valid = net->feat32_valid = false;   // (nothing for rz_net_heads_gemm)
        const TrunkClass tc = trunk_class(net);
        const bool bits = leaves.stones != nullptr;
        // Small batches of small boards (every board has a workgroup of its own, nothing of another lane to overlap with): the
        // trunk's workgroups run the FC layers on their boards themselves -- no FC launch, no kernel boundary (same bits).
        // Every workgroup then streams ALL FC weights from L2 for its one board (the GEMM launch reads them once per 32
        // boards): AUTO takes this route while the weights are at most 40 KB (6 x 6: 39 KB, TicTacToe one game +6 %, 16 games +3 %;
        // Connect4: 26 KB); at 9 x 9 (146 KB) the
        // launch it saves is cheaper than the stream it costs (64 games -5 %, profiles/r03/in_trunk_fc.txt)
        const bool fc_here = !later.slot_of && internal && tc.ms != 0 && net->dev.BH <= 10 && !rows_kernel_covers(net->dev.BH, net->dev.BW) &&
                             (net->heads_algo == RZ_NET_HEADS_IN_TRUNK ||
                              (net->heads_algo == RZ_NET_HEADS_AUTO && net->max_wgs == 0 && n_boards <= wg_cap &&
                               ((size_t)net->dev.A * 4 * net->dev.S + (size_t)64 * 2 * net->dev.S) * 4 <= 40 * 1024));
        float *raw = fc_here ? net->d_raw : nullptr, *hid = fc_here ? net->d_hid : nullptr;
        net->raw_from_trunk = fc_here;
        if (fc_here) net->feat16_valid = false;   // (the pieces stayed in LDS)
        if (net->algo == RZ_NET_SPLIT_F16 && rows_kernel_covers(net->dev.BH, net->dev.BW)) {   // wide boards: one N-tile per row
            const bool fp8 = net->fp8_cross;   // (float planes in this mode were refused by the callers)
            with_board_rows(net->dev.BH, [&](auto nt) {
                launch_trunk_rows<decltype(nt)::value>(bits, pgrid, (hipStream_t)stream, net->dev, d_obs, leaves, f32, f16, n_boards, net->d_flags, later, fp8);
            });
        } else {
            // small boards, more boards than half the CUs: the compact LDS grid, two workgroups per CU
            const bool compact = tc.compact && !fc_here && (2 * n_boards > wg_cap || net->compact_always);
            const dim3 cgrid((unsigned)(n_boards < 2 * wg_cap ? n_boards : 2 * wg_cap));
            launch_trunk_split<false>(tc.ms, compact, compact ? cgrid : pgrid, (hipStream_t)stream, net->dev, d_obs, leaves, f32, f16, n_boards,
                                      net->d_flags, raw, hid, later, ResArgs<false>{});
        }
    }
    else
        k_trunk<<<grid, dim3(kTrunkThreads), 0, (hipStream_t)stream>>>(net->dev, d_obs, d_feat, n_boards);
}

// The FC GEMM of the heads on the internal features -> net->d_raw (policy logits) / net->d_hid (value hidden layer).
static void launch_heads_gemm(rz_net *net, const float *d_feat, int32_t n_boards, void *stream) {
    use_internal_feat_layout(net);
    if (net->raw_from_trunk && d_feat == net->d_feat) {   // the trunk's workgroups ran these layers on their boards
        net->raw_parts = 1;
        return;
    }
    int algo = net->heads_algo;
    // after the split-f16 trunk: the f16 pipe.  Beside a capped trunk the GEMM has 32 CUs (64-board workgroups keep
    // the loads of a CU below its vector memory rate), alone it has the chip (many small workgroups hide the load
    // latency); up to 256 boards the single-wave K-quarter workgroups are the shortest launch (+4 % whole-step at 64 and
    // 256 boards, level above that); every shape gives the same bits (profiles/r01/sweep_heads.txt, r02/heads_small.txt)
    if (algo == RZ_NET_HEADS_AUTO || algo == RZ_NET_HEADS_IN_TRUNK)   // (IN_TRUNK on a board size the trunk does not do it for)
        algo = net->max_wgs > 0 ? RZ_NET_HEADS_SPLIT_64 : n_boards <= 256 ? RZ_NET_HEADS_SPLIT_PARTS : RZ_NET_HEADS_SPLIT_32;
    if (d_feat != net->d_feat || !net->feat16_valid) algo = RZ_NET_HEADS_F32;
    else if (algo == RZ_NET_HEADS_F32 && !net->feat32_valid)  // F32 chosen after a trunk that wrote only the f16 pieces
        algo = net->max_wgs > 0 ? RZ_NET_HEADS_SPLIT_64 : RZ_NET_HEADS_SPLIT_32;
    const f32x4 *f16 = reinterpret_cast<const f32x4 *>(net->d_feat16.p);
    const int n_act_tiles = net->dev.Npad / 32;
    net->raw_parts = 1;
    if (algo == RZ_NET_HEADS_SPLIT_PARTS) {
        net->raw_parts = 4;
        const dim3 grid((unsigned)((n_boards + 31) / 32), (unsigned)(n_act_tiles + 2), 4);
        k_heads_part<5><<<grid, dim3(64), 0, (hipStream_t)stream>>>(net->dev, f16, net->d_raw, net->d_hid,
                                                                     (long long)net->raw_part_floats, (long long)net->hid_part_floats);
    } else if (algo == RZ_NET_HEADS_SPLIT_64) {
        // y = policy half (4 N-tiles) + value tile y: both halves exist even when the second has no policy tile
        const dim3 grid((unsigned)((n_boards + 63) / 64), 2);
        k_heads_split<2, 4, 3, true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(net->dev, f16, net->d_raw, net->d_hid, n_boards);
    } else if (algo == RZ_NET_HEADS_SPLIT_32) {
        const dim3 grid((unsigned)((n_boards + 31) / 32), (unsigned)((n_act_tiles + 1) / 2 + 2));
        k_heads_split<1, 2, 5, false><<<grid, dim3(256), 0, (hipStream_t)stream>>>(net->dev, f16, net->d_raw, net->d_hid, n_boards);
    } else {
        const dim3 grid((unsigned)((n_boards + 31) / 32), (unsigned)(net->dev.Npad / 32 + 2));
        k_heads_gemm<<<grid, dim3(64 * kHeadWaves), 0, (hipStream_t)stream>>>(net->dev, d_feat, net->d_raw, net->d_hid, n_boards);
    }
}

static int launch_heads(rz_net *net, const float *d_feat, int32_t n_boards, float *d_logp, float *d_value,
                        void *stream) {
    launch_heads_gemm(net, d_feat, n_boards, stream);
    k_heads_finish<<<dim3((unsigned)n_boards), dim3(64), 0, (hipStream_t)stream>>>(
        net->dev, net->d_raw, net->d_hid, d_logp, d_value, n_boards, net->raw_parts, (long long)net->raw_part_floats,
        (long long)net->hid_part_floats);
    return rz_launched("k_heads_*");
}

int rz_net_trunk(rz_net *net, const float *d_obs, int32_t n_boards, float *d_feat, void *stream) {
    RZ_ENTER(net_ready, net, n_boards);
    if (n_boards == 0) return RZ_OK;  // an empty batch is a no-op (its tensors have no storage)
    if (!d_obs) return rz_fail(RZ_ERR_ARG, "NULL device pointer");
    if (net->fp8_cross)
        return rz_fail(RZ_ERR_ARG, "RZ_NET_SPLIT_F16_FP8 evaluates positions (rz_net_trunk_leaves*, rz_net_search_resident): float planes are refused, "
                                    "not computed in another arithmetic");
    if (!d_feat) {  // internal feature buffer (the input of rz_net_heads)
        if (n_boards > net->feat_boards) return rz_fail(RZ_ERR_ARG, "batch larger than rz_net_reserve()d");
        d_feat = net->d_feat;
    }
    launch_trunk(net, d_obs, d_feat, n_boards, stream);
    return rz_launched("k_trunk");
}

int rz_net_trunk_leaves(rz_net *net, const uint64_t *d_stones, const int32_t *d_to_move, const int32_t *d_last_cell,
                        int32_t n_boards, void *stream) {
    RZ_ENTER(net_ready, net, n_boards);
    if (n_boards == 0) return RZ_OK;
    if (!d_stones || !d_to_move || !d_last_cell) return rz_fail(RZ_ERR_ARG, "NULL device pointer");
    if (n_boards > net->feat_boards) return rz_fail(RZ_ERR_ARG, "batch larger than rz_net_reserve()d");
    if (!split_trunk_ok(net))
        return rz_fail(RZ_ERR_ARG, "rz_net_trunk_leaves needs the RZ_NET_SPLIT_F16 trunk (the others read float planes: rz_net_trunk)");
    launch_trunk(net, nullptr, net->d_feat, n_boards, stream, LeafBits{d_stones, d_to_move, d_last_cell});
    return rz_launched("k_trunk_split");
}

int rz_net_deferred_reserve(rz_net *net, int32_t max_boards, int32_t slots) {
    RZ_ENTER(net_ready, net, max_boards);
    if (slots < 1 || max_boards < 1) return rz_fail(RZ_ERR_ARG, "rz_net_deferred_reserve: slots and max_boards must be positive");
    if (max_boards <= net->store_boards && slots <= net->store_slots) return RZ_OK;
    // grow to the larger of what is held and what is asked in BOTH directions: an engine that reserved more boards (or slots)
    // earlier keeps fitting when another one asks for more of the other
    if (max_boards < net->store_boards) max_boards = net->store_boards;
    if (slots < net->store_slots) slots = net->store_slots;
    (void)hipDeviceSynchronize();
    net->d_store16.release();
    net->d_store_raw.release();
    net->d_valfeat.release();
    net->store_boards = 0;
    net->store_slots = 0;
    const int tiles = ((max_boards + 63) / 64) * 2;   // whole 64-board blocks: the GEMM's workgroups take two tiles
    const size_t store_bytes = (size_t)slots * tiles * net->dev.groups_act * 2048;
    const size_t raw_bytes = (size_t)slots * tiles * 32 * net->dev.Npad * sizeof(float);
    const size_t val_bytes = (size_t)tiles * 32 * net->vf_groups * 4 * sizeof(float);
    if (!net->d_store16.alloc(store_bytes) || !net->d_store_raw.alloc(raw_bytes) || !net->d_valfeat.alloc(val_bytes))
        return rz_fail(RZ_ERR_OOM, "hipMalloc failed (deferred-priors store)");
    // the K tail of a tile's last K-step, the rows of boards that do not exist and the padding of the value rows are never
    // written: they must read as finite values (they meet zero weights, or rows nobody reads)
    if (!net->d_store16.fill(0) || !net->d_valfeat.fill(0))
        return rz_fail(RZ_ERR_HIP, "hipMemset failed (deferred-priors store)");
    net->store_tiles = tiles;
    net->store_slots = slots;
    net->store_boards = max_boards;
    return RZ_OK;
}

int rz_net_trunk_leaves_deferred(rz_net *net, const uint64_t *d_stones, const int32_t *d_to_move, const int32_t *d_last_cell,
                                 int32_t n_boards, const int32_t *d_slot_of_board, rz_value_head *out, void *stream) {
    RZ_ENTER(net_ready, net, n_boards);
    if (!out) return rz_fail(RZ_ERR_ARG, "NULL output pointer");
    if (!split_trunk_ok(net))
        return rz_fail(RZ_ERR_ARG, "the deferred-priors route needs the RZ_NET_SPLIT_F16 trunk (a net with finite activation bounds)");
    if (n_boards > net->store_boards) return rz_fail(RZ_ERR_ARG, "batch larger than rz_net_deferred_reserve()d");
    if (n_boards > 0) {
        if (!d_stones || !d_to_move || !d_last_cell || !d_slot_of_board) return rz_fail(RZ_ERR_ARG, "NULL device pointer");
        launch_trunk(net, nullptr, net->d_feat, n_boards, stream, LeafBits{d_stones, d_to_move, d_last_cell}, store_out(net, d_slot_of_board, true));
        RZ_TRY(rz_launched("the split-f16 trunk"));
    }
    *out = value_head_of(net);
    return RZ_OK;
}

// policy == false: rz_net_search_resident_values (policy on demand: k_delta_res<false> or a refusal)
static int search_resident(rz_net *net, rz_engine *engine, int32_t n_sims, int32_t select_first, void *stream, bool policy) {
    rzt::Dev dev;
    RZ_TRY(engine_view(net, engine, &dev));
    if (n_sims < 1) return rz_fail(RZ_ERR_ARG, "rz_net_search_resident: n_sims must be positive");
    // a game's leaves go to store slots pend[g] .. pend[g] + n_sims - 1: more simulations than either side has slots can never fit
    // (and a leaf whose slot lies beyond the store is not written: the tree code flags its game RZ_FLAG_INTERNAL)
    if (n_sims > net->store_slots || n_sims > dev.pend_cap) {
        return rz_fail(RZ_ERR_ARG, "rz_net_search_resident: more simulations than the store has slots: %d simulations, %d / %d slots "
                                   "(rz_net_deferred_reserve / rz_deferred_reserve)", n_sims, net->store_slots, dev.pend_cap);
    }
    const bool rows = net->algo == RZ_NET_SPLIT_F16 && rows_kernel_covers(net->dev.BH, net->dev.BW);
    const TrunkClass tc = trunk_class(net);
    if (!split_trunk_ok(net) || (!rows && (tc.ms == 0 || net->dev.BH > 10 || net->dev.BW > 10)))
        return rz_fail(RZ_ERR_ARG, "the resident search needs the RZ_NET_SPLIT_F16 trunk on a board of 11 .. 16 rows and columns (the row-tile "
                                    "kernel) or of up to 10 x 10 (k_trunk_split with one N-tile per wave)");
    if (dev.K != 1 || dev.score_mode != RZ_SCORE_UCT_REF || dev.pend_cap <= 0)
        return rz_fail(RZ_ERR_ARG, "the resident search is the deferred-priors route: RZ_SCORE_UCT_REF, one simulation in flight, rz_deferred_reserve first");
    RZ_TRY(same_board(net, dev, true));
    // receptive-field evaluation (rz_net_delta_reserve for this many games, the default trunk on a board of 11 .. 16 rows and columns):
    // k_delta_res, TWO workgroups per CU; rz_net_delta_resident(net, 0) keeps k_trunk_rows_res
    const bool delta_res = net->delta_resident && delta_covers(net) && net->base_games >= dev.n_games;
    // k_trunk_rows_res holds a CU (151 KB of LDS) for a whole search: at most one game per CU.  k_delta_res holds half a CU and its
    // workgroups depend on nothing outside their game: a batch beyond two per CU runs in ROUNDS, the dispatcher handing a CU's free half
    // to the next game of the grid as a search ends (1024 / 1536 games: two / three rounds of 512, the chip full throughout)
    // (small boards on the compact LDS grid: 69 KB, two workgroups per CU -- the same freedom; and for fewer games too: the smaller grid
    // is 1-2 % ahead even with ONE game on the chip, TicTacToe 93.3 -> 94.6 k)
    const bool compact_res = !rows && tc.compact;
    if (dev.n_games > net->store_boards || (!delta_res && !compact_res && dev.n_games > net->n_cus))
        return rz_fail(RZ_ERR_ARG, "the resident search runs one workgroup per game, at most one per CU (any number with rz_net_delta_reserve, or on a board of "
                                    "the compact grid) and rz_net_deferred_reserve()d");
    if (rows ? (net->vf_groups != 64 && net->vf_groups != 128) : net->vf_groups > 64) return rz_fail(RZ_ERR_INTERNAL, "value head groups");
    ResArgs<true> res;
    res.E = dev;
    res.vh = value_head_of(net, false);
    res.n_sims = n_sims;
    res.select_first = select_first ? 1 : 0;
    // rz_set_playouts: a game with fewer simulations leaves the slots pend[g] + sims_of[g] .. of the feature store as they were
    // (zeros, or finite features of an earlier search).  They are NOT skipped: rz_net_deferred_gemm runs over them -- rows do not mix,
    // the GEMM raises no range flag (only the trunk's stores do) -- and what it computes there is IGNORED: k_deferred_priors reads the
    // slots below pend[g] only, and pend[g] counts the leaves the game stored.
    RZ_TRY(rz_playouts_view(engine, &res.sims_of, &res.order));
    const DeferredOut later = store_out(net, dev.pend, false);
    const LeafBits leaves{dev.leaf_stones, dev.leaf_to_move, dev.leaf_last};
    const dim3 grid((unsigned)dev.n_games);
    const hipStream_t st = (hipStream_t)stream;
    net->feat16_valid = net->feat32_valid = false;
    if (!policy && !delta_res)
        return rz_fail(RZ_ERR_ARG, "rz_net_search_resident_values: the search without policy features is k_delta_res's (the default trunk on a board of "
                                    "11 .. 16 rows and columns, rz_net_delta_reserve for the engine's games, rz_net_delta_resident on)");
    if (delta_res) {
        if (select_first) {   // a search begins: the bases of its roots (a continued search finds them, or takes the route without)
            RZ_TRY(rz_net_delta_bases(net, dev.root_stones, dev.root_to_move, dev.n_games, stream));
        }
        const dl::DeltaArgs da = delta_args(net, nullptr, nullptr, true, 0, net->d_win);
        if (policy) dl::k_delta_res<true><<<grid, dim3(256), 0, st>>>(net->dev, net->d_store16, later, da, res);
        else dl::k_delta_res<false><<<grid, dim3(256), 0, st>>>(net->dev, net->d_store16, later, da, res);
        return rz_launched("the resident search (k_delta_res)");
    }
    if (rows)
        with_board_rows(net->dev.BH, [&](auto nt) {
            launch_search_rows<decltype(nt)::value>(grid, st, net->dev, leaves, net->d_store16, dev.n_games, net->d_flags, later, res, net->fp8_cross);
        });
    else   // (the launches of launch_trunk for these boards, RES instantiations)
        launch_trunk_split<true>(tc.ms, compact_res, grid, st, net->dev, nullptr, leaves, nullptr, net->d_store16, dev.n_games, net->d_flags,
                                 nullptr, nullptr, later, res);
    return rz_launched("the resident search");
}

int rz_net_search_resident(rz_net *net, rz_engine *engine, int32_t n_sims, int32_t select_first, void *stream) {
    return search_resident(net, engine, n_sims, select_first, stream, true);
}

int rz_net_search_resident_values(rz_net *net, rz_engine *engine, int32_t n_sims, int32_t select_first, void *stream) {
    return search_resident(net, engine, n_sims, select_first, stream, false);
}

// The resident search under RZ_SCORE_PUCT (k_trunk_split<1, MS, RES, 18 x 18, PUCT>).  The route, as route.decide(resident_puct=True) states
// it on the other side of the ABI: the split-f16 trunk, positions, one simulation in flight, RZ_SCORE_PUCT, a board of up to 10 x 10 that is the
// net's, any FC arithmetic but RZ_NET_HEADS_F32, at most one game per CU -- and, here only, rows of d_raw / d_hid for every game.
int rz_net_search_resident_puct(rz_net *net, rz_engine *engine, int32_t n_sims, int32_t select_first, void *stream) {
    rzt::Dev dev;
    RZ_TRY(engine_view(net, engine, &dev));
    if (n_sims < 1) return rz_fail(RZ_ERR_ARG, "rz_net_search_resident_puct: n_sims must be positive");
    if (dev.K != 1 || dev.score_mode != RZ_SCORE_PUCT)
        return rz_fail(RZ_ERR_ARG, "rz_net_search_resident_puct: RZ_SCORE_PUCT and one simulation in flight per tree (RZ_SCORE_UCT_REF: rz_net_search_resident)");
    const TrunkClass tc = trunk_class(net);
    if (tc.ms == 0 || net->dev.BH > 10 || net->dev.BW > 10)
        return rz_fail(RZ_ERR_ARG, "rz_net_search_resident_puct: a board of up to 10 x 10 (k_trunk_split with one N-tile per wave and the FC layers in the trunk)");
    if (!split_trunk_ok(net))
        return rz_fail(RZ_ERR_ARG, "rz_net_search_resident_puct needs the RZ_NET_SPLIT_F16 trunk (a net with finite activation bounds)");
    if (net->heads_algo == RZ_NET_HEADS_F32)
        return rz_fail(RZ_ERR_ARG, "rz_net_search_resident_puct runs the FC layers on the f16 pipe: RZ_NET_HEADS_F32 is the three-launch step's (another arithmetic)");
    RZ_TRY(same_board(net, dev, true));
    if (dev.n_games > net->n_cus)
        return rz_fail(RZ_ERR_ARG, "rz_net_search_resident_puct: one workgroup per game, one per CU: %d games, %d CUs", dev.n_games, net->n_cus);
    if (dev.n_games > net->feat_boards)
        return rz_fail(RZ_ERR_ARG, "rz_net_search_resident_puct: more games than rz_net_reserve()d (a row of logits per game)");
    ResArgs<true> res;
    res.E = dev;
    res.vh = rz_value_head{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};   // (the value head is finished from d_hid: rz_raw_heads)
    res.n_sims = n_sims;
    res.select_first = select_first ? 1 : 0;
    RZ_TRY(rz_playouts_view(engine, &res.sims_of, &res.order));   // (NULL under PUCT: rz_set_playouts and the cap refuse the rule)
    // what the launch leaves in the internal buffers: final logits and hidden rows of the LAST leaves (rz_net_heads_gemm then has nothing
    // to run and nothing stale to read), no feature pieces
    net->feat16_valid = net->feat32_valid = false;
    net->raw_from_trunk = true;
    net->raw_parts = 1;
    launch_search_split_puct(tc.ms, dim3((unsigned)dev.n_games), (hipStream_t)stream, net->dev, LeafBits{dev.leaf_stones, dev.leaf_to_move, dev.leaf_last},
                             dev.n_games, net->d_flags, net->d_raw, net->d_hid, res);
    return rz_launched("the resident search (PUCT)");
}

int rz_net_policy_rows(rz_net *net, rz_engine *engine, const rz_kept_rows *kept, void *stream) {
    if (!kept) return rz_fail(RZ_ERR_ARG, "NULL argument");
    rzt::Dev dev;
    RZ_TRY(engine_view(net, engine, &dev));
    if (!kept->rows || !kept->count) return rz_fail(RZ_ERR_ARG, "rz_kept_rows: NULL pointer");
    if (!delta_covers(net) || net->base_games < dev.n_games || !split_trunk_ok(net))
        return rz_fail(RZ_ERR_ARG, "rz_net_policy_rows: the receptive-field trunk (the default trunk on a board of 11 .. 16 rows and columns) and "
                                    "rz_net_delta_reserve for the engine's games");
    RZ_TRY(same_board(net, dev, true));
    if (dev.pend_cap <= 0 || dev.pend_stones == nullptr || dev.pend_lw == nullptr) return rz_fail(RZ_ERR_ARG, "rz_net_policy_rows: rz_deferred_reserve first");
    // a listed row addresses slot rows[i] / n_games of the store (the kernel skips a slot beyond it) and the game's tile
    if (kept->n_games != dev.n_games || dev.n_games > net->store_boards || kept->capacity < 1 || kept->capacity > (int64_t)dev.pend_cap * dev.n_games)
        return rz_fail(RZ_ERR_ARG, "rz_net_policy_rows: the rows are not this engine's, or more boards than rz_net_deferred_reserve()d");
    const dl::DeltaArgs da = delta_args(net, nullptr, nullptr, false, 0);
    const dl::PolicyRows pr{kept->rows, kept->count, dev.pend_stones, dev.pend_lw, dev.n_games, net->store_slots, store_stride(net)};
    const dim3 grid((unsigned)(2 * (net->n_cus > 0 ? net->n_cus : 1)));   // fixed: two workgroups per CU, striding over the device's count
    dl::k_trunk_policy_rows<<<grid, dim3(256), 0, (hipStream_t)stream>>>(net->dev, net->d_store16, da, pr);
    return rz_launched("k_trunk_policy_rows");
}

int rz_net_delta_reserve(rz_net *net, int32_t n_games) {
    RZ_ENTER(net_ready, net, n_games);
    if (!delta_covers(net))
        return rz_fail(RZ_ERR_ARG, "receptive-field evaluation exists for the RZ_NET_SPLIT_F16 trunk on boards of 11 .. 16 rows and columns");
    if (n_games < 1) return rz_fail(RZ_ERR_ARG, "rz_net_delta_reserve: n_games must be positive");
    if (n_games <= net->base_games) return RZ_OK;
    (void)hipDeviceSynchronize();
    if (!net->d_win) {   // the window table of the net's board (k_delta_res's leaf_windows)
        std::vector<uint64_t> win(rzw::kEntries);
        rzw::window_table(win.data(), net->dev.BH, net->dev.BW);
        if (!net->d_win.alloc(win.size() * sizeof(uint64_t))) return rz_fail(RZ_ERR_OOM, "hipMalloc failed (window table)");
        if (hipMemcpy(net->d_win, win.data(), win.size() * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess)
            return rz_fail(RZ_ERR_HIP, "hipMemcpy failed (window table)");
    }
    net->d_base_hdr.release();
    net->d_base_recs.release();
    net->d_base_ones.release();
    net->base_games = 0;
    const size_t hdr_bytes = (size_t)n_games * sizeof(dl::BaseHdr), rec_bytes = (size_t)n_games * 2 * dl::kBaseBytes;
    if (!net->d_base_hdr.alloc(hdr_bytes) || !net->d_base_recs.alloc(rec_bytes) || !net->d_base_ones.alloc((size_t)n_games))
        return rz_fail(RZ_ERR_OOM, "hipMalloc failed (base cache)");
    if (!net->d_base_ones.fill(1)) return rz_fail(RZ_ERR_HIP, "hipMemset failed (base cache)");
    if (!net->d_delta_stats && !net->d_delta_stats.alloc(8 * sizeof(unsigned)))
        return rz_fail(RZ_ERR_OOM, "hipMalloc failed (delta counters)");
    // valid = 0: a leaf of a game without bases takes the four passes without a base
    if (!net->d_base_hdr.fill(0) || !net->d_delta_stats.fill(0))
        return rz_fail(RZ_ERR_HIP, "hipMemset failed (base cache)");
    net->base_games = n_games;
    return RZ_OK;
}

int rz_net_delta_resident(rz_net *net, int32_t on) {
    if (!net) return rz_fail(RZ_ERR_ARG, "net handle is NULL");
    net->delta_resident = on != 0;
    return RZ_OK;
}

int rz_net_delta_invalidate(rz_net *net, void *stream) {
    if (!net) return rz_fail(RZ_ERR_ARG, "net handle is NULL");
    if (net->base_games > 0 &&
        hipMemsetAsync(net->d_base_hdr, 0, (size_t)net->base_games * sizeof(dl::BaseHdr), (hipStream_t)stream) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "hipMemsetAsync failed (base cache)");
    return RZ_OK;
}

int rz_net_delta_bases(rz_net *net, const uint64_t *d_root_stones, const int32_t *d_root_to_move, int32_t n_games, void *stream) {
    RZ_ENTER(net_ready, net, n_games);
    if (n_games == 0) return RZ_OK;
    if (!delta_covers(net)) return rz_fail(RZ_ERR_ARG, "receptive-field evaluation: RZ_NET_SPLIT_F16 on boards of 11 .. 16 rows and columns");
    if (n_games > net->base_games) return rz_fail(RZ_ERR_ARG, "more games than rz_net_delta_reserve()d");
    if (!d_root_stones || !d_root_to_move) return rz_fail(RZ_ERR_ARG, "NULL device pointer");
    const dl::DeltaArgs da = delta_args(net, nullptr, nullptr, false, 1);
    dl::k_trunk_delta<false><<<dim3((unsigned)(2 * n_games)), dim3(256), 0, (hipStream_t)stream>>>(
        net->dev, LeafBits{d_root_stones, d_root_to_move, nullptr}, nullptr, 2 * n_games, no_store(), da);
    return rz_launched("k_trunk_delta (bases)");
}

int rz_net_delta_leaves(rz_net *net, const uint64_t *d_stones, const int32_t *d_to_move, const int32_t *d_last_cell, int32_t n_boards,
                        const int32_t *d_slot_of_board, const uint8_t *d_active, float *d_feat32, int32_t without_base, rz_value_head *out,
                        void *stream) {
    RZ_ENTER(net_ready, net, n_boards);
    if (!delta_covers(net)) return rz_fail(RZ_ERR_ARG, "receptive-field evaluation: RZ_NET_SPLIT_F16 on boards of 11 .. 16 rows and columns");
    if (without_base && n_boards > net->base_games) RZ_TRY(rz_net_delta_reserve(net, n_boards));   // (the kernel reads a header per board in every mode)
    if (n_boards > net->base_games) return rz_fail(RZ_ERR_ARG, "more boards than rz_net_delta_reserve()d games");
    if (d_slot_of_board && n_boards > net->store_boards) return rz_fail(RZ_ERR_ARG, "batch larger than rz_net_deferred_reserve()d");
    if (n_boards > 0) {
        if (!d_stones || !d_to_move || !d_last_cell) return rz_fail(RZ_ERR_ARG, "NULL device pointer");
        if (!d_slot_of_board && !d_feat32) return rz_fail(RZ_ERR_ARG, "rz_net_delta_leaves: neither a store slot nor an f32 buffer to write to");
        const DeferredOut later = store_out(net, d_slot_of_board, true);
        const dl::DeltaArgs da = delta_args(net, d_active, d_feat32, true, without_base ? 2 : 0);
        const dim3 grid((unsigned)n_boards);
        _Float16 *store = d_slot_of_board ? net->d_store16 : nullptr;
        if (d_slot_of_board) net->feat16_valid = net->feat32_valid = false;
        if (net->d_trace && d_slot_of_board)
            dl::k_trunk_delta<true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(net->dev, LeafBits{d_stones, d_to_move, d_last_cell}, store, n_boards, later, da);
        else
            dl::k_trunk_delta<false><<<grid, dim3(256), 0, (hipStream_t)stream>>>(net->dev, LeafBits{d_stones, d_to_move, d_last_cell}, store, n_boards, later, da);
        RZ_TRY(rz_launched("k_trunk_delta"));
    }
    if (out) *out = value_head_of(net);
    return RZ_OK;
}

// the two calls above on an engine's own arrays (rz_device_view): the bases from its ROOT positions, the step on its leaves (store
// slot pend[g], games whose active flag is 0 skipped)
int rz_net_delta_bases_engine(rz_net *net, rz_engine *engine, void *stream) {
    rzt::Dev dev;
    RZ_TRY(engine_view(net, engine, &dev));
    RZ_TRY(same_board(net, dev, false));
    return rz_net_delta_bases(net, dev.root_stones, dev.root_to_move, dev.n_games, stream);
}

int rz_net_delta_step(rz_net *net, rz_engine *engine, rz_value_head *out, void *stream) {
    rzt::Dev dev;
    RZ_TRY(engine_view(net, engine, &dev));
    if (!out) return rz_fail(RZ_ERR_ARG, "NULL output pointer");
    if (dev.K != 1 || dev.pend_cap <= 0 || dev.pend == nullptr)
        return rz_fail(RZ_ERR_ARG, "rz_net_delta_step is the deferred-priors route: one simulation in flight, rz_deferred_reserve first");
    RZ_TRY(same_board(net, dev, false));
    return rz_net_delta_leaves(net, dev.leaf_stones, dev.leaf_to_move, dev.leaf_last, dev.n_games, dev.pend, dev.active, nullptr, 0, out, stream);
}

// rz_net_trunk_leaves on the engine's leaves through the receptive-field kernel: the features go to the internal buffer's f16 tiles
// (policy and value K-steps of the FC GEMM: rz_net_heads_gemm next) -- the three-launch step (PUCT) on boards of 11 .. 16 rows.
int rz_net_delta_trunk_engine(rz_net *net, rz_engine *engine, void *stream) {
    rzt::Dev dev;
    RZ_TRY(engine_view(net, engine, &dev));
    if (!delta_covers(net)) return rz_fail(RZ_ERR_ARG, "receptive-field evaluation: RZ_NET_SPLIT_F16 on boards of 11 .. 16 rows and columns");
    if (dev.K != 1) return rz_fail(RZ_ERR_ARG, "rz_net_delta_trunk_engine: one simulation in flight per tree (a base per game)");
    RZ_TRY(same_board(net, dev, false));
    if (dev.n_games > net->base_games) return rz_fail(RZ_ERR_ARG, "more games than rz_net_delta_reserve()d");
    if (dev.n_games > net->feat_boards) return rz_fail(RZ_ERR_ARG, "batch larger than rz_net_reserve()d");
    if (net->heads_algo == RZ_NET_HEADS_F32) return rz_fail(RZ_ERR_ARG, "rz_net_delta_trunk_engine writes the f16 tiles only (RZ_NET_HEADS_F32 reads f32 features: rz_net_trunk_leaves)");
    net->feat16_valid = true;
    net->feat32_valid = false;
    net->raw_from_trunk = false;
    use_internal_feat_layout(net);
    const dl::DeltaArgs da = delta_args(net, dev.active, nullptr, true, 0);
    dl::k_trunk_delta<false><<<dim3((unsigned)dev.n_games), dim3(256), 0, (hipStream_t)stream>>>(
        net->dev, LeafBits{dev.leaf_stones, dev.leaf_to_move, dev.leaf_last}, net->d_feat16, dev.n_games, no_store(), da);
    return rz_launched("k_trunk_delta");
}

int rz_net_delta_stats(rz_net *net, uint32_t *h_out8, int32_t reset) {
    if (!net || !h_out8) return rz_fail(RZ_ERR_ARG, "NULL argument");
    memset(h_out8, 0, 8 * sizeof(uint32_t));
    if (!net->d_delta_stats) return RZ_OK;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h_out8, net->d_delta_stats, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "hipMemcpy failed (delta counters)");
    if (reset && hipMemset(net->d_delta_stats, 0, 8 * sizeof(uint32_t)) != hipSuccess) return rz_fail(RZ_ERR_HIP, "hipMemset failed (delta counters)");
    return RZ_OK;
}

int rz_net_trace_attach(rz_net *net, void *d_trace) {
    if (!net) return rz_fail(RZ_ERR_ARG, "net handle is NULL");
    net->d_trace = (unsigned long long *)d_trace;
    return RZ_OK;
}

int rz_net_deferred_gemm(rz_net *net, int32_t n_boards, int32_t n_slots, rz_deferred_logits *out, void *stream) {
    RZ_ENTER(net_ready, net, n_boards);
    if (!out) return rz_fail(RZ_ERR_ARG, "NULL output pointer");
    if (n_slots < 0 || n_slots > net->store_slots || n_boards > net->store_boards)
        return rz_fail(RZ_ERR_ARG, "more slots / boards than rz_net_deferred_reserve()d");
    if (n_slots > 0 && n_boards > 0) {
        // the store is a list of n_slots * store_tiles tiles of groups_act K-steps each: k_heads_split's policy groups over all of
        // them (64 boards x 128 outputs per workgroup, the K quarters over its four waves: the bits of every other shape)
        NetDev nd;
        int n_groups = 0;
        RZ_TRY(policy_store_dev(net, &nd, &n_groups));
        const size_t pairs = (size_t)n_slots * net->store_tiles / 2;   // workgroups per output group: two board tiles each
        const dim3 grid((unsigned)(n_groups == 2 ? 2 * ((pairs + 7) / 8 * 8) : pairs));
        k_heads_split<2, 4, 3, false, true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(
            nd, reinterpret_cast<const f32x4 *>(net->d_store16.p), net->d_store_raw, nullptr, n_slots * net->store_tiles * 32);
        RZ_TRY(rz_launched("k_heads_split"));
    }
    out->raw = net->d_store_raw;
    out->ld = net->dev.Npad;
    out->rows_per_slot = net->store_tiles * 32;
    return RZ_OK;
}

int rz_net_deferred_gemm_rows(rz_net *net, const rz_kept_rows *kept, rz_deferred_logits *out, void *stream) {
    if (!kept || !out) return rz_fail(RZ_ERR_ARG, "NULL argument");
    RZ_ENTER(net_ready, net, kept->n_games);
    if (!kept->rows || !kept->count) return rz_fail(RZ_ERR_ARG, "rz_kept_rows: NULL pointer");
    // a listed row addresses slot rows[i] / n_games < capacity / n_games of the store, and logits row i < capacity exists
    if (kept->n_games < 1 || kept->n_games > net->store_boards || kept->capacity < 1 || kept->capacity > (int64_t)net->store_slots * kept->n_games)
        return rz_fail(RZ_ERR_ARG, "more slots / boards than rz_net_deferred_reserve()d");
    NetDev nd;
    int n_groups = 0;
    RZ_TRY(policy_store_dev(net, &nd, &n_groups));
    // one workgroup per CU (`part` is 128 KB of its LDS), whole groups of 16 (k_heads_rows: the output groups of a block 8 apart)
    const dim3 grid((unsigned)(((net->n_cus > 16 ? net->n_cus : 16) + 15) / 16 * 16));
    k_heads_rows<2, 4, 3><<<grid, dim3(256), 0, (hipStream_t)stream>>>(nd, reinterpret_cast<const f32x4 *>(net->d_store16.p), net->d_store_raw,
                                                                     kept->rows, kept->count, kept->n_games, net->store_tiles);
    RZ_TRY(rz_launched("k_heads_rows"));
    out->raw = net->d_store_raw;
    out->ld = net->dev.Npad;
    out->rows_per_slot = 0;
    return RZ_OK;
}

int rz_net_set_algo(rz_net *net, int32_t algo) {
    if (!net) return rz_fail(RZ_ERR_ARG, "net handle is NULL");
    if (algo != RZ_NET_DIRECT && algo != RZ_NET_WINOGRAD_F4 && algo != RZ_NET_SPLIT_F16 && algo != RZ_NET_SPLIT_F16_TILES &&
        algo != RZ_NET_SPLIT_F16_FP8)
        return rz_fail(RZ_ERR_ARG, "unknown algorithm");
    if (algo == RZ_NET_SPLIT_F16_FP8 && !rows_kernel_covers(net->dev.BH, net->dev.BW))
        return rz_fail(RZ_ERR_ARG, "RZ_NET_SPLIT_F16_FP8 exists for boards of 11 .. 16 rows and columns (k_trunk_rows)");
    net->fp8_cross = algo == RZ_NET_SPLIT_F16_FP8;
    net->algo = net->fp8_cross ? RZ_NET_SPLIT_F16 : algo;
    return RZ_OK;
}

int rz_net_range_info(rz_net *net, float *h_info8) {
    if (!net || !h_info8) return rz_fail(RZ_ERR_ARG, "NULL argument");
    if (!net->loaded) return rz_fail(RZ_ERR_ARG, "rz_net_load has not been called");
    memcpy(h_info8, net->range_info, sizeof(net->range_info));
    return RZ_OK;
}

#ifdef RZ_NET_PROFILE
int rz_net_debug_profile(long long *h_out16) {
    return hipDeviceSynchronize() == hipSuccess && hipMemcpyFromSymbol(h_out16, HIP_SYMBOL(net_prof), 24 * sizeof(long long)) == hipSuccess ? RZ_OK : RZ_ERR_HIP;
}
#endif

int rz_net_set_heads_algo(rz_net *net, int32_t heads_algo) {
    if (!net) return rz_fail(RZ_ERR_ARG, "net handle is NULL");
    if (heads_algo < RZ_NET_HEADS_AUTO || heads_algo > RZ_NET_HEADS_IN_TRUNK) return rz_fail(RZ_ERR_ARG, "unknown heads algorithm");
    net->heads_algo = heads_algo;
    return RZ_OK;
}

int rz_net_set_max_workgroups(rz_net *net, int32_t max_workgroups) {
    if (!net) return rz_fail(RZ_ERR_ARG, "net handle is NULL");
    if (max_workgroups < 0) return rz_fail(RZ_ERR_ARG, "max_workgroups must be >= 0");
    net->max_wgs = max_workgroups;
    return RZ_OK;
}

int rz_net_heads_gemm(rz_net *net, int32_t n_boards, rz_raw_heads *out, void *stream) {
    RZ_ENTER(net_ready, net, n_boards);
    if (!out) return rz_fail(RZ_ERR_ARG, "NULL output pointer");
    if (n_boards > net->feat_boards) return rz_fail(RZ_ERR_ARG, "batch larger than rz_net_reserve()d");
    if (n_boards > 0) {
        launch_heads_gemm(net, net->d_feat, n_boards, stream);
        RZ_TRY(rz_launched("k_heads_gemm"));
    }
    memset(out, 0, sizeof(*out));
    out->raw = net->d_raw;
    out->hid = net->d_hid;
    out->w2 = net->dev.fc_val2_w;
    out->b2 = net->dev.fc_val2_b;
    out->act_scale = net->dev.s_inv + 3;
    out->act_bias = net->dev.fc_act_b;
    out->val_scale = net->dev.s_inv + 4;
    out->val_bias = net->dev.fc_val1_b;
    out->raw_part_stride = (int64_t)net->raw_part_floats;
    out->hid_part_stride = (int64_t)net->hid_part_floats;
    out->ld = net->dev.Npad;
    out->n_parts = n_boards > 0 ? net->raw_parts : 1;
    return RZ_OK;
}

int rz_net_heads(rz_net *net, int32_t n_boards, float *d_logp, float *d_value, void *stream) {
    RZ_ENTER(net_ready, net, n_boards);
    if (n_boards == 0) return RZ_OK;
    if (!d_logp || !d_value) return rz_fail(RZ_ERR_ARG, "NULL device pointer");
    if (n_boards > net->feat_boards) return rz_fail(RZ_ERR_ARG, "batch larger than rz_net_reserve()d");
    return launch_heads(net, net->d_feat, n_boards, d_logp, d_value, stream);
}

int rz_net_forward(rz_net *net, const float *d_obs, int32_t n_boards, float *d_logp, float *d_value, void *stream) {
    RZ_ENTER(net_ready, net, n_boards);
    if (n_boards == 0) return RZ_OK;
    if (!d_obs || !d_logp || !d_value) return rz_fail(RZ_ERR_ARG, "NULL device pointer");
    if (net->fp8_cross)
        return rz_fail(RZ_ERR_ARG, "RZ_NET_SPLIT_F16_FP8 evaluates positions (rz_net_trunk_leaves*, rz_net_search_resident): float planes are refused, "
                                    "not computed in another arithmetic");
    if (n_boards > net->feat_boards)
        return rz_fail(RZ_ERR_ARG, "batch larger than rz_net_reserve()d (no allocation on the launch path)");
    launch_trunk(net, d_obs, net->d_feat, n_boards, stream);
    RZ_TRY(rz_launched("k_trunk"));
    return launch_heads(net, net->d_feat, n_boards, d_logp, d_value, stream);
}

}  // extern "C"
