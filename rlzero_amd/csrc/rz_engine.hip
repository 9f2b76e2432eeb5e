// rz_engine.hip -- MI355X (gfx950 / CDNA4) AlphaZero self-play MCTS engine.
//
// One 64-lane wavefront per game, one simulation in flight per tree (the reference runs
// its simulations strictly sequentially, rlzero/mcts/alphazero_mcts.py:82-85, so this is
// what bit-exact parity requires); the parallelism is across the lock-stepped games.
//
// Tree layout (HBM, one arena pair per game).  A node is ONE 32-byte record (two int4):
//   lo = {N   visit count                        (TreeNode.explore_count, rlzero/mcts/node.py:28),
//         FC  slot of the first child record, -1 = no child record yet,
//         NV  number of children already visited,
//         K | cap << 16:  K = legal moves at this node = len(TreeNode._children), 0 = not expanded;
//                         cap = child records reserved at FC}
//   hi = {Wsum float64 total value               (TreeNode.total_reward, node.py:29),
//         PB  offset of the node's block of K child priors (TreeNode.prior of each child, node.py:30),
//         the node's own prior (float bits; maintained for roots and for dense blocks)}
// so a level of the descent costs one 32-byte load per lane, all from one cache line.
// The reference's selection rule gives an unvisited child +inf and Python's max() keeps the first
// maximum (node.py:41-42,75-88), so the visited children of every node are always a PREFIX of its
// children in ascending action order: "first unvisited child" is child NV, no scan;
// a scan (coalesced, fp64 score, first-index tie-break across the wave) happens only once all K are
// visited.  Only VISITED children need a record, so the child records of a node are a contiguous
// vector [FC, FC + cap) that grows on demand (4, 8, 16 ... K: the wave copies the visited prefix to a
// new block at the top of the arena; the old block is reclaimed by the next re-root compaction).
// An 800-simulation search then touches ~1.5 k records (~50 KB per game, cache resident) instead of
// one K-slot block per expansion (~5 MB per game): the tree step is latency bound, and that
// latency is dominated by address translation and cache misses, not by instruction count.
// The K priors of an expanded node are written once, to a bump-allocated block of the separate
// prior arena (the reference's rule never reads them; the opt-in PUCT rule does).  PUCT mode
// reserves and initialises all K child records at expansion (cap = K) and always scans.
//
// Boards: two bitboards per game (4 x u64 per colour), cell = h*BW + w.  Gomoku / TicTacToe:
// action = cell (rlzero/games/gomoku/gomoku_env.py:227-234).  Connect4 (no reference
// implementation: build-defined, docs/open-spiel_alphazero.md:58 only mentions it): action =
// column, the stone drops to the lowest empty cell, row 0 is the bottom row.
//
// Bit-exactness: fp64 throughout, this file is compiled with
// -ffp-contract=off (q + c*u is two roundings in CPython), IEEE division and sqrt, and
// ln(parent N) comes from a table filled by the HOST libm -- the function CPython's
// math.log calls -- never from a device logarithm.
//
// This file is the host side of ONE translation unit: the kernels lie in headers beside it, one per family, each of which compiles
// alone (tests/test_csrc_headers.py) and describes its kernels where they are defined; the device code they all call is rz_tree.h.
//   rz_engine_step.h      the step-by-step tree kernels: k_select, k_expand_backup, k_expand_backup_raw, k_tree_step_raw, k_tree_step,
//                         and k_tree_step_vl, the sequential restatement of the in-flight kernel
//   rz_engine_deferred.h  deferred priors: k_expand_backup_def, k_tree_step_def, the flush (deferred_priors_body, k_deferred_priors)
//                         and the kept flush (Keep, k_keep_mark, k_keep_rows, k_deferred_priors_rows), k_deferred_reset
//   rz_engine_ml.h        k_tree_step_ml: K simulations in flight, level-synchronous (MlSlot, ml_lds_bytes)
//   rz_engine_eval.h      the synthetic and rollout evaluators: k_eval_synth, k_eval_rollout
//   rz_engine_roots.h     the root readers (k_root_children, k_root_stats, k_root_values), tree reuse (advance_body, k_advance), the
//                         game step (step_body, k_step_games) and the setters and getters of per-game state
//   rz_engine_play.h      the whole device move step: Play, k_play_draw, k_root_pruned, k_play_apply and the kernels of its options
// Below: g_err and rz_set_error, struct rz_engine, the launch helpers and every extern "C" entry point of the engine.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "rlzero_hip.h"
#include "rz_host.h"
#include "rz_trace.h"

#pragma clang fp contract(off)

#include "rz_tree.h"

// (this order is the order of the kernels in the code object; the template instantiations follow in the order the code below names them)
#include "rz_engine_step.h"
#include "rz_engine_deferred.h"
#include "rz_engine_ml.h"
#include "rz_engine_eval.h"
#include "rz_engine_roots.h"
#include "rz_engine_play.h"

using namespace rzt;

namespace {

thread_local char g_err[kRzErrBytes] = "";

}  // namespace

// rz_host.h (rz_fail): set the thread-local message returned by rz_last_error()
void rz_set_error(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg ? msg : ""); }

struct rz_engine {
    rz_config cfg;
    Dev dev;
    DevPool pool;   // every device array of the engine (rz_stats::device_bytes: its count)
    long long n_select = 0;
    int kb = 1, ks = 1;  // rz_set_in_flight: slots the next launches back up / select (sims_in_flight > 1 only)
    bool ml = false;     // sims_in_flight > 1: the level-synchronous kernel (default) instead of the sequential restatement
    int ml_lds = 0;
    double *d_logtab = nullptr;
    uint64_t *d_line_tab = nullptr;   // Dev::line_tab
    Play play = {};      // rz_play_attach
    bool play_seen = false;   // rz_play_attach has been called: `play` holds the arrays it got (all of them once play_on)
    bool play_on = false, play_drawn = false;
    long long play_steps = 0;   // move steps enqueued (rz_play_apply calls) since rz_play_attach
    float *play_vring = nullptr;   // rz_play_set_root_values: the caller's ring of root values (nullptr: off), an argument of k_play_draw
    int32_t *play_pring = nullptr;   // rz_play_set_pruned_visits: the caller's ring of pruned counts (nullptr: off), written by k_root_pruned in front of the draw
    // rz_set_playouts: the host's per-game simulation counts (and workgroup order) of the resident search, copies of the caller's
    int32_t *pl_counts = nullptr, *pl_order = nullptr;
    bool pl_on = false, pl_ordered = false;
    bool cap_ordered = true;   // rz_play_set_cap_order: k_play_order runs and the resident search follows it
    Keep keep = {};            // the kept flush (rz_deferred_keep): sized by rz_deferred_reserve
    int open_cap = 0;          // rz_play_set_match: openings the engine's copy of the table has room for
    double play_margin_cfg = 0.0;   // rz_play_config::stall_margin as given (rz_play_set_temperatures: 0 -> the margin follows the ply's T)
};

namespace {

int eng_ready(rz_engine *e) {
    if (e == nullptr) return rz_fail(RZ_ERR_ARG, "engine handle is NULL");
    return rz_on_device(e->cfg.device);
}

inline hipStream_t as_stream(void *s) { return (hipStream_t)s; }
inline dim3 per_game(const rz_engine *e) { return dim3((unsigned)e->cfg.n_games); }
inline dim3 per_leaf(const rz_engine *e) { return dim3((unsigned)(e->cfg.n_games * e->dev.K)); }
inline dim3 flat_grid(const rz_engine *e) { return dim3((unsigned)((e->cfg.n_games + 255) / 256)); }

// sims_in_flight > 1: every step-by-step route is one launch of the in-flight tree step -- the level-synchronous kernel, or its sequential
// restatement (rz_config::in_flight_impl); kb / ks: the slots it backs up / selects, 0 for a route that does only the other half
template <bool RAW>
int launch_in_flight(rz_engine *e, const float *logp, const float *value, const RawHeads &rh, float *obs, int kb, int ks, void *stream) {
    if (e->ml) k_tree_step_ml<RAW><<<per_game(e), dim3(kWave * e->dev.K), e->ml_lds, as_stream(stream)>>>(e->dev, logp, value, rh, obs, kb, ks);
    else k_tree_step_vl<RAW><<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, logp, value, rh, obs, kb, ks);
    return rz_launched("k_tree_step_vl");
}

}  // namespace

extern "C" {

int rz_abi_version(void) { return RZ_ABI_VERSION; }
#ifndef RZ_SOURCE_HASH
#define RZ_SOURCE_HASH "unknown"   /* rlzero_amd/_build.py passes the hash of sources + headers + flags */
#endif
// the marker is what rlzero_amd/_build.py searches the library's bytes for (no need to load it); the accessor returns the hash alone
const char *rz_source_hash(void) {
    static const char marker[] = "RZ_SOURCE_HASH=" RZ_SOURCE_HASH;
    return marker + 15;
}
const char *rz_last_error(void) { return g_err; }

int rz_create(const rz_config *cfg, rz_engine **out) {
    if (cfg == nullptr || out == nullptr) return rz_fail(RZ_ERR_ARG, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->abi_version != RZ_ABI_VERSION)
        return rz_fail(RZ_ERR_ARG, "abi_version %d != library %d", cfg->abi_version, RZ_ABI_VERSION);
    int BH, BW, A, n_row = cfg->n_in_row;
    if (cfg->game_kind == RZ_GAME_GOMOKU) {
        if (cfg->board_size < 1 || cfg->board_size > RZ_MAX_BOARD_SIZE)
            return rz_fail(RZ_ERR_ARG, "board_size %d not in 1..%d", cfg->board_size, RZ_MAX_BOARD_SIZE);
        BH = BW = cfg->board_size;
        A = BH * BW;
    } else if (cfg->game_kind == RZ_GAME_CONNECT4) {
        BH = cfg->board_height > 0 ? cfg->board_height : 6;
        BW = cfg->board_width > 0 ? cfg->board_width : 7;
        if (n_row == 0) n_row = 4;
        if (BH > RZ_MAX_BOARD_SIZE || BW > RZ_MAX_BOARD_SIZE)
            return rz_fail(RZ_ERR_ARG, "board %dx%d exceeds %d", BH, BW, RZ_MAX_BOARD_SIZE);
        A = BW;
    } else {
        return rz_fail(RZ_ERR_ARG, "unknown game_kind %d", cfg->game_kind);
    }
    if (n_row < 1 || (n_row > BH && n_row > BW)) return rz_fail(RZ_ERR_ARG, "n_in_row %d does not fit the board", n_row);
    if (cfg->n_games < 1) return rz_fail(RZ_ERR_ARG, "n_games must be >= 1");
    if (cfg->n_playout < 1) return rz_fail(RZ_ERR_ARG, "n_playout must be >= 1");
    if (cfg->score_mode != RZ_SCORE_UCT_REF && cfg->score_mode != RZ_SCORE_PUCT)
        return rz_fail(RZ_ERR_ARG, "unknown score_mode %d", cfg->score_mode);
    if (!(cfg->c_puct >= 0.0)) return rz_fail(RZ_ERR_ARG, "c_puct must be >= 0");
    if (cfg->sims_in_flight < 0 || cfg->sims_in_flight > RZ_MAX_IN_FLIGHT)
        return rz_fail(RZ_ERR_ARG, "sims_in_flight %d not in 0..%d", cfg->sims_in_flight, RZ_MAX_IN_FLIGHT);
    if (cfg->in_flight_impl != 0 && cfg->in_flight_impl != 1) return rz_fail(RZ_ERR_ARG, "unknown in_flight_impl %d", cfg->in_flight_impl);
    int n_dev = 0;
    RZ_HIP(hipGetDeviceCount(&n_dev));
    if (cfg->device < 0 || cfg->device >= n_dev)
        return rz_fail(RZ_ERR_ARG, "device %d not in 0..%d", cfg->device, n_dev - 1);
    RZ_HIP(hipSetDevice(cfg->device));

    rz_engine *e = new (std::nothrow) rz_engine();
    if (e == nullptr) return rz_fail(RZ_ERR_OOM, "host allocation failed");
    e->cfg = *cfg;
    Dev &D = e->dev;
    memset(&D, 0, sizeof(D));
    const int S = BH * BW;
    const double pf = cfg->pool_factor > 0.0 ? cfg->pool_factor : 2.0;
    D.kind = cfg->game_kind;
    D.BH = BH;
    D.BW = BW;
    D.S = S;
    D.A = A;
    D.n_row = n_row;
    D.bw_rcp = (65536 + BW - 1) / BW;
    for (int y = 0; y < BH && S <= 64; ++y) D.col0 |= 1ull << (y * BW);
    D.n_rcp = (65536 + n_row - 1) / n_row;
    D.n_games = cfg->n_games;
    D.n_playout = cfg->n_playout;
    D.K = cfg->sims_in_flight > 1 ? cfg->sims_in_flight : 1;
    e->kb = e->ks = D.K;
    e->ml = D.K > 1 && cfg->in_flight_impl == 0;
    if (e->ml) {
        e->ml_lds = ml_lds_bytes(D.K, A, cfg->score_mode == RZ_SCORE_PUCT);
        if (e->ml_lds > 160 * 1024) {
            const int need = e->ml_lds;
            delete e;
            return rz_fail(RZ_ERR_ARG, "sims_in_flight %d x %d actions needs %d bytes of LDS (> 160 KB)", cfg->sims_in_flight, A, need);
        }
        // the attribute belongs to the kernel, not to this engine: set to the hardware's 160 KB once and for all, so that a
        // later engine with a smaller K x A cannot lower it under an earlier, larger one
        const int most = 160 * 1024;
        hipError_t a1 = hipFuncSetAttribute((const void *)k_tree_step_ml<true>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
        hipError_t a2 = hipFuncSetAttribute((const void *)k_tree_step_ml<false>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
        if (a1 != hipSuccess || a2 != hipSuccess) {
            delete e;
            return rz_fail(RZ_ERR_HIP, "hipFuncSetAttribute(dynamic LDS %d bytes) failed", most);
        }
    }
    D.score_mode = cfg->score_mode;
    D.add_noise = cfg->add_noise ? 1 : 0;
    D.noise_seed = (uint64_t)(uint32_t)cfg->noise_seed;
    D.c_puct = cfg->c_puct;
    // qcap expanded nodes (= prior blocks) per arena: this move's n_playout plus a carried subtree of
    // up to pf * n_playout.  Record slots: dense (PUCT) = one K-block per expansion; otherwise only
    // visited nodes hold records, at most ~3 slots per simulation with the doubling child vectors
    // (typically ~2), so 16 per expansion leaves a wide margin.
    D.qcap = (int)((pf + 1.0) * (double)cfg->n_playout) + 8;
    D.pcap = (long long)D.qcap * A;
    D.cap = cfg->score_mode == RZ_SCORE_PUCT ? (long long)D.qcap * A + 2
                                             : (long long)D.qcap * 16 + 2 * A + 64;
    D.path_stride = S + 2;
    D.logtab_n = (long long)cfg->n_playout * (S + 1) + 2;
    for (int j = 0; j < kWords; ++j) {
        const int lo = 64 * j;
        D.valid[j] = S >= lo + 64 ? ~0ull : (S > lo ? ((1ull << (S - lo)) - 1ull) : 0ull);
    }
    const long long G = cfg->n_games, GL = G * D.K;  // games, leaves in flight
    const long long slots = G * 2 * D.cap;
    if (D.cap >= (1ll << 30) || D.pcap >= (1ll << 31))
    {
        delete e;
        return rz_fail(RZ_ERR_ARG, "n_playout %d is too large for 32-bit slot indices", cfg->n_playout);
    }
    int rc = RZ_OK;
#define RZ_ALLOC(field, count)                               \
    if (rc == RZ_OK) rc = e->pool.alloc(&D.field, (count))
    RZ_ALLOC(R, slots * 2);
    RZ_ALLOC(P, G * 2 * D.pcap);
    RZ_ALLOC(cur_arena, G);
    RZ_ALLOC(top, G);
    RZ_ALLOC(ptop, G);
    RZ_ALLOC(nblk, G);
    RZ_ALLOC(root_stones, G * 2 * kWords);
    RZ_ALLOC(root_to_move, G);
    RZ_ALLOC(root_last, G);
    RZ_ALLOC(active, G);
    RZ_ALLOC(path, GL * D.path_stride);
    RZ_ALLOC(leaf_node, GL);
    RZ_ALLOC(leaf_depth, GL);
    RZ_ALLOC(leaf_fresh, GL);
    RZ_ALLOC(leaf_term, GL);
    RZ_ALLOC(leaf_tval, GL);
    RZ_ALLOC(leaf_stones, GL * 2 * kWords);
    RZ_ALLOC(leaf_to_move, GL);
    RZ_ALLOC(leaf_last, GL);
    RZ_ALLOC(queue, G * D.qcap);
    RZ_ALLOC(err, G);
    RZ_ALLOC(err_any, 1);
    RZ_ALLOC(reuse_drops, 1);
    RZ_ALLOC(noise_ctr, G);
    RZ_ALLOC(noise_key, G);
    if (rc == RZ_OK) rc = e->pool.alloc(&e->d_logtab, D.logtab_n);
    if (rc == RZ_OK) rc = e->pool.alloc(&e->d_line_tab, 2 * kWave);
#undef RZ_ALLOC
    if (rc != RZ_OK) {
        rz_destroy(e);
        return rc;
    }
    D.logtab = e->d_logtab;
    D.line_tab = e->d_line_tab;
    // zero the small state; arenas need no initialisation beyond the root slot
    hipError_t herr = hipSuccess;
    auto zero = [&](void *p, size_t bytes) { if (herr == hipSuccess) herr = hipMemset(p, 0, bytes); };
    zero(D.cur_arena, G * 4); zero(D.top, G * 4); zero(D.ptop, G * 4); zero(D.nblk, G * 4);
    zero(D.root_stones, G * 2 * kWords * 8); zero(D.root_to_move, G * 4);
    zero(D.leaf_node, GL * 4); zero(D.leaf_depth, GL * 4); zero(D.leaf_fresh, GL * 4);
    zero(D.leaf_term, GL * 4); zero(D.leaf_tval, GL * 8); zero(D.leaf_stones, GL * 2 * kWords * 8);
    zero(D.leaf_to_move, GL * 4); zero(D.path, GL * D.path_stride * 4);
    zero(D.err, G * 4); zero(D.err_any, 4); zero(D.reuse_drops, 4); zero(D.noise_ctr, G * 4);
    if (herr == hipSuccess) herr = hipMemset(D.root_last, 0xff, G * 4);  // -1
    if (herr == hipSuccess) herr = hipMemset(D.leaf_last, 0xff, GL * 4);
    if (herr == hipSuccess) herr = hipMemset(D.active, 1, G);
    if (herr != hipSuccess) {
        rz_destroy(e);
        return rz_fail(RZ_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(herr));
    }
    {
        std::vector<double> tab((size_t)D.logtab_n);
        tab[0] = 0.0;
        for (long long i = 1; i < D.logtab_n; ++i) tab[(size_t)i] = std::log((double)i);
        herr = hipMemcpy(e->d_logtab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
        if (herr != hipSuccess) {
            rz_destroy(e);
            return rz_fail(RZ_ERR_HIP, "hipMemcpy(log table) failed: %s", hipGetErrorString(herr));
        }
    }
    {   // Dev::line_tab: the window of lane l -- bits j * stride of its n cells (boards of up to 128 cells: a low word [l] and a high word
        // [64 + l], the high one empty unless a window spans 64 cell numbers or more); boards of more cells: its first n - 1 cells in [l],
        // and line_masks says whether those fit
        uint64_t tab[2 * kWave] = {0};
        const int cells = S <= 128 ? n_row : n_row - 1;
        D.line_masks = (cells - 1) * (BW + 1) < 64 ? 1 : 0;
        for (int l = 0; l < kWave && l < 4 * n_row; ++l) {
            const int d = l / n_row, stride = d == 0 ? 1 : d == 1 ? BW : d == 2 ? BW + 1 : BW - 1;
            for (int j = 0; j < cells; ++j) {
                const int o = j * stride;
                if (o < 64) tab[l] |= 1ull << o;
                else if (o < 128) tab[kWave + l] |= 1ull << (o - 64);
            }
        }
        herr = hipMemcpy(e->d_line_tab, tab, sizeof(tab), hipMemcpyHostToDevice);
        if (herr != hipSuccess) {
            rz_destroy(e);
            return rz_fail(RZ_ERR_HIP, "hipMemcpy(line table) failed: %s", hipGetErrorString(herr));
        }
    }
    {   // fresh trees
        std::vector<int32_t> mv((size_t)G, -1);
        DevBuf<int32_t> d_mv;
        herr = d_mv.alloc(G * 4) ? hipSuccess : hipErrorOutOfMemory;
        if (herr == hipSuccess) herr = hipMemcpy(d_mv, mv.data(), G * 4, hipMemcpyHostToDevice);
        if (herr == hipSuccess) {
            k_advance<<<dim3((unsigned)G), dim3(kWave), 0, 0>>>(D, d_mv);
            k_set_noise_keys<<<dim3((unsigned)((G + 255) / 256)), dim3(256), 0, 0>>>(D, nullptr, nullptr);   // the default keys
            herr = hipDeviceSynchronize();
        }
        d_mv.release();
        if (herr != hipSuccess) {
            rz_destroy(e);
            return rz_fail(RZ_ERR_HIP, "tree initialisation failed: %s", hipGetErrorString(herr));
        }
    }
    *out = e;
    return RZ_OK;
}

int rz_destroy(rz_engine *e) {
    if (e == nullptr) return RZ_OK;
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
    delete e;   // (the pool frees)
    return RZ_OK;
}

int rz_geometry(rz_engine *e, int32_t *height, int32_t *width, int32_t *n_actions) {
    if (e == nullptr) return rz_fail(RZ_ERR_ARG, "engine handle is NULL");
    if (height) *height = e->dev.BH;
    if (width) *width = e->dev.BW;
    if (n_actions) *n_actions = e->dev.A;
    return RZ_OK;
}

int rz_upload_log_table(rz_engine *e, const double *h_table, int64_t count) {
    RZ_ENTER(eng_ready, e);
    if (h_table == nullptr || count < 2) return rz_fail(RZ_ERR_ARG, "table is NULL or too short");
    if (count > e->dev.logtab_n) count = e->dev.logtab_n;
    RZ_HIP(hipDeviceSynchronize());
    RZ_HIP(hipMemcpy(e->d_logtab, h_table, (size_t)count * sizeof(double), hipMemcpyHostToDevice));
    return RZ_OK;
}

int rz_log_table_size(rz_engine *e, int64_t *count) {
    if (e == nullptr || count == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    *count = e->dev.logtab_n;
    return RZ_OK;
}

// an entry point of the move step: a valid engine that rz_play_attach has been called on
#define RZ_ENTER_PLAY(e)                                                                  \
    do {                                                                                  \
        RZ_ENTER(eng_ready, e);                                                           \
        if (!(e)->play_on) return rz_fail(RZ_ERR_ARG, "call rz_play_attach first");       \
    } while (0)
// per-game simulation counts exist in the resident search only (rz_net_search_resident): the step-by-step routes refuse them
#define RZ_NO_PLAYOUTS(e)                                                                                                             \
    do {                                                                                                                              \
        if ((e)->pl_on || ((e)->play_on && (e)->play.cap_on))                                                                         \
            return rz_fail(RZ_ERR_ARG, "%s: per-game simulation counts (rz_set_playouts, rz_play_set_cap) are served by the "          \
                                       "resident search only (rz_net_search_resident); clear them for this route", __func__);        \
    } while (0)

int rz_set_roots(rz_engine *e, const uint64_t *d_stones, const int32_t *d_to_move,
                 const int32_t *d_last_move, const uint8_t *d_mask, int reset_trees, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_stones); RZ_NEED(d_to_move); RZ_NEED(d_last_move);
    k_set_roots<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev, d_stones, d_to_move,
                                                                   d_last_move, d_mask, reset_trees);
    return rz_launched("k_set_roots");
}

int rz_get_roots(rz_engine *e, uint64_t *d_stones, int32_t *d_to_move, int32_t *d_last_move,
                 void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_stones); RZ_NEED(d_to_move); RZ_NEED(d_last_move);
    k_get_roots<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev, d_stones, d_to_move, d_last_move);
    return rz_launched("k_get_roots");
}

int rz_set_active(rz_engine *e, const uint8_t *d_active, void *stream) {
    RZ_ENTER(eng_ready, e);
    k_set_active<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev, d_active);
    return rz_launched("k_set_active");
}

int rz_set_noise_keys(rz_engine *e, const uint64_t *d_keys, const uint8_t *d_mask, void *stream) {
    RZ_ENTER(eng_ready, e);
    k_set_noise_keys<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev, d_keys, d_mask);
    return rz_launched("k_set_noise_keys");
}

int rz_set_in_flight(rz_engine *e, int32_t k_backup, int32_t k_select) {
    if (e == nullptr) return rz_fail(RZ_ERR_ARG, "engine handle is NULL");
    if (k_backup < 0 || k_backup > e->dev.K || k_select < 0 || k_select > e->dev.K)
        return rz_fail(RZ_ERR_ARG, "in-flight counts (%d, %d) not in 0..%d", k_backup, k_select, e->dev.K);
    e->kb = k_backup;
    e->ks = k_select;
    return RZ_OK;
}

int rz_select_step(rz_engine *e, float *d_obs, void *stream) {
    RZ_ENTER(eng_ready, e);
    e->n_select += 1;
    if (e->dev.K > 1) return launch_in_flight<false>(e, nullptr, nullptr, RawHeads(), d_obs, 0, e->ks, stream);
    k_select<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, d_obs);
    return rz_launched("k_select");
}

int rz_leaf_buffers(rz_engine *e, const uint64_t **d_stones, const int32_t **d_to_move, const int32_t **d_last_cell) {
    if (e == nullptr || !d_stones || !d_to_move || !d_last_cell) return rz_fail(RZ_ERR_ARG, "NULL argument");
    *d_stones = e->dev.leaf_stones;
    *d_to_move = e->dev.leaf_to_move;
    *d_last_cell = e->dev.leaf_last;
    return RZ_OK;
}

int rz_encode_leaf_obs(rz_engine *e, float *d_obs, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_obs);
    k_encode<<<per_leaf(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, 0, d_obs);
    return rz_launched("k_encode");
}

int rz_encode_root_obs(rz_engine *e, float *d_obs, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_obs);
    k_encode<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, 1, d_obs);
    return rz_launched("k_encode");
}

int rz_get_leaves(rz_engine *e, uint64_t *d_stones, int32_t *d_to_move, int32_t *d_last_move,
                  int32_t *d_terminal, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_stones); RZ_NEED(d_to_move); RZ_NEED(d_last_move); RZ_NEED(d_terminal);
    if (e->dev.K > 1) return rz_fail(RZ_ERR_ARG, "rz_get_leaves serves host evaluators: not available with sims_in_flight > 1");
    k_get_leaves<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev, d_stones, d_to_move,
                                                                    d_last_move, d_terminal);
    return rz_launched("k_get_leaves");
}

int rz_eval_synthetic(rz_engine *e, int kind, float *d_logp, float *d_value, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_value);
    if (kind != RZ_EVAL_V0 && kind != RZ_EVAL_VLIN) return rz_fail(RZ_ERR_ARG, "unknown evaluator %d", kind);
    k_eval_synth<<<per_leaf(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, kind, d_logp, d_value);
    return rz_launched("k_eval_synth");
}

int rz_eval_rollout(rz_engine *e, uint64_t seed, uint32_t sim_index, int32_t n_limit, float *d_value,
                    void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_value);
    if (n_limit < 0) return rz_fail(RZ_ERR_ARG, "n_limit must be >= 0");
    k_eval_rollout<<<per_leaf(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, seed, sim_index, n_limit, d_value);
    return rz_launched("k_eval_rollout");
}

int rz_expand_backup(rz_engine *e, const float *d_logp, const float *d_value, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NO_PLAYOUTS(e);
    RZ_NEED(d_value);
    if (e->dev.K > 1) return launch_in_flight<false>(e, d_logp, d_value, RawHeads(), nullptr, e->kb, 0, stream);
    k_expand_backup<float><<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, d_logp, d_value);
    return rz_launched("k_expand_backup");
}

int rz_expand_backup_f64(rz_engine *e, const float *d_logp, const double *d_value, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NO_PLAYOUTS(e);
    RZ_NEED(d_value);
    if (e->dev.K > 1) return rz_fail(RZ_ERR_ARG, "host evaluators are not available with sims_in_flight > 1");
    k_expand_backup<double><<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, d_logp, d_value);
    return rz_launched("k_expand_backup");
}

int rz_expand_backup_probs(rz_engine *e, const float *d_probs, const double *d_value, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NO_PLAYOUTS(e);
    RZ_NEED(d_value);
    if (e->dev.K > 1) return rz_fail(RZ_ERR_ARG, "host evaluators are not available with sims_in_flight > 1");
    k_expand_backup<double, true><<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, d_probs, d_value);
    return rz_launched("k_expand_backup");
}

int rz_tree_step(rz_engine *e, const float *d_logp, const float *d_value, float *d_obs, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NO_PLAYOUTS(e);
    RZ_NEED(d_value);
    e->n_select += 1;
    if (e->dev.K > 1) return launch_in_flight<false>(e, d_logp, d_value, RawHeads(), d_obs, e->kb, e->ks, stream);
    k_tree_step<float><<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, d_logp, d_value, d_obs);
    return rz_launched("k_tree_step");
}

static int raw_heads_ok(rz_engine *e, const rz_raw_heads *h) {
    if (!h || !h->raw || !h->hid || !h->w2 || !h->b2) return rz_fail(RZ_ERR_ARG, "NULL device pointer");
    if (h->ld < e->dev.A) return rz_fail(RZ_ERR_ARG, "ld %d < n_actions %d", h->ld, e->dev.A);
    if (h->n_parts != 1 && h->n_parts != 4) return rz_fail(RZ_ERR_ARG, "n_parts %d is neither 1 nor 4", h->n_parts);
    if (h->n_parts == 4 && (!h->act_scale || !h->act_bias || !h->val_scale || !h->val_bias))
        return rz_fail(RZ_ERR_ARG, "partial sums need their scales and biases");
    return RZ_OK;
}

int rz_expand_backup_raw(rz_engine *e, const rz_raw_heads *heads, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NO_PLAYOUTS(e);
    RZ_TRY(raw_heads_ok(e, heads));
    const RawHeads rh = *heads;
    if (e->dev.K > 1) return launch_in_flight<true>(e, nullptr, nullptr, rh, nullptr, e->kb, 0, stream);
    k_expand_backup_raw<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, rh);
    return rz_launched("k_expand_backup_raw");
}

static int deferred_ok(rz_engine *e, const rz_value_head *h) {
    if (h == nullptr || !h->valfeat || !h->w1t || !h->b1 || !h->w2 || !h->b2) return rz_fail(RZ_ERR_ARG, "rz_value_head: NULL pointer");
    if ((h->groups != 16 && h->groups != 32 && h->groups != 64 && h->groups != 128) || h->ld != 4 * h->groups)
        return rz_fail(RZ_ERR_ARG, "rz_value_head: groups = %d must be 16, 32, 64 or 128 and ld = 4 * groups", h->groups);
    if (2 * e->dev.S > 4 * h->groups)   // (the kernels also size their bitboard arithmetic by it: words_of_per)
        return rz_fail(RZ_ERR_ARG, "rz_value_head: %d groups of 4 inputs do not hold the 2 x %d inputs of this board", h->groups, e->dev.S);
    if (e->dev.pend_cap <= 0) return rz_fail(RZ_ERR_ARG, "call rz_deferred_reserve first");
    return RZ_OK;
}

int rz_deferred_reserve(rz_engine *e, int32_t slots) {
    RZ_ENTER(eng_ready, e);
    if (slots < 1) return rz_fail(RZ_ERR_ARG, "rz_deferred_reserve: slots must be positive");
    if (e->cfg.score_mode != RZ_SCORE_UCT_REF || e->dev.K != 1)
        return rz_fail(RZ_ERR_ARG, "deferred priors need RZ_SCORE_UCT_REF (the rule that never reads a prior) and sims_in_flight == 1");
    if (slots <= e->dev.pend_cap) return RZ_OK;
    RZ_HIP(hipDeviceSynchronize());
    const long long G = e->cfg.n_games;
    // (the records of a smaller reservation stay allocated until rz_destroy: reservations grow once or twice in a process)
    RZ_TRY(e->pool.alloc(&e->dev.pend_pb, (long long)slots * G));
    RZ_TRY(e->pool.alloc(&e->dev.pend_ctr, (long long)slots * G));
    RZ_TRY(e->pool.alloc(&e->dev.pend_lw, (long long)slots * G));
    RZ_TRY(e->pool.alloc(&e->dev.pend_stones, (long long)slots * G * 2 * kWords));
    if (e->dev.pend == nullptr) {
        RZ_TRY(e->pool.alloc(&e->dev.pend, G));
    }
    RZ_HIP(hipMemset(e->dev.pend, 0, (size_t)G * sizeof(int32_t)));
    // the kept flush: a mask bit and a place in the row list per record, two counts per game
    Keep &kp = e->keep;
    kp.words = (slots + 63) / 64;
    RZ_TRY(e->pool.alloc(&kp.mask, (long long)kp.words * G));
    RZ_TRY(e->pool.alloc(&kp.rows, (long long)slots * G));
    if (kp.cnt == nullptr) {
        RZ_TRY(e->pool.alloc(&kp.cnt, G));
        RZ_TRY(e->pool.alloc(&kp.pcnt, G));
        RZ_TRY(e->pool.alloc(&kp.count, 1));
        RZ_TRY(e->pool.alloc(&kp.stats, 2));
        RZ_HIP(hipMemset(kp.stats, 0, 2 * sizeof(unsigned long long)));
    }
    RZ_HIP(hipMemset(kp.count, 0, sizeof(int32_t)));
    e->dev.pend_cap = slots;
    return RZ_OK;
}

int rz_trace_attach(rz_engine *e, void *d_trace) {
    RZ_ENTER(eng_ready, e);
    e->dev.trace = (unsigned long long *)d_trace;
    return RZ_OK;
}

int rz_device_view(rz_engine *e, void *out, int64_t out_bytes) {
    RZ_ENTER(eng_ready, e);
    if (out == nullptr || out_bytes != (int64_t)sizeof(Dev)) return rz_fail(RZ_ERR_ARG, "rz_device_view: the caller's view is %lld bytes, the engine's %zu", (long long)out_bytes, sizeof(Dev));
    memcpy(out, &e->dev, sizeof(Dev));
    return RZ_OK;
}

int rz_deferred_slots(rz_engine *e, const int32_t **d_slot_of_game) {
    RZ_ENTER(eng_ready, e);
    if (!d_slot_of_game) return rz_fail(RZ_ERR_ARG, "NULL output pointer");
    if (e->dev.pend_cap <= 0) return rz_fail(RZ_ERR_ARG, "call rz_deferred_reserve first");
    *d_slot_of_game = e->dev.pend;
    return RZ_OK;
}

int rz_expand_backup_deferred(rz_engine *e, const rz_value_head *head, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_TRY(deferred_ok(e, head));
    RZ_NO_PLAYOUTS(e);
    const dim3 block(kWave * kDefWaves);
    switch (head->groups) {   // = 4 waves x 2 halves x PER
        case 16: k_expand_backup_def<2><<<per_game(e), block, 0, as_stream(stream)>>>(e->dev, *head); break;
        case 32: k_expand_backup_def<4><<<per_game(e), block, 0, as_stream(stream)>>>(e->dev, *head); break;
        case 64: k_expand_backup_def<8><<<per_game(e), block, 0, as_stream(stream)>>>(e->dev, *head); break;
        default: k_expand_backup_def<16><<<per_game(e), block, 0, as_stream(stream)>>>(e->dev, *head); break;
    }
    return rz_launched("k_expand_backup_def");
}

int rz_tree_step_deferred(rz_engine *e, const rz_value_head *head, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_TRY(deferred_ok(e, head));
    RZ_NO_PLAYOUTS(e);
    e->n_select += 1;
    const dim3 block(kWave * kDefWaves);
    if (e->dev.trace && head->groups == 128) {   // (the traced instantiation exists for the 15 x 15 board's head: rz_trace_attach)
        k_tree_step_def<16, true><<<per_game(e), block, 0, as_stream(stream)>>>(e->dev, *head, nullptr);
        return rz_launched("k_tree_step_def");
    }
    switch (head->groups) {   // = 4 waves x 2 halves x PER
        case 16: k_tree_step_def<2, false><<<per_game(e), block, 0, as_stream(stream)>>>(e->dev, *head, nullptr); break;
        case 32: k_tree_step_def<4, false><<<per_game(e), block, 0, as_stream(stream)>>>(e->dev, *head, nullptr); break;
        case 64: k_tree_step_def<8, false><<<per_game(e), block, 0, as_stream(stream)>>>(e->dev, *head, nullptr); break;
        default: k_tree_step_def<16, false><<<per_game(e), block, 0, as_stream(stream)>>>(e->dev, *head, nullptr); break;
    }
    return rz_launched("k_tree_step_def");
}

int rz_deferred_flush(rz_engine *e, const rz_deferred_logits *logits, int32_t n_slots, void *stream) {
    RZ_ENTER(eng_ready, e);
    if (e->dev.pend_cap <= 0 || n_slots <= 0) return RZ_OK;
    if (!logits || !logits->raw) return rz_fail(RZ_ERR_ARG, "rz_deferred_logits: NULL pointer");
    if (n_slots > e->dev.pend_cap) return rz_fail(RZ_ERR_ARG, "more slots than rz_deferred_reserve()d");
    if (logits->ld < e->dev.A || logits->rows_per_slot < e->cfg.n_games) return rz_fail(RZ_ERR_ARG, "rz_deferred_logits: rows shorter than the batch");
    k_deferred_priors<<<dim3((unsigned)e->cfg.n_games, (unsigned)n_slots), dim3(kWave), 0, as_stream(stream)>>>(
        e->dev, logits->raw, logits->ld, (long long)logits->rows_per_slot);
    // (between rz_play_draw and rz_play_apply the counters restart in k_play_apply: one launch less in the chain of a move)
    if (!(e->play_on && e->play_drawn)) k_deferred_reset<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev);
    return rz_launched("k_deferred_priors");
}

static int keep_ok(rz_engine *e) {
    if (e->dev.pend_cap <= 0) return rz_fail(RZ_ERR_ARG, "call rz_deferred_reserve first");
    if (!(e->play_on && e->play_drawn)) return rz_fail(RZ_ERR_ARG, "the kept flush runs between rz_play_draw and rz_play_apply (the move decides what is kept)");
    return RZ_OK;
}

int rz_deferred_keep(rz_engine *e, rz_kept_rows *out, void *stream) {
    RZ_ENTER(eng_ready, e);
    if (!out) return rz_fail(RZ_ERR_ARG, "NULL output pointer");
    RZ_TRY(keep_ok(e));
    k_keep_mark<<<per_game(e), dim3(256), 0, as_stream(stream)>>>(e->dev, e->play.keep, e->keep);
    k_keep_rows<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, e->keep);
    out->rows = e->keep.rows;
    out->count = e->keep.count;
    out->capacity = (int64_t)e->dev.pend_cap * e->cfg.n_games;
    out->n_games = e->cfg.n_games;
    out->reserved = 0;
    return rz_launched("k_keep_rows");
}

int rz_deferred_keep_all(rz_engine *e, rz_kept_rows *out, void *stream) {
    RZ_ENTER(eng_ready, e);
    if (!out) return rz_fail(RZ_ERR_ARG, "NULL output pointer");
    if (e->dev.pend_cap <= 0) return rz_fail(RZ_ERR_ARG, "call rz_deferred_reserve first");
    Keep all = e->keep;
    all.stats = nullptr;
    k_keep_mark<<<per_game(e), dim3(256), 0, as_stream(stream)>>>(e->dev, nullptr, all);
    k_keep_rows<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, all);
    out->rows = e->keep.rows;
    out->count = e->keep.count;
    out->capacity = (int64_t)e->dev.pend_cap * e->cfg.n_games;
    out->n_games = e->cfg.n_games;
    out->reserved = 0;
    return rz_launched("k_keep_rows");
}

int rz_deferred_flush_rows(rz_engine *e, const rz_deferred_logits *logits, void *stream) {
    RZ_ENTER(eng_ready, e);
    if (e->dev.pend_cap <= 0) return rz_fail(RZ_ERR_ARG, "call rz_deferred_reserve first");
    if (!logits || !logits->raw) return rz_fail(RZ_ERR_ARG, "rz_deferred_logits: NULL pointer");
    if (logits->ld < e->dev.A) return rz_fail(RZ_ERR_ARG, "rz_deferred_logits: rows shorter than the policy");
    k_deferred_priors_rows<<<dim3(2048), dim3(kWave), 0, as_stream(stream)>>>(e->dev, logits->raw, logits->ld, e->keep.rows, e->keep.count);
    // (between rz_play_draw and rz_play_apply the counters restart in k_play_apply, as in rz_deferred_flush)
    if (!(e->play_on && e->play_drawn)) k_deferred_reset<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev);
    return rz_launched("k_deferred_priors_rows");
}

int rz_deferred_flush_kept(rz_engine *e, const rz_deferred_logits *logits, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_TRY(keep_ok(e));
    if (!logits || !logits->raw) return rz_fail(RZ_ERR_ARG, "rz_deferred_logits: NULL pointer");
    if (logits->ld < e->dev.A) return rz_fail(RZ_ERR_ARG, "rz_deferred_logits: rows shorter than the policy");
    // (eight waves per CU of a large chip; the counters restart in k_play_apply)
    k_deferred_priors_rows<<<dim3(2048), dim3(kWave), 0, as_stream(stream)>>>(e->dev, logits->raw, logits->ld, e->keep.rows, e->keep.count);
    return rz_launched("k_deferred_priors_rows");
}

int rz_deferred_keep_stats(rz_engine *e, uint64_t *h_out2, int32_t reset) {
    RZ_ENTER(eng_ready, e);
    if (!h_out2) return rz_fail(RZ_ERR_ARG, "NULL output pointer");
    h_out2[0] = h_out2[1] = 0;
    if (!e->keep.stats) return RZ_OK;
    RZ_HIP(hipDeviceSynchronize());
    RZ_HIP(hipMemcpy(h_out2, e->keep.stats, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) RZ_HIP(hipMemset(e->keep.stats, 0, 2 * sizeof(uint64_t)));
    return RZ_OK;
}

int rz_tree_step_raw(rz_engine *e, const rz_raw_heads *heads, float *d_obs, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NO_PLAYOUTS(e);
    RZ_TRY(raw_heads_ok(e, heads));
    e->n_select += 1;
    const RawHeads rh = *heads;
    if (e->dev.K > 1) return launch_in_flight<true>(e, nullptr, nullptr, rh, d_obs, e->kb, e->ks, stream);
    k_tree_step_raw<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, rh, d_obs);
    return rz_launched("k_tree_step_raw");
}

int rz_root_visits(rz_engine *e, int32_t *d_visits, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_visits);
    k_root_children<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, 0, d_visits);
    return rz_launched("k_root_children");
}

int rz_root_wsum(rz_engine *e, double *d_w, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_w);
    k_root_children<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, 1, d_w);
    return rz_launched("k_root_children");
}

int rz_root_priors(rz_engine *e, float *d_p, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_p);
    k_root_children<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, 2, d_p);
    return rz_launched("k_root_children");
}

int rz_root_stats(rz_engine *e, int32_t *d_n, double *d_w, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_n); RZ_NEED(d_w);
    k_root_stats<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev, d_n, d_w);
    return rz_launched("k_root_stats");
}

int rz_root_values(rz_engine *e, double *d_out, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_out);
    k_root_values<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, d_out);
    return rz_launched("k_root_values");
}

int rz_set_forced_playouts(rz_engine *e, double k) {
    RZ_ENTER(eng_ready, e);
    if (!(std::isfinite(k) && k >= 0.0)) return rz_fail(RZ_ERR_ARG, "rz_set_forced_playouts: k = %g is not a finite number >= 0", k);
    // (a match first: today it runs under RZ_SCORE_UCT_REF only, and the sentence a caller reads should name what it turned on)
    if (e->play_on && e->play.match_on) return rz_fail(RZ_ERR_ARG, "rz_set_forced_playouts: a match is on (rz_play_set_match): its games are not training data");
    if (e->dev.score_mode != RZ_SCORE_PUCT) return rz_fail(RZ_ERR_ARG, "rz_set_forced_playouts: forced playouts are a rule of RZ_SCORE_PUCT (this engine selects by RZ_SCORE_UCT_REF)");
    if (e->dev.K != 1) return rz_fail(RZ_ERR_ARG, "rz_set_forced_playouts: one simulation in flight per tree only (sims_in_flight = %d)", e->dev.K);
    // k travels in the kernel arguments: a move step enqueued -- or captured into a whole-move graph -- keeps the one it had, and the
    // ring of pruned counts was handed over for the k it was set under
    if (e->play_on && (e->play_steps > 0 || e->play_drawn || e->play_pring != nullptr))
        return rz_fail(RZ_ERR_ARG, "rz_set_forced_playouts: the move step holds k since rz_play_attach (attach again)");
    e->dev.forced_k = k;
    return RZ_OK;
}

int rz_root_pruned_visits(rz_engine *e, int32_t *d_out, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_out);
    k_root_pruned<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, e->play, d_out, 0);
    return rz_launched("k_root_pruned");
}

int rz_play_set_pruned_visits(rz_engine *e, int32_t *d_ring, void *stream) {
    RZ_ENTER_PLAY(e);
    (void)stream;   // (nothing is enqueued: the ring is an argument of the launches to come)
    if (e->play_steps > 0 || e->play_drawn) return rz_fail(RZ_ERR_ARG, "rz_play_set_pruned_visits: a move step has been enqueued since rz_play_attach (attach again)");
    if (d_ring != nullptr && !(e->dev.forced_k > 0.0)) return rz_fail(RZ_ERR_ARG, "rz_play_set_pruned_visits: forced playouts are off (rz_set_forced_playouts first)");
    if (d_ring != nullptr && e->play.match_on) return rz_fail(RZ_ERR_ARG, "rz_play_set_pruned_visits: a match is on (rz_play_set_match): its games are not training data");
    // host memory (pinned, written directly like the log) must be addressable from this device
    if (d_ring != nullptr) RZ_TRY(rz_device_address(d_ring, e->cfg.device, "rz_play_set_pruned_visits", "d_ring"));
    e->play_pring = d_ring;
    return RZ_OK;
}

int rz_advance_roots(rz_engine *e, const int32_t *d_moves, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_moves);
    k_advance<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, d_moves);
    return rz_launched("k_advance");
}

int rz_step_games(rz_engine *e, const int32_t *d_moves, int32_t *d_winner, uint8_t *d_ended, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_moves);
    k_step_games<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, d_moves, d_winner, d_ended);
    return rz_launched("k_step_games");
}

// ------------------------------------------------------------------ the move step on the device
int rz_play_attach(rz_engine *e, const rz_play_config *cfg) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(cfg);
    if (e->dev.K != 1) return rz_fail(RZ_ERR_ARG, "rz_play_attach: one simulation in flight per tree only");
    if (!cfg->d_queue_ids || !cfg->d_queue_ctl || !cfg->d_log || cfg->ring_steps < 2) return rz_fail(RZ_ERR_ARG, "rz_play_attach: queue, log and a ring of >= 2 steps are needed");
    if (!(cfg->temperature > 0.0)) return rz_fail(RZ_ERR_ARG, "rz_play_attach: temperature must be positive");
    if (cfg->stall_margin < 0.0 || cfg->stall_margin >= 0.5) return rz_fail(RZ_ERR_ARG, "rz_play_attach: stall_margin not in [0, 0.5)");
    RZ_HIP(hipDeviceSynchronize());
    Play &Y = e->play;
    const long long G = e->cfg.n_games;
    if (!e->play_seen) {   // the first rz_play_attach of this engine: no array yet
        memset(&Y, 0, sizeof(Y));
        e->play_seen = true;
    }
    // Every array once per engine: an attach that ran out of memory is retried array by array -- what an earlier call got stays.
    if (Y.game_id == nullptr) RZ_TRY(e->pool.alloc(&Y.game_id, G));
    if (Y.ply == nullptr) RZ_TRY(e->pool.alloc(&Y.ply, G));
    if (Y.state == nullptr) RZ_TRY(e->pool.alloc(&Y.state, G));
    if (Y.mailbox == nullptr) RZ_TRY(e->pool.alloc(&Y.mailbox, G));
    if (Y.keep == nullptr) RZ_TRY(e->pool.alloc(&Y.keep, G));
    if (Y.stepm == nullptr) RZ_TRY(e->pool.alloc(&Y.stepm, G));
    if (Y.step_ab == nullptr) RZ_TRY(e->pool.alloc(&Y.step_ab, 2));
    if (Y.resign == nullptr) RZ_TRY(e->pool.alloc(&Y.resign, 2));
    if (Y.cap == nullptr) RZ_TRY(e->pool.alloc(&Y.cap, 2));
    if (Y.sims_of == nullptr) RZ_TRY(e->pool.alloc(&Y.sims_of, G));
    if (Y.order == nullptr) RZ_TRY(e->pool.alloc(&Y.order, G));
    if (Y.inv_t_of == nullptr) {
        double *tab = nullptr;
        RZ_TRY(e->pool.alloc(&tab, 2 * e->dev.S));
        Y.inv_t_of = tab;
    }
    if (Y.top_hwm == nullptr) RZ_TRY(e->pool.alloc(&Y.top_hwm, G));
    Y.queue_ids = cfg->d_queue_ids;
    Y.queue_ctl = cfg->d_queue_ctl;
    Y.log = cfg->d_log;
    // a log in HOST memory (pinned: the kernels write it directly) must be addressable from THIS device
    RZ_TRY(rz_device_address(Y.log, e->cfg.device, "rz_play_attach", "d_log"));
    Y.ring = cfg->ring_steps;
    Y.words = RZ_PLAY_RECORD_WORDS + e->dev.A;
    Y.seed = cfg->seed;
    Y.inv_t = 1.0 / cfg->temperature;
    Y.margin = ry::stall_margin(cfg->stall_margin, Y.inv_t);
    Y.resign_on = 0;   // (resignation is off after every attach: rz_play_set_resign)
    Y.cap_on = 0;      // (and so is the playout cap: rz_play_set_cap)
    Y.match_on = 0;    // (and match mode: rz_play_set_match)
    Y.queue_cap = 0;   // (and the queue of game ids is the linear one: rz_play_queue_ring)
    e->play_margin_cfg = cfg->stall_margin;
    Y.temp_on = 0;     // (and the temperature schedule: rz_play_set_temperatures)
    Y.n_full = e->cfg.n_playout;
    RZ_HIP(hipMemset(Y.step_ab, 0, 8));
    RZ_HIP(hipMemset(Y.ply, 0, (size_t)G * 4));
    RZ_HIP(hipMemset(Y.top_hwm, 0, (size_t)G * 4));
    k_play_stop<<<flat_grid(e), dim3(256), 0, 0>>>(e->dev, Y);
    RZ_HIP(hipDeviceSynchronize());
    e->play_on = true;
    e->play_drawn = false;
    e->play_steps = 0;
    e->play_vring = nullptr;   // (and the ring of root values: rz_play_set_root_values)
    e->play_pring = nullptr;   // (and the ring of pruned counts: rz_play_set_pruned_visits)
    return RZ_OK;
}

int rz_play_set_root_values(rz_engine *e, float *d_ring, void *stream) {
    RZ_ENTER_PLAY(e);
    (void)stream;   // (nothing is enqueued: the ring is an argument of the draws to come)
    // a move step enqueued -- or captured into a whole-move graph -- holds the ring it was launched with
    if (e->play_steps > 0 || e->play_drawn) return rz_fail(RZ_ERR_ARG, "rz_play_set_root_values: a move step has been enqueued since rz_play_attach (attach again)");
    if (d_ring != nullptr && e->play.match_on) return rz_fail(RZ_ERR_ARG, "rz_play_set_root_values: a match is on (rz_play_set_match): its games are not training data");
    // host memory (pinned, written directly like the log) must be addressable from this device
    if (d_ring != nullptr) RZ_TRY(rz_device_address(d_ring, e->cfg.device, "rz_play_set_root_values", "d_ring"));
    e->play_vring = d_ring;
    return RZ_OK;
}

int rz_play_queue_ring(rz_engine *e, int32_t capacity) {
    RZ_ENTER_PLAY(e);
    if (capacity < 0) return rz_fail(RZ_ERR_ARG, "rz_play_queue_ring: capacity %d is negative", capacity);
    // the capacity is a kernel argument of the move step: one enqueued -- or captured into a whole-move graph -- keeps the one it had
    if (e->play_steps > 0 || e->play_drawn) return rz_fail(RZ_ERR_ARG, "rz_play_queue_ring: a move step has been enqueued since rz_play_attach (attach again)");
    e->play.queue_cap = capacity;
    return RZ_OK;
}

int rz_play_queue_push(rz_engine *e, int64_t first_id, int32_t count, void *stream) {
    RZ_ENTER_PLAY(e);
    const int cap = e->play.queue_cap;
    if (cap <= 0) return rz_fail(RZ_ERR_ARG, "rz_play_queue_push: the queue is linear (call rz_play_queue_ring first)");
    if (first_id < 0) return rz_fail(RZ_ERR_ARG, "rz_play_queue_push: first id %lld is negative", (long long)first_id);
    if (count < 0 || count > cap) return rz_fail(RZ_ERR_ARG, "rz_play_queue_push: %d ids for a ring of %d", count, cap);
    if (count == 0) return RZ_OK;
    k_play_push<<<dim3(1), dim3(256), 0, as_stream(stream)>>>(e->dev, e->play, first_id, count);
    return rz_launched("k_play_push");
}

int rz_play_draw(rz_engine *e, void *stream) {
    RZ_ENTER_PLAY(e);
    // (rz_play_set_pruned_visits: the pruned counts of the roots the draw is about to read, into the row of the same step)
    if (e->play_pring != nullptr) k_root_pruned<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, e->play, e->play_pring, 1);
    k_play_draw<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, e->play, e->play_vring);
    e->play_drawn = true;
    return rz_launched("k_play_draw");
}

int rz_play_apply(rz_engine *e, void *stream) {
    RZ_ENTER_PLAY(e);
    const Play &Y = e->play;
    if (!e->play_drawn) k_play_no_draw<<<dim3(1), dim3(1), 0, as_stream(stream)>>>(Y);   // (the step counter k_play_draw would have handed on)
    k_play_apply<<<per_game(e), dim3(kWave), 0, as_stream(stream)>>>(e->dev, Y, e->play_drawn ? 1 : 0);
    // (rz_play_set_cap: the workgroup order of the coming search, from the budgets k_play_apply has just written)
    if (Y.cap_on && e->cap_ordered) k_play_order<<<dim3(1), dim3(256), 0, as_stream(stream)>>>(e->dev.active, Y.sims_of, Y.n_full, e->cfg.n_games, Y.order);
    e->play_drawn = false;
    e->play_steps += 1;
    return rz_launched("k_play_apply");
}

int rz_play_set_resign(rz_engine *e, double threshold, double disabled_frac, void *stream) {
    RZ_ENTER_PLAY(e);
    if (!(disabled_frac >= 0.0 && disabled_frac <= 1.0)) return rz_fail(RZ_ERR_ARG, "rz_play_set_resign: disabled_frac %g not in [0, 1]", disabled_frac);
    if (e->play.match_on) return rz_fail(RZ_ERR_ARG, "rz_play_set_resign: a match is on (rz_play_set_match): its games are played to the end");
    k_play_set_resign<<<dim3(1), dim3(1), 0, as_stream(stream)>>>(e->play.resign, threshold, disabled_frac);
    e->play.resign_on = 1;
    return rz_launched("k_play_set_resign");
}

int rz_play_set_temperatures(rz_engine *e, const double *h_temps, int32_t n, void *stream) {
    RZ_ENTER_PLAY(e);
    Play &Y = e->play;
    const int S = e->dev.S;
    if (n < 0 || n > S) return rz_fail(RZ_ERR_ARG, "rz_play_set_temperatures: %d entries for a board of %d cells (a game has no more plies)", n, S);
    if (n > 0 && h_temps == nullptr) return rz_fail(RZ_ERR_ARG, "rz_play_set_temperatures: NULL table");
    if (Y.match_on) return rz_fail(RZ_ERR_ARG, "rz_play_set_temperatures: a match is on (rz_play_set_match): its moves keep the temperature of rz_play_attach");
    for (int p = 0; p < n; ++p)
        if (!(std::isfinite(h_temps[p]) && h_temps[p] > 0.0))
            return rz_fail(RZ_ERR_ARG, "rz_play_set_temperatures: entry %d (%g) is not a finite positive temperature", p, h_temps[p]);
    // 1 / T on the host (the division of rz_play_attach), padded with the last entry; n == 0: the temperature of rz_play_attach.
    // Behind it each ply's stall margin by rz_play_attach's rule (rz_play.h: temp_entry).
    for (int base = 0; base < 2 * S; base += kTempChunk) {
        TempChunk c = {};
        for (int i = 0; i < kTempChunk && base + i < 2 * S; ++i) c.v[i] = ry::temp_entry(base + i, S, h_temps, n, Y.inv_t, e->play_margin_cfg);
        k_play_set_temps<<<dim3(1), dim3(kTempChunk), 0, as_stream(stream)>>>(const_cast<double *>(Y.inv_t_of), c, base, 2 * S);
    }
    Y.temp_on = 1;
    return rz_launched("k_play_set_temps");
}

static int playouts_route_ok(rz_engine *e, const char *what) {
    if (e->dev.K != 1 || e->dev.score_mode != RZ_SCORE_UCT_REF)
        return rz_fail(RZ_ERR_ARG, "%s: per-game simulation counts need the resident search (RZ_SCORE_UCT_REF, one simulation in flight per tree)", what);
    return RZ_OK;
}

int rz_play_set_cap(rz_engine *e, int32_t n_fast, double p_full, void *stream) {
    RZ_ENTER_PLAY(e);
    RZ_TRY(playouts_route_ok(e, "rz_play_set_cap"));
    if (e->play.match_on) return rz_fail(RZ_ERR_ARG, "rz_play_set_cap: a match is on (rz_play_set_match): every search of it has n_playout simulations");
    if (!std::isnan(p_full)) {
        if (!(p_full > 0.0 && p_full <= 1.0)) return rz_fail(RZ_ERR_ARG, "rz_play_set_cap: p_full %g not in (0, 1]", p_full);
        if (n_fast < 1 || n_fast > e->cfg.n_playout) return rz_fail(RZ_ERR_ARG, "rz_play_set_cap: n_fast %d not in 1 .. n_playout = %d", n_fast, e->cfg.n_playout);
    }
    const Play &Y = e->play;
    k_play_cap<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev, Y, (double)n_fast, p_full);
    k_play_order<<<dim3(1), dim3(256), 0, as_stream(stream)>>>(e->dev.active, Y.sims_of, Y.n_full, e->cfg.n_games, Y.order);
    e->play.cap_on = 1;
    return rz_launched("k_play_cap");
}

int rz_play_set_cap_order(rz_engine *e, int32_t longest_first) {
    if (e == nullptr) return rz_fail(RZ_ERR_ARG, "engine handle is NULL");
    e->cap_ordered = longest_first != 0;
    return RZ_OK;
}

int rz_set_playouts(rz_engine *e, const int32_t *d_counts, const int32_t *d_order, void *stream) {
    RZ_ENTER(eng_ready, e);
    if (d_counts == nullptr) {
        if (d_order != nullptr) return rz_fail(RZ_ERR_ARG, "rz_set_playouts: an order without counts");
        e->pl_on = e->pl_ordered = false;
        return RZ_OK;
    }
    RZ_TRY(playouts_route_ok(e, "rz_set_playouts"));
    const long long G = e->cfg.n_games;
    if (e->pl_counts == nullptr) RZ_TRY(e->pool.alloc(&e->pl_counts, G));
    if (e->pl_order == nullptr) RZ_TRY(e->pool.alloc(&e->pl_order, G));
    RZ_HIP(hipMemcpyAsync(e->pl_counts, d_counts, (size_t)G * 4, hipMemcpyDeviceToDevice, as_stream(stream)));
    if (d_order != nullptr) RZ_HIP(hipMemcpyAsync(e->pl_order, d_order, (size_t)G * 4, hipMemcpyDeviceToDevice, as_stream(stream)));
    e->pl_on = true;
    e->pl_ordered = d_order != nullptr;
    return RZ_OK;
}

int rz_playouts_view(rz_engine *e, const int32_t **d_counts, const int32_t **d_order) {
    RZ_ENTER(eng_ready, e);
    if (!d_counts || !d_order) return rz_fail(RZ_ERR_ARG, "NULL output pointer");
    *d_counts = *d_order = nullptr;
    if (e->pl_on) {   // the host's counts come before the device's rule
        *d_counts = e->pl_counts;
        *d_order = e->pl_ordered ? e->pl_order : nullptr;
    } else if (e->play_on && e->play.cap_on) {
        *d_counts = e->play.sims_of;
        *d_order = e->cap_ordered ? e->play.order : nullptr;
    }
    return RZ_OK;
}

int rz_playouts_read(rz_engine *e, int32_t *h_counts, int32_t *h_order, int32_t *h_source) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(h_source);
    const int32_t *dc = nullptr, *dor = nullptr;
    RZ_TRY(rz_playouts_view(e, &dc, &dor));
    RZ_HIP(hipDeviceSynchronize());
    const size_t G = (size_t)e->cfg.n_games;
    if (dc != nullptr && h_counts != nullptr) RZ_HIP(hipMemcpy(h_counts, dc, G * 4, hipMemcpyDeviceToHost));
    if (dor != nullptr && h_order != nullptr) RZ_HIP(hipMemcpy(h_order, dor, G * 4, hipMemcpyDeviceToHost));
    *h_source = dc == nullptr ? 0 : (e->pl_on ? 1 : 2) | (dor != nullptr ? 4 : 0);
    return RZ_OK;
}

int rz_play_set_match(rz_engine *e, const uint64_t *d_open_stones, const int32_t *d_open_to_move, const int32_t *d_open_last, int32_t n_openings,
                      void *stream) {
    RZ_ENTER_PLAY(e);
    Play &Y = e->play;
    if (n_openings == 0) {   // off again: the slots' flags as k_play_apply leaves them
        if (Y.match_on) k_play_side<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev, Y, -1);
        Y.match_on = 0;
        return rz_launched("k_play_side");
    }
    if (n_openings < 0 || !d_open_stones || !d_open_to_move || !d_open_last) return rz_fail(RZ_ERR_ARG, "rz_play_set_match: a table of n_openings >= 1 positions is needed");
    if (e->cfg.add_noise) return rz_fail(RZ_ERR_ARG, "rz_play_set_match: a match is played without Dirichlet noise (add_noise = 0)");
    if (e->dev.K != 1 || e->dev.score_mode != RZ_SCORE_UCT_REF)
        return rz_fail(RZ_ERR_ARG, "rz_play_set_match: matches need the resident search (RZ_SCORE_UCT_REF, one simulation in flight per tree)");
    if (Y.resign_on || Y.cap_on) return rz_fail(RZ_ERR_ARG, "rz_play_set_match: resignation or a playout cap is set (attach again: a match has neither)");
    if (Y.temp_on) return rz_fail(RZ_ERR_ARG, "rz_play_set_match: a temperature schedule is set (attach again: a match keeps the temperature of rz_play_attach)");
    if (e->play_vring != nullptr) return rz_fail(RZ_ERR_ARG, "rz_play_set_match: a ring of root values is set (rz_play_set_root_values; attach again: a match logs none)");
    if (n_openings > e->open_cap) {   // (hipFree waits for the device: no launch still reads the old table)
        const void *old[3] = {Y.open_stones, Y.open_to_move, Y.open_last};
        for (const void *p : old) {
            if (p == nullptr) continue;
            e->pool.ptrs.erase(std::remove(e->pool.ptrs.begin(), e->pool.ptrs.end(), const_cast<void *>(p)), e->pool.ptrs.end());
            RZ_HIP(hipFree(const_cast<void *>(p)));
        }
        Y.open_stones = nullptr, Y.open_to_move = Y.open_last = nullptr;
        e->open_cap = 0;
        uint64_t *st = nullptr;
        int32_t *tm = nullptr, *la = nullptr;
        RZ_TRY(e->pool.alloc(&st, (long long)n_openings * 2 * kWords));
        Y.open_stones = st;
        RZ_TRY(e->pool.alloc(&tm, n_openings));
        Y.open_to_move = tm;
        RZ_TRY(e->pool.alloc(&la, n_openings));
        Y.open_last = la;
        e->open_cap = n_openings;
    }
    RZ_HIP(hipMemcpyAsync(const_cast<uint64_t *>(Y.open_stones), d_open_stones, (size_t)n_openings * 2 * kWords * 8, hipMemcpyDeviceToDevice, as_stream(stream)));
    RZ_HIP(hipMemcpyAsync(const_cast<int32_t *>(Y.open_to_move), d_open_to_move, (size_t)n_openings * 4, hipMemcpyDeviceToDevice, as_stream(stream)));
    RZ_HIP(hipMemcpyAsync(const_cast<int32_t *>(Y.open_last), d_open_last, (size_t)n_openings * 4, hipMemcpyDeviceToDevice, as_stream(stream)));
    Y.n_open = n_openings;
    Y.match_on = 1;
    return RZ_OK;
}

int rz_play_side(rz_engine *e, int32_t side, void *stream) {
    RZ_ENTER(eng_ready, e);
    if (!e->play_on || !e->play.match_on) return rz_fail(RZ_ERR_ARG, "rz_play_side: call rz_play_set_match first");
    if (side != 0 && side != 1) return rz_fail(RZ_ERR_ARG, "rz_play_side: side %d is neither 0 (network A) nor 1 (network B)", side);
    k_play_side<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev, e->play, side);
    return rz_launched("k_play_side");
}

int rz_active_read(rz_engine *e, uint8_t *h_active) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(h_active);
    RZ_HIP(hipDeviceSynchronize());
    RZ_HIP(hipMemcpy(h_active, e->dev.active, (size_t)e->cfg.n_games, hipMemcpyDeviceToHost));
    return RZ_OK;
}

int rz_play_resolve(rz_engine *e, int32_t slot, int32_t move, void *stream) {
    RZ_ENTER_PLAY(e);
    if (slot < 0 || slot >= e->cfg.n_games || move < 0 || move >= e->dev.A) return rz_fail(RZ_ERR_ARG, "rz_play_resolve: slot %d / move %d out of range", slot, move);
    k_play_resolve<<<dim3(1), dim3(1), 0, as_stream(stream)>>>(e->play, slot, move);
    return rz_launched("k_play_resolve");
}

int rz_play_stop(rz_engine *e, void *stream) {
    RZ_ENTER_PLAY(e);
    k_play_stop<<<flat_grid(e), dim3(256), 0, as_stream(stream)>>>(e->dev, e->play);
    return rz_launched("k_play_stop");
}

int rz_play_state(rz_engine *e, int64_t *h_game_id, int32_t *h_ply, int32_t *h_state, int64_t *h_steps) {
    RZ_ENTER_PLAY(e);
    RZ_HIP(hipDeviceSynchronize());
    const size_t G = (size_t)e->cfg.n_games;
    if (h_game_id) RZ_HIP(hipMemcpy(h_game_id, e->play.game_id, G * 8, hipMemcpyDeviceToHost));
    if (h_ply) RZ_HIP(hipMemcpy(h_ply, e->play.ply, G * 4, hipMemcpyDeviceToHost));
    if (h_state) RZ_HIP(hipMemcpy(h_state, e->play.state, G * 4, hipMemcpyDeviceToHost));
    if (h_steps) {
        int32_t ab[2] = {0, 0};
        RZ_HIP(hipMemcpy(ab, e->play.step_ab, 8, hipMemcpyDeviceToHost));
        *h_steps = ab[0];
    }
    return RZ_OK;
}

int rz_get_stats(rz_engine *e, rz_stats *out) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(out);
    RZ_HIP(hipDeviceSynchronize());
    const size_t G = (size_t)e->cfg.n_games;
    std::vector<int32_t> err(G), top(G), nblk(G);
    int32_t any = 0, drops = 0;
    RZ_HIP(hipMemcpy(&any, e->dev.err_any, 4, hipMemcpyDeviceToHost));
    RZ_HIP(hipMemcpy(&drops, e->dev.reuse_drops, 4, hipMemcpyDeviceToHost));
    RZ_HIP(hipMemcpy(err.data(), e->dev.err, G * 4, hipMemcpyDeviceToHost));
    RZ_HIP(hipMemcpy(top.data(), e->dev.top, G * 4, hipMemcpyDeviceToHost));
    RZ_HIP(hipMemcpy(nblk.data(), e->dev.nblk, G * 4, hipMemcpyDeviceToHost));
    if (e->play_on) {   // device-driven moves: the arenas' tops at the END of the searches (now they hold the kept subtrees)
        std::vector<int32_t> hwm(G);
        RZ_HIP(hipMemcpy(hwm.data(), e->play.top_hwm, G * 4, hipMemcpyDeviceToHost));
        for (size_t g = 0; g < G; ++g)
            if (hwm[g] > top[g]) top[g] = hwm[g];
    }
    memset(out, 0, sizeof(*out));
    out->error_flags = any;
    out->first_bad_game = -1;
    for (size_t g = 0; g < G; ++g) {
        if ((err[g] & ~RZ_FLAG_REUSE_DROPPED) && out->first_bad_game < 0) out->first_bad_game = (int32_t)g;
        if (top[g] > out->max_slots_used) out->max_slots_used = top[g];
        if (nblk[g] > out->max_blocks_used) out->max_blocks_used = nblk[g];
    }
    out->arena_slots = e->dev.cap;
    out->prior_floats = e->dev.pcap;
    out->device_bytes = e->pool.bytes;
    out->n_select_calls = e->n_select;
    out->reuse_dropped = drops;
    return RZ_OK;
}

int rz_poll_errors(rz_engine *e, int32_t *h_flags, int32_t *h_reuse_dropped, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(h_flags);
    RZ_HIP(hipStreamSynchronize(as_stream(stream)));
    RZ_HIP(hipMemcpy(h_flags, e->dev.err_any, 4, hipMemcpyDeviceToHost));
    if (h_reuse_dropped) RZ_HIP(hipMemcpy(h_reuse_dropped, e->dev.reuse_drops, 4, hipMemcpyDeviceToHost));
    return RZ_OK;
}

int rz_clear_errors(rz_engine *e) {
    RZ_ENTER(eng_ready, e);
    RZ_HIP(hipDeviceSynchronize());
    RZ_HIP(hipMemset(e->dev.err, 0, (size_t)e->cfg.n_games * 4));
    RZ_HIP(hipMemset(e->dev.err_any, 0, 4));
    RZ_HIP(hipMemset(e->dev.reuse_drops, 0, 4));
    return RZ_OK;
}

int rz_copy_arena(rz_engine *e, int32_t game, int64_t max_slots, int32_t *h_n, double *h_w,
                  int32_t *h_first_child, int32_t *h_n_visited, int32_t *h_n_children,
                  int32_t *h_prior_block, float *h_root_prior, int32_t *h_top) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(h_top);
    if (game < 0 || game >= e->cfg.n_games) return rz_fail(RZ_ERR_ARG, "game %d out of range", game);
    RZ_HIP(hipDeviceSynchronize());
    int32_t arena = 0, top = 0;
    RZ_HIP(hipMemcpy(&arena, e->dev.cur_arena + game, 4, hipMemcpyDeviceToHost));
    RZ_HIP(hipMemcpy(&top, e->dev.top + game, 4, hipMemcpyDeviceToHost));
    *h_top = top;
    long long n = top < max_slots ? top : max_slots;
    if (n <= 0) return RZ_OK;
    const long long base = ((long long)game * 2 + arena) * e->dev.cap;
    std::vector<int4> rec((size_t)n * 2);
    RZ_HIP(hipMemcpy(rec.data(), e->dev.R + 2 * base, (size_t)n * 2 * sizeof(int4), hipMemcpyDeviceToHost));
    for (long long i = 0; i < n; ++i) {
        const int4 lo = rec[(size_t)(2 * i)], hi = rec[(size_t)(2 * i + 1)];
        if (h_n) h_n[i] = lo.x;
        if (h_first_child) h_first_child[i] = lo.y;
        if (h_n_visited) h_n_visited[i] = lo.z;
        if (h_n_children) h_n_children[i] = lo.w & 0xffff;
        if (h_prior_block) h_prior_block[i] = hi.z;
        if (h_w) memcpy(&h_w[i], &hi.x, 8);
    }
    if (h_root_prior) memcpy(h_root_prior, &rec[1].w, 4);
    return RZ_OK;
}

int rz_copy_priors(rz_engine *e, int32_t game, int64_t max_floats, float *h_priors, int32_t *h_count) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(h_count);
    if (game < 0 || game >= e->cfg.n_games) return rz_fail(RZ_ERR_ARG, "game %d out of range", game);
    RZ_HIP(hipDeviceSynchronize());
    int32_t arena = 0, ptop = 0;
    RZ_HIP(hipMemcpy(&arena, e->dev.cur_arena + game, 4, hipMemcpyDeviceToHost));
    RZ_HIP(hipMemcpy(&ptop, e->dev.ptop + game, 4, hipMemcpyDeviceToHost));
    *h_count = ptop;
    const long long n = ptop < max_floats ? ptop : max_floats;
    if (n <= 0 || h_priors == nullptr) return RZ_OK;
    RZ_HIP(hipMemcpy(h_priors, e->dev.P + ((long long)game * 2 + arena) * e->dev.pcap, (size_t)n * 4,
                     hipMemcpyDeviceToHost));
    return RZ_OK;
}

int rz_uct_scores(rz_engine *e, const double *d_w, const int32_t *d_n, const int32_t *d_np,
                  double c_puct, double *d_out, int64_t count, void *stream) {
    RZ_ENTER(eng_ready, e);
    RZ_NEED(d_w); RZ_NEED(d_n); RZ_NEED(d_np); RZ_NEED(d_out);
    if (count <= 0) return RZ_OK;
    const unsigned blocks = (unsigned)((count + 255) / 256);
    k_uct_scores<<<dim3(blocks), dim3(256), 0, as_stream(stream)>>>(d_w, d_n, d_np, c_puct, e->d_logtab,
                                                                    e->dev.logtab_n, d_out, count);
    return rz_launched("k_uct_scores");
}

}  // extern "C"
