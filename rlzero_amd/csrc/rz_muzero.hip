// rz_muzero.hip -- MI355X (gfx950) MuZero search tree: latent-state MCTS with pUCT selection and
// min-max value normalisation, for many independent games (environments) at once.
//
// The reference only names MuZero (README.md:3, rlzero/algorithms/rl_args.py:21-24): there is no
// implementation to follow, so the algorithm is the published one -- Schrittwieser et al., "Mastering
// Atari, Go, Chess and Shogi by Planning with a Learned Model" (arXiv:1911.08265v2), appendix
// pseudocode: run_mcts / select_child / ucb_score / expand_node / backpropagate / MinMaxStats --
// which the parity tests restate in CPython and compare against, statistic for statistic.
// Single-player form (to_play is constant, CartPole): no sign flip in the backup.
//
// Three routes, one tree arithmetic (mz_descend / mz_grow_backup and their LDS twins give the same bits):
//   * step by step (rz_mz_select / rz_mz_expand_backup, one THREAD per game): the learned model stays outside -- the
//     caller gathers the parents' hidden states, runs dynamics + prediction on the batch, stores the new hidden states
//     at the leaf slots and hands reward / policy / value back;
//   * rz_mz_search: all simulations of a move in ONE launch, the model evaluated inside the kernel (k_mz_search);
//   * rz_mz_play_env (rz_mz_play_cartpole is its CartPole form): whole MOVES in one launch -- initial inference, root noise, search,
//     action draw, environment step, episode history on the device (k_mz_search with its MOVES stages, instantiated per environment
//     trait of rz_mz_env.h: CartPole, Acrobot).
// Behind rz_mz_search, for any environment whose rules the library holds: rz_mz_env_move -- action draw,
// environment step, record, hand-over of finished episodes, a thread per environment -- with rz_mz_root_noise and rz_mz_env_step
// (rz_cartpole_step is its CartPole instantiation) beside it.
// The RULES of a move -- CartPole and Acrobot, splitmix64 and the keys built from it, the action draw, the layout of a record -- are
// plain C++ in rz_mz_env.h, tested on the CPU; the whole moves and the moves behind a search call the same functions, and share
// mz_root_gammas (the root noise's draws) and mz_claim_episode (the hand-over's counters and entry) of rz_muzero_noise.h.
// A MuZero tree is tiny (n_sims + 1 expanded nodes, A children each) and its walk is a short chain of dependent steps,
// so the parallelism is across the thousands of games.  Tree layout in HBM (per game g, node slot i, slot index
// g * cap + i): one 32-byte record per node: N int32, first_child int32 (-1 = not expanded; the A children of a node are
// the consecutive slots first_child .. first_child + A - 1), value_sum f64, prior f64, reward f32.
//
// Arithmetic: fp64, one rounding per operation (-ffp-contract=off), IEEE divide and sqrt; the
// log((N + c2 + 1) / c2) factor of pUCT comes from a table filled by the HOST libm (what CPython's
// math.log calls), so a tree is bit-identical to the CPython restatement.
//
// This file is the host side of ONE translation unit: the kernels lie in headers beside it, one per family, each of which compiles
// alone (tests/test_csrc_headers.py) and describes its kernels where they are defined.
//   rz_muzero_tree.h    no kernel: MzNode, MzDev, the walk and the backup every route calls (mz_descend, mz_grow_backup)
//   rz_muzero_step.h    the step-by-step kernels: k_mz_init, k_mz_select, k_mz_expand_backup
//   rz_muzero_noise.h   no kernel: what whole moves and the moves behind a search share (mz_gamma, mz_root_gammas, mz_claim_episode)
//   rz_muzero_hot.h     no kernel: the LDS twins of the walk and the backup (MzHot, mz_descend_hot, mz_grow_backup_hot)
//   rz_muzero_search.h  k_mz_search with MzModel, MzTrace, MzPlay and its LDS budget (mz_search_lds_bytes)
//   rz_muzero_roots.h   the root readers: k_mz_root_children, k_mz_root_stats
//   rz_muzero_moves.h   the moves behind a search: k_mz_env_step, k_mz_env_move (MzEnvPlay), k_mz_root_noise
// What the two loaders compute before they upload is plain C++ in rz_mz_pack.h, tested on the CPU (tests/test_mz_pack.py).
// Below: struct rz_muzero, the table of k_mz_search's instantiations, the launch helpers and every extern "C" entry point.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <new>
#include <vector>

#include "rlzero_hip.h"
#include "rz_host.h"
#include "rz_mz_env.h"
#include "rz_mz_pack.h"

#pragma clang fp contract(off)

// (this order is the order of the kernels in the code object; the template instantiations follow in the order the code below names them)
#include "rz_muzero_tree.h"
#include "rz_muzero_step.h"
#include "rz_muzero_noise.h"
#include "rz_muzero_hot.h"
#include "rz_muzero_search.h"
#include "rz_muzero_roots.h"
#include "rz_muzero_moves.h"

struct rz_muzero {
    rz_mz_config cfg;
    MzDev dev;
    DevPool pool;   // everything the handle owns on the device: the trees, the model, the representation
    MzModel model = {};          // rz_mz_load_model
    float *d_model = nullptr;    // one allocation behind the pointers above
    bool model_loaded = false, representation_loaded = false;
    int rep_obs_dim = 0;         // rz_mz_load_representation: the observation features of the loaded rep1
    bool f16_ok = false;   // rz_mz_load_model: finite weights and a finite bound on relu(dyn1): whole MOVES may run their layers on the f16 pipe
    float *d_rep = nullptr;      // rz_mz_load_representation
    int n_cus = 256;             // of cfg.device
    int games_per_wg = 0;        // rz_mz_set_search_shape: 0 = chosen from n_games and n_cus
    bool value_transform = false;   // rz_mz_set_value_transform: the launchers take the VT instantiations of k_mz_search
};

namespace {

inline dim3 mz_grid(const rz_muzero *e) { return dim3((unsigned)((e->cfg.n_games + 127) / 128)); }

// the instantiation of k_mz_search for a tree placement, a route, an environment and the value transform (MAXA: the kernel's default)
template <bool TREE_LDS, bool MOVES, typename Env, bool VT>
constexpr auto mz_search_kernel = k_mz_search<TREE_LDS, MOVES, Env, (MOVES ? Env::kActions : kMzMaxA), VT>;

// EVERY instantiation of k_mz_search the library has, once: mz_launch_search takes its kernel from these rows and rz_mz_load_model walks
// the same rows for the dynamic-LDS attribute, so what can be launched is what was prepared.  A row is a route -- the search alone
// (kMzNoEnv) or whole moves of an environment kind -- with or without the value transform, and holds its kernel for either placement of
// the trees.  A new environment is one line: its two rows.  (The rows stand in the order of the instantiations in the code object.)
typedef void (*MzSearchFn)(MzDev, MzModel, float *, int, int, MzTrace, MzPlay);
constexpr int kMzNoEnv = -1;
struct MzSearchRow {
    int kind;   // RZ_MZ_ENV_* of whole moves, kMzNoEnv for rz_mz_search
    bool vt;
    MzSearchFn tree_lds, tree_hbm;
};
template <bool MOVES, typename Env, bool VT>
constexpr MzSearchRow mz_search_row(int kind) {
    return {kind, VT, mz_search_kernel<true, MOVES, Env, VT>, mz_search_kernel<false, MOVES, Env, VT>};
}
constexpr MzSearchRow kMzSearchRows[] = {
    mz_search_row<false, rzmze::EnvCartPole, false>(kMzNoEnv), mz_search_row<true, rzmze::EnvCartPole, false>(RZ_MZ_ENV_CARTPOLE),
    mz_search_row<false, rzmze::EnvCartPole, true>(kMzNoEnv), mz_search_row<true, rzmze::EnvCartPole, true>(RZ_MZ_ENV_CARTPOLE),
    mz_search_row<true, rzmze::EnvAcrobot, true>(RZ_MZ_ENV_ACROBOT), mz_search_row<true, rzmze::EnvAcrobot, false>(RZ_MZ_ENV_ACROBOT),
};

int mz_ready(rz_muzero *e) {
    if (e == nullptr) return rz_fail(RZ_ERR_ARG, "muzero handle is NULL");
    return rz_on_device(e->cfg.device);
}

// What a launch of k_mz_search looks like for the engine's current shape: mz_launch_search launches exactly this, and
// rz_mz_search_plan reports it (the tests prove through it which instantiation they ran).  `whole_moves`: the MOVES
// instantiations (rz_mz_play_env); they share the LDS layout of the move-by-move search up to dyn1's action columns -- one per action
// past the second (mz_w1_cols) -- so the plan is the same at two actions and is the engine's action count's beyond.
struct MzPlan {
    int gpw;        // games per workgroup
    bool tree_lds;  // trees in LDS (k_mz_search<true, ...>) or in HBM (<false, ...>)
    int lds;        // dynamic LDS bytes of the launch
};
MzPlan mz_search_plan(const rz_muzero *e, bool whole_moves) {
    MzPlan p;
    const int w1c = mz_w1_cols(whole_moves, e->cfg.n_actions <= kMzMaxA ? e->cfg.n_actions : kMzMaxA);
    // games per workgroup: a search is a latency chain per game and two workgroups share a CU without slowing each
    // other, so the 16 columns of a tile are filled first (profiles/r02/muzero_search_shape.txt)
    p.gpw = e->games_per_wg > 0 ? e->games_per_wg : kMzMaxGpw;
    // the trees go to LDS when two workgroups still fit on a CU
    const MzDev &D = e->dev;
    p.tree_lds = mz_search_lds_bytes(p.gpw, D.cap, D.path_stride, D.n_sims, true, w1c) <= 80 * 1024;
    p.lds = mz_search_lds_bytes(p.gpw, D.cap, D.path_stride, D.n_sims, p.tree_lds, w1c);
    return p;
}

// play != nullptr: whole moves of the environment `kind` (checked by rz_mz_play_env)
int mz_launch_search(rz_muzero *e, float *d_hidden, int32_t n_sims, const MzTrace &T, const MzPlay *play, int kind, void *stream) {
    const MzPlan plan = mz_search_plan(e, play != nullptr);
    if (plan.lds > 160 * 1024) return rz_fail(RZ_ERR_ARG, "n_sims too large for the fused search (paths do not fit in LDS)");
    const int route = play != nullptr ? kind : kMzNoEnv;
    MzSearchFn fn = nullptr;
    for (const MzSearchRow &row : kMzSearchRows)
        if (row.kind == route && row.vt == e->value_transform) fn = plan.tree_lds ? row.tree_lds : row.tree_hbm;
    if (fn == nullptr) return rz_fail(RZ_ERR_ARG, "unknown environment kind %d", kind);
    const dim3 grid((unsigned)((e->cfg.n_games + plan.gpw - 1) / plan.gpw)), block(64 * kMzWaves);
    const MzPlay none = {};
    fn<<<grid, block, plan.lds, (hipStream_t)stream>>>(e->dev, e->model, d_hidden, n_sims, plan.gpw, T, play != nullptr ? *play : none);
    return rz_launched("k_mz_search");
}

template <typename Env>
int mz_env_step_launch(double *d_state, int64_t *d_steps, int64_t *d_episode, const int64_t *d_actions, int32_t n_envs, uint64_t seed,
                       int64_t max_episode_steps, float *d_obs, float *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, void *stream) {
    k_mz_env_step<Env><<<dim3((unsigned)((n_envs + 127) / 128)), dim3(128), 0, (hipStream_t)stream>>>(
        d_state, reinterpret_cast<long long *>(d_steps), reinterpret_cast<long long *>(d_episode), reinterpret_cast<const long long *>(d_actions),
        n_envs, seed, max_episode_steps, d_obs, d_reward, d_terminated, d_truncated);
    return rz_launched("k_mz_env_step");
}

template <typename Env>
int mz_env_move_launch(rz_muzero *e, const MzEnvPlay &p, void *stream) {
    static_assert(Env::kState <= RZ_MZE_MAX_STATE && Env::kObs <= RZ_MZE_MAX_OBS && Env::kActions <= RZ_MZE_MAX_ACTIONS, "environment limits");
    if (e->cfg.n_actions != Env::kActions) return rz_fail(RZ_ERR_ARG, "the tree has %d actions, the environment %d", e->cfg.n_actions, Env::kActions);
    k_mz_env_move<Env><<<mz_grid(e), dim3(128), 0, (hipStream_t)stream>>>(e->dev, p);
    return rz_launched("k_mz_env_move");
}

}  // namespace

extern "C" {

int rz_mz_create(const rz_mz_config *cfg, rz_muzero **out) {
    if (cfg == nullptr || out == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (cfg->abi_version != RZ_ABI_VERSION) return rz_fail(RZ_ERR_ARG, "rz_mz_config.abi_version does not match the library");
    if (cfg->n_games < 1 || cfg->n_actions < 1 || cfg->n_actions > 64 || cfg->n_sims < 1)
        return rz_fail(RZ_ERR_ARG, "n_games / n_actions (1..64) / n_sims out of range");
    if (!(cfg->discount > 0.0) || !(cfg->pb_c_base > 0.0)) return rz_fail(RZ_ERR_ARG, "discount and pb_c_base must be > 0");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || cfg->device < 0 || cfg->device >= n_dev)
        return rz_fail(RZ_ERR_ARG, "bad device ordinal");
    if (hipSetDevice(cfg->device) != hipSuccess) return rz_fail(RZ_ERR_HIP, "hipSetDevice failed");
    rz_muzero *e = new (std::nothrow) rz_muzero();
    if (!e) return rz_fail(RZ_ERR_OOM, "host allocation failed");
    e->cfg = *cfg;
    if (hipDeviceGetAttribute(&e->n_cus, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess || e->n_cus < 1) e->n_cus = 256;
    MzDev &D = e->dev;
    D.n_games = cfg->n_games;
    D.n_actions = cfg->n_actions;
    D.n_sims = cfg->n_sims;
    D.cap = 1 + cfg->n_actions * (cfg->n_sims + 1);  // root + one block of children per expansion
    D.path_stride = cfg->n_sims + 2;
    D.discount = cfg->discount;
    D.pb_c_init = cfg->pb_c_init;
    const long long G = cfg->n_games, slots = G * D.cap;
    int rc = RZ_OK;
    double *d_log = nullptr;
#define MZ_ALLOC(field, count) if (rc == RZ_OK) rc = e->pool.alloc(&D.field, (count))
    MZ_ALLOC(nodes, slots);
    MZ_ALLOC(top, G);
    MZ_ALLOC(depth, G);
    MZ_ALLOC(path, G * D.path_stride);
    MZ_ALLOC(vmin, G);
    MZ_ALLOC(vmax, G);
    MZ_ALLOC(err, 1);
#undef MZ_ALLOC
    if (rc == RZ_OK) rc = e->pool.alloc(&d_log, cfg->n_sims + 2);
    if (rc == RZ_OK) {
        std::vector<double> tab((size_t)cfg->n_sims + 2);
        for (int n = 0; n < cfg->n_sims + 2; ++n) tab[(size_t)n] = std::log(((double)n + cfg->pb_c_base + 1.0) / cfg->pb_c_base);
        if (hipMemcpy(d_log, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(D.err, 0, 4) != hipSuccess || hipMemset(D.nodes, 0xff, (size_t)slots * sizeof(MzNode)) != hipSuccess ||
            hipMemset(D.top, 0, (size_t)G * 4) != hipSuccess || hipMemset(D.depth, 0, (size_t)G * 4) != hipSuccess)
            rc = rz_fail(RZ_ERR_HIP, "initialisation of the muzero tree failed");
    }
    if (rc != RZ_OK) {
        rz_mz_destroy(e);
        return rc;
    }
    D.pb_log = d_log;
    *out = e;
    return RZ_OK;
}

int rz_mz_destroy(rz_muzero *e) {
    if (e == nullptr) return RZ_OK;
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
    delete e;   // (the pool frees)
    return RZ_OK;
}

int rz_mz_upload_log_table(rz_muzero *e, const double *h_table, int64_t count) {
    RZ_ENTER(mz_ready, e);
    if (h_table == nullptr || count != e->cfg.n_sims + 2) return rz_fail(RZ_ERR_ARG, "table must hold n_sims + 2 entries");
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(const_cast<double *>(e->dev.pb_log), h_table, (size_t)count * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "hipMemcpy(log table) failed");
    return RZ_OK;
}

int rz_mz_init_roots(rz_muzero *e, const float *d_probs, const double *d_noise, double noise_frac, const uint8_t *d_mask,
                     void *stream) {
    RZ_ENTER(mz_ready, e);
    if (d_probs == nullptr) return rz_fail(RZ_ERR_ARG, "d_probs is NULL");
    k_mz_init<<<mz_grid(e), dim3(128), 0, (hipStream_t)stream>>>(e->dev, d_probs, d_noise, noise_frac, d_mask);
    return rz_launched("k_mz_init");
}

int rz_mz_select(rz_muzero *e, int32_t *d_parent, int32_t *d_action, int32_t *d_leaf, const uint8_t *d_mask, void *stream) {
    RZ_ENTER(mz_ready, e);
    if (!d_parent || !d_action || !d_leaf) return rz_fail(RZ_ERR_ARG, "NULL output pointer");
    k_mz_select<<<mz_grid(e), dim3(128), 0, (hipStream_t)stream>>>(e->dev, d_parent, d_action, d_leaf, d_mask);
    return rz_launched("k_mz_select");
}

int rz_mz_expand_backup(rz_muzero *e, const float *d_reward, const float *d_probs, const float *d_value,
                        const uint8_t *d_mask, void *stream) {
    RZ_ENTER(mz_ready, e);
    if (!d_reward || !d_probs || !d_value) return rz_fail(RZ_ERR_ARG, "NULL input pointer");
    k_mz_expand_backup<<<mz_grid(e), dim3(128), 0, (hipStream_t)stream>>>(e->dev, d_reward, d_probs, d_value, d_mask);
    return rz_launched("k_mz_expand_backup");
}

int rz_mz_root_children(rz_muzero *e, int32_t what, void *d_out, void *stream) {
    RZ_ENTER(mz_ready, e);
    if (d_out == nullptr || what < 0 || what > 3) return rz_fail(RZ_ERR_ARG, "bad argument");
    k_mz_root_children<<<mz_grid(e), dim3(128), 0, (hipStream_t)stream>>>(e->dev, what, d_out);
    return rz_launched("k_mz_root_children");
}

int rz_mz_root_stats(rz_muzero *e, int32_t *d_n, double *d_value_sum, double *d_vmin, double *d_vmax, void *stream) {
    RZ_ENTER(mz_ready, e);
    k_mz_root_stats<<<mz_grid(e), dim3(128), 0, (hipStream_t)stream>>>(e->dev, d_n, d_value_sum, d_vmin, d_vmax);
    return rz_launched("k_mz_root_stats");
}

int rz_mz_load_model(rz_muzero *e, const float *const *h_params, int32_t n_params, int32_t hidden) {
    RZ_ENTER(mz_ready, e);
    if (h_params == nullptr || n_params != 14) return rz_fail(RZ_ERR_ARG, "expected the 14 tensors of the dynamics / reward / prediction layers");
    if (hidden != kMzH) return rz_fail(RZ_ERR_ARG, "the fused search is built for hidden size 64");
    const int A = e->cfg.n_actions;
    if (A > kMzMaxA) return rz_fail(RZ_ERR_ARG, "the fused search handles up to 8 actions");
    for (int i = 0; i < 14; ++i)
        if (!h_params[i]) return rz_fail(RZ_ERR_ARG, "a parameter pointer is NULL");
    const rzmp::Model packed = rzmp::pack_model(h_params, A);   // layouts, scales and the f16 verdict: rz_mz_pack.h
    const size_t *off = packed.off, off_scales = packed.off_scales, total = packed.host.size();
    e->f16_ok = packed.f16_ok;
    RZ_HIP(hipDeviceSynchronize());
    if (e->d_model == nullptr) {
        RZ_TRY(e->pool.alloc(&e->d_model, (long long)total));
        const int most = 160 * 1024;
        for (const MzSearchRow &row : kMzSearchRows)
            for (MzSearchFn fn : {row.tree_lds, row.tree_hbm})
                if (hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess)
                    return rz_fail(RZ_ERR_HIP, "hipFuncSetAttribute(dynamic LDS) failed");
    }
    if (hipMemcpy(e->d_model, packed.host.data(), total * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "hipMemcpy(model) failed");
    const float *b = e->d_model;
    const MzModel seen = e->model;   // (the representation layers are loaded by their own call)
    e->model = MzModel{b + off[0], b + off[1], b + off[2], b + off[3], b + off[4], b + off[5], b + off[6], b + off[7],
                       b + off[8], b + off[9], b + off[10], b + off[11], b + off[12], b + off[13],
                       seen.rep1_w, seen.rep1_b, seen.rep2_w, seen.rep2_b, b + off_scales};
    e->model_loaded = true;
    return RZ_OK;
}

int rz_mz_load_representation(rz_muzero *e, const float *const *h_params, int32_t n_params, int32_t obs_dim, int32_t hidden) {
    RZ_ENTER(mz_ready, e);
    if (h_params == nullptr || n_params != 4) return rz_fail(RZ_ERR_ARG, "expected rep1.weight, rep1.bias, rep2.weight, rep2.bias");
    if (hidden != kMzH || obs_dim < 1 || obs_dim > kMzObs) return rz_fail(RZ_ERR_ARG, "the fused moves are built for hidden size 64 and <= 8 observation features");
    for (int i = 0; i < 4; ++i)
        if (!h_params[i]) return rz_fail(RZ_ERR_ARG, "a parameter pointer is NULL");
    // rep1.w [64][obs_dim] -> k-major [8][64] (rows >= obs_dim zero), rep1.b, rep2.w [64][64] -> k-major, rep2.b: rz_mz_pack.h
    const rzmp::Representation packed = rzmp::pack_representation(h_params, obs_dim);
    const size_t *off = packed.off, total = packed.host.size();
    RZ_HIP(hipDeviceSynchronize());
    if (e->d_rep == nullptr) RZ_TRY(e->pool.alloc(&e->d_rep, (long long)total));
    if (hipMemcpy(e->d_rep, packed.host.data(), total * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "hipMemcpy(representation) failed");
    e->model.rep1_w = e->d_rep + off[0];
    e->model.rep1_b = e->d_rep + off[1];
    e->model.rep2_w = e->d_rep + off[2];
    e->model.rep2_b = e->d_rep + off[3];
    e->representation_loaded = true;
    e->rep_obs_dim = obs_dim;
    return RZ_OK;
}

int rz_mz_search(rz_muzero *e, float *d_hidden, int32_t n_sims, int32_t *d_trace_parent, int32_t *d_trace_action,
                 int32_t *d_trace_leaf, float *d_trace_reward, float *d_trace_probs, float *d_trace_value, void *stream) {
    RZ_ENTER(mz_ready, e);
    if (!e->model_loaded) return rz_fail(RZ_ERR_ARG, "rz_mz_load_model has not been called");
    if (d_hidden == nullptr || n_sims < 1 || n_sims > e->cfg.n_sims) return rz_fail(RZ_ERR_ARG, "d_hidden is NULL or n_sims out of range");
    const bool any = d_trace_parent || d_trace_action || d_trace_leaf || d_trace_reward || d_trace_probs || d_trace_value;
    const bool all = d_trace_parent && d_trace_action && d_trace_leaf && d_trace_reward && d_trace_probs && d_trace_value;
    if (any && !all) return rz_fail(RZ_ERR_ARG, "the trace arrays come all together or not at all");
    const MzTrace T = {d_trace_parent, d_trace_action, d_trace_leaf, d_trace_reward, d_trace_probs, d_trace_value};
    return mz_launch_search(e, d_hidden, n_sims, T, nullptr, 0, stream);
}

// whole moves of the environment `kind`: the checks and the launch behind rz_mz_play_env and rz_mz_play_cartpole
static int mz_play_launch(rz_muzero *e, int32_t kind, float *d_hidden, int32_t n_sims, int32_t n_moves, const rz_mz_whole_play *play, void *stream) {
    RZ_ENTER(mz_ready, e);
    int env_actions = 0, env_obs = 0;
    if (kind == RZ_MZ_ENV_CARTPOLE) {
        env_actions = rzmze::EnvCartPole::kActions;
        env_obs = rzmze::EnvCartPole::kObs;
    } else if (kind == RZ_MZ_ENV_ACROBOT) {
        env_actions = rzmze::EnvAcrobot::kActions;
        env_obs = rzmze::EnvAcrobot::kObs;
    } else {
        return rz_fail(RZ_ERR_ARG, "unknown environment kind %d", kind);
    }
    if (!e->model_loaded || !e->representation_loaded) return rz_fail(RZ_ERR_ARG, "rz_mz_load_model and rz_mz_load_representation first");
    if (e->cfg.n_actions != env_actions) {
        if (kind == RZ_MZ_ENV_CARTPOLE) return rz_fail(RZ_ERR_ARG, "CartPole has 2 actions");
        return rz_fail(RZ_ERR_ARG, "the tree has %d actions, the environment %d", e->cfg.n_actions, env_actions);
    }
    if (e->rep_obs_dim != env_obs)
        return rz_fail(RZ_ERR_ARG, "the loaded representation takes obs_dim %d observations, the environment gives %d", e->rep_obs_dim, env_obs);
    if (!e->f16_ok)
        return rz_fail(RZ_ERR_ARG, "the model has non-finite weights: whole moves run their layers on the f16 matrix pipe and need finite "
                                   "bounds (use the move-by-move search, rz_mz_search / fused_moves=False)");
    if (d_hidden == nullptr || play == nullptr || n_sims < 1 || n_sims > e->cfg.n_sims || n_moves < 1)
        return rz_fail(RZ_ERR_ARG, "NULL pointer or n_sims / n_moves out of range");
    if (!play->d_state || !play->d_steps || !play->d_episode || !play->d_episode_start || !play->d_ring || !play->d_arena ||
        !play->d_counters || !play->d_entries)
        return rz_fail(RZ_ERR_ARG, "NULL environment / history pointer");
    if (play->max_episode_steps < 1) return rz_fail(RZ_ERR_ARG, "max_episode_steps must be >= 1");
    if (play->ring_steps < play->max_episode_steps + n_moves || play->arena_rows < 1 || play->max_entries < (int64_t)e->cfg.n_games * n_moves || play->first_step < 0)
        return rz_fail(RZ_ERR_ARG, "ring_steps must cover an episode (%lld steps) + the launch, max_entries one entry per environment and move",
                       (long long)play->max_episode_steps);
    if (!(play->dirichlet_alpha > 0.0) || play->noise_frac < 0.0 || play->noise_frac > 1.0) return rz_fail(RZ_ERR_ARG, "dirichlet_alpha must be > 0, noise_frac in [0, 1]");
    // mz_gamma floors a draw at 1e-30: P(Gamma(alpha, 1) < 1e-30) is 1.05e-3 at alpha 0.1 and 0.128 at 0.03, and a move whose draws are
    // ALL floored gets uniform noise where Dirichlet(alpha) is almost one-hot (tests/test_noise_streams_host.py states the figures)
    if (play->dirichlet_alpha < 0.1)
        return rz_fail(RZ_ERR_ARG, "dirichlet_alpha must be >= 0.1: below it the root noise's float32 draws reach their 1e-30 floor too often");
    MzPlay p = {};
    p.n_moves = n_moves;
    p.row = rzmze::record_layout(env_obs, env_actions).row;
    p.state = play->d_state;
    p.steps = reinterpret_cast<long long *>(play->d_steps);
    p.episode = reinterpret_cast<long long *>(play->d_episode);
    p.env_seed = play->env_seed;
    p.noise_seed = play->noise_seed;
    p.noise_frac = play->noise_frac;
    p.inv_temperature = play->temperature > 0.0 ? 1.0 / play->temperature : 0.0;
    p.alpha = (float)play->dirichlet_alpha;
    p.ring = play->d_ring;
    p.hist = play->ring_steps;
    p.t0 = play->first_step;
    p.ep_start = reinterpret_cast<long long *>(play->d_episode_start);
    p.arena = play->d_arena;
    p.arena_rows = play->arena_rows;
    p.counters = reinterpret_cast<long long *>(play->d_counters);
    p.entries = reinterpret_cast<long long *>(play->d_entries);
    p.max_entries = play->max_entries;
    p.max_episode_steps = play->max_episode_steps;
    const MzTrace T = {};
    return mz_launch_search(e, d_hidden, n_sims, T, &p, kind, stream);
}

int rz_mz_play_env(rz_muzero *e, int32_t kind, float *d_hidden, int32_t n_sims, int32_t n_moves, const rz_mz_whole_play *play, void *stream) {
    return mz_play_launch(e, kind, d_hidden, n_sims, n_moves, play, stream);
}

// CartPole-v1 through the same launcher: its play record + the limit of 500 steps
int rz_mz_play_cartpole(rz_muzero *e, float *d_hidden, int32_t n_sims, int32_t n_moves, const rz_mz_cartpole_play *play, void *stream) {
    if (play == nullptr) return mz_play_launch(e, RZ_MZ_ENV_CARTPOLE, d_hidden, n_sims, n_moves, nullptr, stream);
    rz_mz_whole_play p = {};
    p.d_state = play->d_state;
    p.d_steps = play->d_steps;
    p.d_episode = play->d_episode;
    p.d_episode_start = play->d_episode_start;
    p.env_seed = play->env_seed;
    p.noise_seed = play->noise_seed;
    p.noise_frac = play->noise_frac;
    p.dirichlet_alpha = play->dirichlet_alpha;
    p.temperature = play->temperature;
    p.d_ring = play->d_ring;
    p.ring_steps = play->ring_steps;
    p.first_step = play->first_step;
    p.d_arena = play->d_arena;
    p.arena_rows = play->arena_rows;
    p.d_counters = play->d_counters;
    p.d_entries = play->d_entries;
    p.max_entries = play->max_entries;
    p.max_episode_steps = 500;
    return mz_play_launch(e, RZ_MZ_ENV_CARTPOLE, d_hidden, n_sims, n_moves, &p, stream);
}

int rz_mz_set_value_transform(rz_muzero *e, int32_t on) {
    if (e == nullptr) return rz_fail(RZ_ERR_ARG, "muzero handle is NULL");
    if (on != 0 && on != 1) return rz_fail(RZ_ERR_ARG, "value transform: 0 (off) or 1 (on)");
    e->value_transform = on != 0;
    return RZ_OK;
}

int rz_mz_set_search_shape(rz_muzero *e, int32_t games_per_workgroup) {
    if (e == nullptr) return rz_fail(RZ_ERR_ARG, "muzero handle is NULL");
    if (games_per_workgroup < 0 || games_per_workgroup > kMzMaxGpw) return rz_fail(RZ_ERR_ARG, "games_per_workgroup must be 0 (auto) .. 16");
    e->games_per_wg = games_per_workgroup;
    return RZ_OK;
}

#ifdef RZ_MZ_PROFILE
int rz_mz_debug_profile(long long *h_out16) {
    return hipDeviceSynchronize() == hipSuccess && hipMemcpyFromSymbol(h_out16, HIP_SYMBOL(mz_prof), 16 * sizeof(long long)) == hipSuccess ? RZ_OK : RZ_ERR_HIP;
}
#endif

int rz_mz_search_plan(rz_muzero *e, int32_t whole_moves, int32_t *games_per_workgroup, int32_t *tree_in_lds, int32_t *lds_bytes) {
    if (e == nullptr) return rz_fail(RZ_ERR_ARG, "muzero handle is NULL");
    const MzPlan plan = mz_search_plan(e, whole_moves != 0);
    if (games_per_workgroup) *games_per_workgroup = plan.gpw;
    if (tree_in_lds) *tree_in_lds = plan.tree_lds ? 1 : 0;
    if (lds_bytes) *lds_bytes = plan.lds;
    return RZ_OK;
}

int rz_mz_tree_nodes(rz_muzero *e, void *h_nodes, int32_t *h_top) {
    RZ_ENTER(mz_ready, e);
    if (h_nodes == nullptr || h_top == nullptr) return rz_fail(RZ_ERR_ARG, "h_nodes / h_top is NULL");
    static_assert(sizeof(MzNode) == sizeof(rz_mz_node), "rz_mz_node is the device's node record");
    const size_t G = (size_t)e->cfg.n_games;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(h_nodes, e->dev.nodes, G * (size_t)e->dev.cap * sizeof(MzNode), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(h_top, e->dev.top, G * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "hipMemcpy(tree nodes) failed");
    return RZ_OK;
}

int rz_mz_geometry(rz_muzero *e, int32_t *slots_per_game, int64_t *device_bytes) {
    if (e == nullptr) return rz_fail(RZ_ERR_ARG, "muzero handle is NULL");
    if (slots_per_game) *slots_per_game = e->dev.cap;
    if (device_bytes) *device_bytes = e->pool.bytes;
    return RZ_OK;
}

int rz_mz_error_flags(rz_muzero *e, int32_t *flags) {
    RZ_ENTER(mz_ready, e);
    if (flags == nullptr) return rz_fail(RZ_ERR_ARG, "flags is NULL");
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(flags, e->dev.err, 4, hipMemcpyDeviceToHost) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "hipMemcpy(err) failed");
    return RZ_OK;
}

// ---- moves kept on the device behind rz_mz_search, generic over the environment (rz_muzero_moves.h)

int rz_mz_env_step(int32_t kind, double *d_state, int64_t *d_steps, int64_t *d_episode, const int64_t *d_actions, int32_t n_envs, uint64_t seed,
                   int64_t max_episode_steps, float *d_obs, float *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, void *stream) {
    if (!d_state || !d_steps || !d_episode || !d_obs || n_envs < 1) return rz_fail(RZ_ERR_ARG, "NULL pointer or n_envs < 1");
    if (d_actions != nullptr && (!d_reward || !d_terminated || !d_truncated)) return rz_fail(RZ_ERR_ARG, "a step needs d_reward, d_terminated and d_truncated");
    if (max_episode_steps < 1) return rz_fail(RZ_ERR_ARG, "max_episode_steps must be >= 1");
    if (kind == RZ_MZ_ENV_CARTPOLE)
        return mz_env_step_launch<rzmze::EnvCartPole>(d_state, d_steps, d_episode, d_actions, n_envs, seed, max_episode_steps, d_obs, d_reward, d_terminated, d_truncated, stream);
    if (kind == RZ_MZ_ENV_ACROBOT)
        return mz_env_step_launch<rzmze::EnvAcrobot>(d_state, d_steps, d_episode, d_actions, n_envs, seed, max_episode_steps, d_obs, d_reward, d_terminated, d_truncated, stream);
    return rz_fail(RZ_ERR_ARG, "unknown environment kind %d", kind);
}

int rz_cartpole_step(double *d_state, int64_t *d_steps, int64_t *d_episode, const int64_t *d_actions, int32_t n_envs, uint64_t seed,
                     float *d_obs, float *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, void *stream) {
    if (!d_state || !d_steps || !d_episode || !d_actions || !d_obs || !d_reward || !d_terminated || !d_truncated || n_envs < 1)
        return rz_fail(RZ_ERR_ARG, "NULL pointer or n_envs < 1");
    return mz_env_step_launch<rzmze::EnvCartPole>(d_state, d_steps, d_episode, d_actions, n_envs, seed, 500, d_obs, d_reward, d_terminated, d_truncated, stream);
}

int rz_mz_env_move(rz_muzero *e, int32_t kind, const rz_mz_env_play *play, void *stream) {
    RZ_ENTER(mz_ready, e);
    if (play == nullptr) return rz_fail(RZ_ERR_ARG, "play is NULL");
    if (!play->d_state || !play->d_steps || !play->d_episode || !play->d_episode_start || !play->d_ring || !play->d_arena || !play->d_counters ||
        !play->d_entries || !play->d_obs)
        return rz_fail(RZ_ERR_ARG, "NULL environment / history pointer");
    if (play->max_episode_steps < 1 || play->ring_steps < play->max_episode_steps || play->arena_rows < 1 || play->max_entries < (int64_t)e->cfg.n_games ||
        play->step < 0)
        return rz_fail(RZ_ERR_ARG, "ring_steps must cover an episode (max_episode_steps), max_entries one entry per environment, step >= 0");
    MzEnvPlay p = {};
    p.state = play->d_state;
    p.steps = reinterpret_cast<long long *>(play->d_steps);
    p.episode = reinterpret_cast<long long *>(play->d_episode);
    p.ep_start = reinterpret_cast<long long *>(play->d_episode_start);
    p.env_seed = play->env_seed;
    p.noise_seed = play->noise_seed;
    p.inv_temperature = play->temperature > 0.0 ? 1.0 / play->temperature : 0.0;
    p.max_episode_steps = play->max_episode_steps;
    p.ring = play->d_ring;
    p.hist = play->ring_steps;
    p.t = play->step;
    p.arena = play->d_arena;
    p.arena_rows = play->arena_rows;
    p.counters = reinterpret_cast<long long *>(play->d_counters);
    p.entries = reinterpret_cast<long long *>(play->d_entries);
    p.max_entries = play->max_entries;
    p.obs = play->d_obs;
    if (kind == RZ_MZ_ENV_CARTPOLE) return mz_env_move_launch<rzmze::EnvCartPole>(e, p, stream);
    if (kind == RZ_MZ_ENV_ACROBOT) return mz_env_move_launch<rzmze::EnvAcrobot>(e, p, stream);
    return rz_fail(RZ_ERR_ARG, "unknown environment kind %d", kind);
}

int rz_mz_root_noise(rz_muzero *e, const int64_t *d_episode, const int64_t *d_steps, uint64_t noise_seed, double dirichlet_alpha, double *d_eta,
                     void *stream) {
    RZ_ENTER(mz_ready, e);
    if (!d_episode || !d_steps || !d_eta) return rz_fail(RZ_ERR_ARG, "NULL pointer");
    if (e->cfg.n_actions > kMzMaxA) return rz_fail(RZ_ERR_ARG, "the root noise serves at most 8 actions");
    // (the floor of mz_gamma: see rz_mz_play_cartpole)
    if (!(dirichlet_alpha >= 0.1))
        return rz_fail(RZ_ERR_ARG, "dirichlet_alpha must be >= 0.1: below it the root noise's float32 draws reach their 1e-30 floor too often");
    k_mz_root_noise<<<mz_grid(e), dim3(128), 0, (hipStream_t)stream>>>(e->cfg.n_games, e->cfg.n_actions, reinterpret_cast<const long long *>(d_episode),
                                                                        reinterpret_cast<const long long *>(d_steps), noise_seed, (float)dirichlet_alpha,
                                                                        d_eta);
    return rz_launched("k_mz_root_noise");
}

}  // extern "C"
