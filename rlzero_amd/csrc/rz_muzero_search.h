// rz_muzero_search.h -- the whole search in ONE launch: k_mz_search of rz_muzero.hip, with the records it takes (MzModel, MzTrace,
// MzPlay), its LDS budget (mz_search_lds_bytes, which the host's plan calls too), its matrix-pipe and lane helpers and the
// out-of-line environment calls of its whole moves.  The walk and the backup are rz_muzero_tree.h's, on LDS trees rz_muzero_hot.h's.
//
// k_mz_search: every simulation of every game's search -- select, gather of the parent's hidden state, recurrent
// inference (dynamics + reward head + prediction of rlzero_amd/muzero/network.py, hidden size 64), scatter of the new
// hidden state, expand + backup -- inside one kernel: no launch, no global synchronisation and no weight traffic
// between simulations (the step-by-step route replays a hipGraph of ~15 small launches per simulation).
// A search is a chain of short dependent steps per game, so the kernel is built for LATENCY and for filling the chip
// with few games: a workgroup of 4 waves owns `gpw` <= 16 games (4096 games -> 256 workgroups, one per CU).
//   * the layers are 64 x K GEMMs over the workgroup's games on the matrix pipe, v_mfma_f32_16x16x4_f32 (exact f32
//     products, f32 accumulation): games = the 16 columns, wave w owns output units 16w .. 16w+15.  The WEIGHTS are
//     the A operands and never change: each wave keeps its fragments of all layers in registers for the whole launch;
//     activations go [k][game] through LDS (B operand: one conflict-free ds_read_b32 per MFMA);
//   * dyn2 and rew1 read the same activations: one pass over k feeds both; the per-sample min-max scaling of the new
//     state reduces over the rows with two cross-row steps inside a wave and over the 4 waves through LDS; the scalar
//     heads (reward; policy logits, value) are dot products of the rows a lane already holds: partial sums per wave,
//     summed in wave order by the lane that owns the game;
//   * wave 0 walks and updates the trees, one lane per game, with the code of k_mz_select / k_mz_expand_backup
//     (mz_descend / mz_grow_backup): fp64, the host's log table -- the tree arithmetic is the step-by-step route's,
//     bit for bit, given the same network outputs (the outputs differ from rocBLAS' in the last bits: another
//     summation order).  TREE_LDS: the trees (32 B x slots per game), the paths and the log table live in LDS for the
//     search (a level of the walk costs an LDS round trip instead of an L2 one) and are written back at the end;
//   * MOVES (rz_mz_play_env): whole MOVES of the environments in the launch -- per move the initial inference
//     (representation + prediction on the same tiles), root expansion with Dirichlet noise, the n_sims simulations,
//     the action drawn from the visit counts, one packed record for the host and the environment step: the host's
//     part of self-play shrinks to reading the records.  The stages are generic over the environment trait `Env` of rz_mz_env.h
//     (EnvCartPole: 2 actions, 4 observations; EnvAcrobot: 3 actions, 6 observations): the action count of the unrolled loops, of the
//     walk and of dyn1's one-hot columns is Env::kActions, the LDS record of an environment is Env::kState doubles + steps, episode,
//     episode start (<= 8), Env::observe fills Env::kObs rows of OBS (the rest stay zero, as rep1_w's rows past obs_dim), the record is
//     record_layout(Env::kObs, Env::kActions) with the reward Env::step returns, the time limit comes from MzPlay.  Every rule is
//     called from the header, none restated.  Acrobot's step and observation (RK4 and double sin / cos: 230 registers) are CALLS
//     (mz_env_step_far): inlined they spilled inside the simulation loop; as calls the simulation loop touches no scratch and the
//     save / reload of the f16 fragments sits once per move (profiles/mz_whole_env/kernel_resources.txt).
//   * ROOTS (rz_mz_search_obs): the search alone from raw observations -- representation, root prediction, softmax and the roots
//     (k_mz_init's rule, rz_mz_roots.h) as a stage in front of simulation 0, on an observation tile and a staged first layer of its own
//     in LDS (MzRoots, below): a Reanalyse chunk is one launch between `positions` and the read-out.  With GUMBEL
//     (rz_mz_search_obs_gumbel; scalar heads or CAT) the stage also writes log(prior) and the root's v_hat, and the Gumbel preamble's own
//     prediction of the roots does not run: a Gumbel device move of self-play is this launch and k_mz_env_move.
//   * TREE_LDS trees use their own record: MzHot (N, first_child, value_sum, prior and q = reward + discount * value(),
//     refreshed by the backup that changes it, so the walk does not divide value_sum / N again at every visit) plus one
//     float of reward per node; sqrt(N) of the walk comes from a table filled with the same IEEE sqrt.  Same operations on
//     the same operands as mz_descend / mz_grow_backup: same bits (tests: fused search == step-by-step == CPython).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "rlzero_hip.h"
#include "rz_muzero_hot.h"
#include "rz_muzero_noise.h"
#include "rz_muzero_tree.h"
#include "rz_mz_env.h"
#include "rz_mz_gumbel.h"
#include "rz_mz_pack.h"
#include "rz_mz_roots.h"
#include "rz_mz_support.h"
#include "rz_mz_value.h"

#pragma clang fp contract(off)

namespace {

using rzmp::kMzH, rzmp::kMzMaxA, rzmp::kMzObs, rzmp::kMzRootObs;   // the model's sizes: defined once, beside the packing of its weights
constexpr int kMzWaves = 4, kMzTile = 16, kMzKX = kMzH + kMzMaxA, kMzMaxGpw = 16;
constexpr int kMzRedRows = 4 + kMzMaxA;   // min, max, reward, value, logits
constexpr int kMzHeadRows = 2 + kMzMaxA;  // rew2, val, pol rows
constexpr int kMzLgStride = rzmzs::kLanes + 1;   // (CAT) floats between two games' logits in LDS: lane (game, chunk) reads bank game + 16 chunk + j
typedef float mz_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 mz_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 mz_f16x4 __attribute__((ext_vector_type(4)));

struct MzModel {        // device pointers, weights k-major: w[k][unit]
    const float *dyn1_w, *dyn1_b, *dyn2_w, *dyn2_b, *rew1_w, *rew1_b, *rew2_w, *rew2_b, *pre1_w, *pre1_b, *pol_w, *pol_b,
        *val_w, *val_b, *rep1_w, *rep1_b, *rep2_w, *rep2_b;   // rep1_w: [kMzObs][64], rows >= obs_dim zero
    // whole MOVES run dyn1 / dyn2 / rew1 / pre1 on the f16 matrix pipe with hi + lo operand pairs (k_mz_search, F16): the powers of
    // two that bring each layer's largest weight into [2^13, 2^14) -- sw of dyn1 (its 64 state columns), dyn2, rew1, pre1 -- and the
    // scale s1 <= 16 of relu(dyn1)'s f16 pieces from a bound on them (states lie in [0, 1]): [5] floats
    const float *f16_scales;
};

struct MzTrace {        // optional per-simulation outputs for the parity tests: [n_sims][n_games] (probs: x n_actions)
    int32_t *parent, *action, *leaf;
    float *reward, *probs, *value;
};

struct MzPlay {         // rz_mz_play_env (rz_mz_play_cartpole)
    int n_moves, row;                       // row = doubles per packed record = D + 4 + A
    double *state;                          // [G][Env::kState]
    long long *steps, *episode;             // [G]
    unsigned long long env_seed, noise_seed;
    double noise_frac, inv_temperature;     // inv_temperature <= 0: arg-max of the visit counts
    float alpha;
    // history on the device: every move's record -- obs (D) | action | reward | visits (A) | root value | done -- goes
    // to ring[environment][step % hist]; when an episode ends, its records are copied into `arena` as one contiguous
    // run and (environment, end step, length, first arena row) is appended to `entries`: the host reads finished
    // episodes, not moves
    double *ring;                           // [G][hist][row]
    int hist;
    long long t0;                           // global step index of the first move of this launch
    long long *ep_start;                    // [G]: step index where the running episode of an environment began
    double *arena;                          // [arena_rows][row]
    long long arena_rows;
    long long *counters;                    // [0] arena rows claimed, [1] entries, [2] episodes that did not fit (row -1)
    long long *entries;                     // [max_entries][4]
    long long max_entries;
    long long max_episode_steps;            // the time limit of an episode (CartPole-v1: 500)
};

// LDS of k_mz_search in bytes: activations, reductions, head weights, per-game scalars, paths, log table (+ the trees)
// `w1_cols`: dyn1's action columns kept in LDS -- 2, or the action count of a whole-move environment with more (mz_w1_cols)
__host__ __device__ inline int mz_search_fixed_floats(int w1_cols) {
    return kMzKX * kMzTile + (kMzH * kMzTile + 128) + kMzRedRows * kMzWaves * kMzTile + 16 + kMzHeadRows * kMzH + kMzObs * kMzTile + 16 +
           kMzTile * 16 +                  // (+ the environments of whole MOVES: kState + 3 doubles per game, 8 reserved)
           w1_cols * kMzH + kMzTile;       // (+ dyn1's action columns [action][unit] and the games' actions: the f16 layers of whole
                                           // MOVES; every byte counts -- two workgroups of 16 games share a CU's 160 KB with 1.5 KB to spare)
}
__host__ __device__ constexpr int mz_w1_cols(bool whole_moves, int n_actions) { return whole_moves && n_actions > 2 ? n_actions : 2; }
// `gumbel`: the GUMBEL instantiations add, per node of an LDS tree, log(prior) (a double) and the raw value v_hat (a float), and for
// every launch the considered-visits table (int32 [n_sims]) and the games' Gumbel rows (float [gpw][8])
// `cat`: the CAT instantiations add, behind everything else, relu(rew1)'s activations [64][16], the two heads' logits [2][16][65], their
// weights [2][64][64] and their biases [2][64]
// (the ROOTS instantiations add nothing: their observation tile and staged first layer lie in RED and XS, which are idle until the stage's end)
__host__ __device__ inline int mz_search_lds_bytes(int gpw, int cap, int path_stride, int n_sims_cfg, bool tree_lds, int w1_cols, bool gumbel = false,
                                                   bool cat = false) {
    int bytes = mz_search_fixed_floats(w1_cols) * 4 + gpw * path_stride * 4;
    bytes = (bytes + 15) / 16 * 16;
    bytes += 2 * (((n_sims_cfg + 2) * 8 + 15) / 16 * 16);   // log and sqrt tables
    if (tree_lds) bytes += gpw * (cap + 1) * (int)sizeof(MzHot) + (gpw * (cap + 1) * 4 + 15) / 16 * 16;   // records (+ a spare per game) + rewards
    if (gumbel) {
        if (tree_lds) bytes += gpw * (cap + 1) * 8 + (gpw * (cap + 1) * 4 + 15) / 16 * 16;
        bytes += (n_sims_cfg * 4 + 15) / 16 * 16 + gpw * rzmzg::kMaxA * 4;
    }
    if (cat) bytes = (bytes + 15) / 16 * 16 + (kMzH * kMzTile + 2 * kMzTile * kMzLgStride + 2 * kMzH * rzmzs::kLanes + 2 * rzmzs::kLanes) * 4;
    return bytes;
}

// Development aid (not built by default): -DRZ_MZ_PROFILE accumulates the shader-clock cycles wave 0 of workgroup 0 spends
// in each stage of k_mz_search into mz_prof[] (read with rz_mz_debug_profile).
#ifdef RZ_MZ_PROFILE
__device__ long long mz_prof[16];
#define MZ_TICK(i) do { const long long now_ = clock64(); prof_acc[i] += now_ - prof_t; prof_t = now_; } while (0)
#else
#define MZ_TICK(i)
#endif

// acc += W(16 units of this wave x 4 STEPS) . B([k][game] in LDS) on the matrix pipe
template <int STEPS>
__device__ __forceinline__ mz_f32x4 mz_tile(const float (&a)[STEPS], const float *B, int q, int n, mz_f32x4 acc) {
#pragma unroll
    for (int s = 0; s < STEPS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], B[(4 * s + q) * kMzTile + n], acc, 0, 0, 0);
    return acc;
}

// sum over the 4 lanes that hold the rows of one game (q = 0 .. 3): every lane ends with the same bits
// the value of lane l ^ 16 / l ^ 32 (gfx950 v_permlane16_swap / v_permlane32_swap: two VALU operations instead of a trip
// through the LDS crossbar)
__device__ __forceinline__ float mz_xor16(float x, int l) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float((l & 16) ? r[0] : r[1]);
}
__device__ __forceinline__ float mz_xor32(float x, int l) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float((l & 32) ? r[0] : r[1]);
}
__device__ __forceinline__ float mz_rowsum(float x, int l) {
    x += mz_xor16(x, l);
    x += mz_xor32(x, l);
    return x;
}

// dot product of the 4 rows a lane holds (16w + 4q .. +3) with a head's weights, summed over the wave's 16 rows
__device__ __forceinline__ float mz_head_partial(const mz_f32x4 &p, const float *head_row, int w, int q, int l) {
    const float4 wv = *reinterpret_cast<const float4 *>(head_row + 16 * w + 4 * q);
    float s = p[0] * wv.x;
    s = fmaf(p[1], wv.y, s);
    s = fmaf(p[2], wv.z, s);
    s = fmaf(p[3], wv.w, s);
    return mz_rowsum(s, l);
}

// ---- Gumbel MuZero on wave 0 (the GUMBEL instantiations; the rules and their one summation order: rz_mz_gumbel.h)
// A pUCT level costs two divisions; a Gumbel level costs, per child, a completed value (a division), an fp64 exp and two more divisions,
// and sums over the children that every child's score needs.  So the walk is laid out ACROSS the children: all 64 lanes of wave 0 walk,
// lane 16 q + n on game n and the actions 2 q, 2 q + 1 -- the (n, q) layout of the heads.  A lane forms its two children's terms; the
// visited-prior sums of v_mix, the visit total and maximum, the maximum and the sum of the exponentials and the (score, action) arg-max
// are combined over q with v_permlane16_swap / v_permlane32_swap in mz_rowsum's order: no LDS round trip, no barrier, and the four
// lanes of a game hold the same bits and step down together.  No log in the walk: log(prior) is formed when a node is expanded and
// kept beside the record (LDS trees: a double array beside REW; HBM trees: MzGumbel::logit); the node's raw value v_hat lives in a
// float array beside REW, in HBM in MzNode's pad word.  Expansion and backup are mz_grow_backup's arithmetic, run by the four lanes
// of a game on the same words with the same values (an HBM lane reads only what it wrote itself).
struct MzGumbel {
    const int32_t *cv;     // [n_sims]: the considered-visits table
    const float *g;        // [G][A]: the Gumbel draws of this move
    double *logit;         // [G][cap]: log(prior) of the HBM trees
    int32_t *action_out;   // [G]
    float *pi_out;         // [G][A]
    double c_visit, c_scale;
};
struct MzNoGumbel {};

// ---- categorical reward and value heads (the CAT instantiations; the rule and its one summation order: rz_mz_support.h)
// Each head is a 64 x 64 layer -- the support's B = 2 S + 1 <= 63 bins, padded with rows of zero weights and a bias of -inf -- run on the
// whole 16-game tile by all four waves with the trunk's arithmetic (v_mfma_f32_16x16x4_f32; wave w owns bins 16 w .. 16 w + 15): the
// reward head beside S3, where relu(rew1) waits in LDS (RA), the value head behind S4 on relu(pre1), which takes relu(dyn1)'s place in
// HP.  The trunk's fragments fill the registers (32 more spill inside the simulation loop), so the heads' weights wait in LDS, 32 KB:
// [head][k][64] with row k rotated by 16 k bins, so that the A operand of a step -- lane (q, n): W[bin 16 w + n][k = 4 s + q] -- is one
// conflict-free ds_read_b32 at a column the lane keeps for the launch, (16 (w + q) + n) mod 64.  The logits go to LDS as [head][game][bin]; at S5 the four lanes wave 0
// has per game each take a chunk of 16 bins -- maximum, denominator and numerator in fp64 with the header's functions -- and combine them
// with two lane exchanges in the header's order; h^-1 of the quotient is the scalar the trace, the backup and MinMax see.
struct MzSupport {
    const float *rew2_w, *rew2_b, *val_w, *val_b;   // k-major [64][64 bins] and [64] (rz_mz_pack.h: pack_model with a support)
    int S;
};
struct MzNoSupport {};

// ---- the search from raw observations (the ROOTS instantiations; rz_mz_search_obs)
// Everything in front of a search that PyTorch ran before it -- representation, root prediction, softmax, the strided copy of the root
// states, k_mz_init -- is one stage at the head of the launch, on the tiles the simulations use:
//   * the workgroup's games load their observation rows into an LDS tile [16 features][16 games] (a thread per element; rows past
//     n_games and features past obs_dim are written as zero and nothing outside the array is read), and rep1's weights, k-major
//     [16][64] with the rows past obs_dim zero (rzmp::pack_root_model), are staged with one 16-byte load per thread -- they are used
//     once, so they never become fragments that live across the simulation loop.  Neither costs LDS of its own: the tile lies in RED
//     (first written by the stage's own min-max step, a barrier after the tile's last read) and the weights in rows 0 .. 63 of XS (first
//     written by scale_and_store, two barriers after their last read; the one-hot rows behind them keep their zeros) -- 6 KB more
//     would have put the trees of Reanalyse's standing shape (2 actions, 50 simulations, 16 games: 81152 of 81920 bytes) into HBM;
//   * rep1 is four K steps of v_mfma_f32_16x16x4_f32 over the padded tile, rep2 sixteen, with the operand layout, the bias as the
//     accumulator's start and the order of accumulation of the simulations' layers (mz_tile): observations are raw -- no range is known
//     for them -- so the products are the exact f32 ones of this route's other layers, not the f16 pieces of whole moves, whose scales rest
//     on states in [0, 1].  rep2's fragments and the two biases come straight from L2 and die with the stage;
//   * the min-max scaling, the store of the root state to slot 0 of `hidden` and the prediction are the simulations' own pieces
//     (scale_and_store with Gleaf = 0, predict_partials, finish_prediction); the scaled state stays in XS, where simulation 0 -- whose
//     parent is the root in every game -- reads it without the gather from HBM;
//   * wave 0 takes the value (through h^-1 with VT) and the float32 softmax row, hands them out (root_probs; row 0 of the trace) and
//     makes the root with rz_mz_roots.h's rule, k_mz_init's: with TREE_LDS the record is born in LDS and reaches HBM with the write-out.
struct MzRoots {
    const float *obs;                        // [n_games][obs_dim]
    int obs_dim;
    const float *rep1_w, *rep1_b, *rep2_w, *rep2_b;   // rzmp::pack_root_model
    const double *noise;                     // [n_games][A] or null (GUMBEL: not read -- Gumbel roots take no noise)
    double noise_frac;
    float *root_probs;                       // [n_games][A] or null: the float32 softmax rows the roots were made from
};
struct MzNoRoots {};
// the double of lane l ^ 1 / l ^ 2 within a quad (DPP quad_perm [1, 0, 3, 2] = 0xB1, [2, 3, 0, 1] = 0x4E)
template <int CTRL>
__device__ __forceinline__ double mz_quad_f64(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <int W>
__device__ __forceinline__ unsigned mz_xor_word(unsigned x, int l) {   // the word of lane l ^ W, W = 16 | 32
    const auto r = W == 16 ? __builtin_amdgcn_permlane16_swap(x, x, false, false) : __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return (l & W) ? r[0] : r[1];
}
template <int W>
__device__ __forceinline__ double mz_xor_f64(double x, int l) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = mz_xor_word<W>((unsigned)b, l), hi = mz_xor_word<W>((unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double mzg_sum(double x, int l) {   // over q: rzmzg::sum4's order in every lane
    x += mz_xor_f64<16>(x, l);
    x += mz_xor_f64<32>(x, l);
    return x;
}

struct MzgChild {
    int N, fc;
    double prior, logit, q;
};
// the two placements of a Gumbel tree behind one set of accessors (slots relative to the game's tree)
struct MzgLds {
    MzHot *hot;
    float *rew, *vh;
    double *lgt;
    double discount;
    __device__ __forceinline__ int first_child(int s) const { return hot[s].first_child; }
    __device__ __forceinline__ MzgChild child(int s) const {
        const MzHot h = hot[s];
        return MzgChild{h.N, h.first_child, h.prior, lgt[s], h.q};
    }
    __device__ __forceinline__ double v_hat(int s) const { return (double)vh[s]; }
    __device__ __forceinline__ void set_v_hat(int s, float v) const { vh[s] = v; }
    // expand_node: the leaf's reward, children and raw value; lane q writes its own two children
    template <int MAXA>
    __device__ __forceinline__ void expand(int leaf, int top, int A, int q, float reward, const float (&probs)[MAXA], float value) const {
        rew[leaf] = reward;
        hot[leaf].first_child = top;
        vh[leaf] = value;
        float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
        for (int a = 0; a < MAXA; ++a) {
            p0 = a == 2 * q ? probs[a] : p0;
            p1 = a == 2 * q + 1 ? probs[a] : p1;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int a = 2 * q + i;
            const float p = i == 0 ? p0 : p1;
            if (a < A) {
                hot[top + a] = MzHot{0, -1, 0.0, (double)p, 0.0};
                rew[top + a] = 0.0f;
                vh[top + a] = 0.0f;
                lgt[top + a] = log((double)p);
            }
        }
    }
    // (ROOTS) the root from the row the launch has just formed: rz_mz_roots.h's records as the preamble would have read them from HBM, with
    // log(prior) and v_hat beside them; every lane of the game writes slot 0, lane q its own two children (Gumbel roots take no noise)
    template <int MAXA>
    __device__ __forceinline__ void make_root(int A, int q, const float (&probs)[MAXA], float value) const {
        const MzNode r = mz_root_record();
        hot[0] = MzHot{r.N, r.first_child, r.value_sum, r.prior, 0.0};
        rew[0] = r.reward;
        vh[0] = value;
        lgt[0] = log(r.prior);
        float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
        for (int a = 0; a < MAXA; ++a) {
            p0 = a == 2 * q ? probs[a] : p0;
            p1 = a == 2 * q + 1 ? probs[a] : p1;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int a = 2 * q + i;
            if (a < A) {
                const MzNode c = mz_root_child(mz_root_prior(i == 0 ? p0 : p1, nullptr, a, 0.0));
                hot[1 + a] = MzHot{c.N, c.first_child, c.value_sum, c.prior, 0.0};
                rew[1 + a] = c.reward;
                vh[1 + a] = __int_as_float(c.pad);
                lgt[1 + a] = log(c.prior);
            }
        }
    }
    // a level of backpropagate: -> the node's new value(), r = its reward
    __device__ __forceinline__ double visit(int s, double v, double &r) const {
        const double sum = hot[s].value_sum + v;
        const int n = hot[s].N + 1;
        r = (double)rew[s];
        const double nv = sum / (double)n;
        hot[s].value_sum = sum;
        hot[s].N = n;
        hot[s].q = r + discount * nv;
        return nv;
    }
};
struct MzgHbm {
    MzNode *nodes;
    double *lgt;
    double discount;
    __device__ __forceinline__ int first_child(int s) const { return nodes[s].first_child; }
    __device__ __forceinline__ MzgChild child(int s) const {
        const MzNode nd = nodes[s];
        return MzgChild{nd.N, nd.first_child, nd.prior, lgt[s], nd.N > 0 ? (double)nd.reward + discount * node_value(nd) : 0.0};
    }
    __device__ __forceinline__ double v_hat(int s) const { return (double)__int_as_float(nodes[s].pad); }
    __device__ __forceinline__ void set_v_hat(int s, float v) const { nodes[s].pad = __float_as_int(v); }
    // (every lane of the game writes every child: a lane then reads nothing but its own stores)
    template <int MAXA>
    __device__ __forceinline__ void expand(int leaf, int top, int A, int, float reward, const float (&probs)[MAXA], float value) const {
        nodes[leaf].reward = reward;
        nodes[leaf].first_child = top;
        nodes[leaf].pad = __float_as_int(value);
#pragma unroll
        for (int a = 0; a < MAXA; ++a) {
            if (a < A) {
                nodes[top + a] = MzNode{0, -1, 0.0, (double)probs[a], 0.0f, 0};
                lgt[top + a] = log((double)probs[a]);
            }
        }
    }
    // (ROOTS; as expand: every lane of the game writes the root and every child)
    template <int MAXA>
    __device__ __forceinline__ void make_root(int A, int, const float (&probs)[MAXA], float value) const {
        MzNode r = mz_root_record();
        lgt[0] = log(r.prior);
        r.pad = __float_as_int(value);
        nodes[0] = r;
#pragma unroll
        for (int a = 0; a < MAXA; ++a) {
            if (a < A) {
                const MzNode c = mz_root_child(mz_root_prior(probs[a], nullptr, a, 0.0));
                nodes[1 + a] = c;
                lgt[1 + a] = log(c.prior);
            }
        }
    }
    __device__ __forceinline__ double visit(int s, double v, double &r) const {
        const double sum = nodes[s].value_sum + v;
        const int n = nodes[s].N + 1;
        nodes[s].value_sum = sum;
        nodes[s].N = n;
        r = (double)nodes[s].reward;
        return sum / (double)n;
    }
};

struct MzgLane {   // a lane's two children of a node: visits, first children, s(a) = logit + sigma(completed q); the node's totals
    int n0, n1, fc0, fc1, sum_n, max_n;
    double s0, s1;
};
template <typename Tree>
__device__ __forceinline__ MzgLane mzg_scores(const MzGumbel &Z, const Tree &tree, int node, int fc, int A, int q, int l, double lo, double hi) {
    const bool h0 = 2 * q < A, h1 = 2 * q + 1 < A;
    const MzgChild none = {0, -1, 0.0, -INFINITY, 0.0};
    const MzgChild r0 = tree.child(fc + (h0 ? 2 * q : 0)), r1 = tree.child(fc + (h1 ? 2 * q + 1 : 0));
    const MzgChild c0 = h0 ? r0 : none, c1 = h1 ? r1 : none;
    const double sp = mzg_sum(rzmzg::sum2(c0.N > 0 ? c0.prior : 0.0, c1.N > 0 ? c1.prior : 0.0), l);
    const double spq = mzg_sum(rzmzg::sum2(c0.N > 0 ? c0.prior * c0.q : 0.0, c1.N > 0 ? c1.prior * c1.q : 0.0), l);
    int sn = c0.N + c1.N, mn = c0.N > c1.N ? c0.N : c1.N;
    sn += (int)mz_xor_word<16>((unsigned)sn, l);
    sn += (int)mz_xor_word<32>((unsigned)sn, l);
    mn = max(mn, (int)mz_xor_word<16>((unsigned)mn, l));
    mn = max(mn, (int)mz_xor_word<32>((unsigned)mn, l));
    const double vm = rzmzg::v_mix(tree.v_hat(node), sn, sp, spq);
    const double scale = rzmzg::sigma_scale(Z.c_visit, Z.c_scale, mn);
    MzgLane L;
    L.n0 = c0.N;
    L.n1 = c1.N;
    L.fc0 = c0.fc;
    L.fc1 = c1.fc;
    L.sum_n = sn;
    L.max_n = mn;
    L.s0 = h0 ? rzmzg::logit_score(c0.logit, scale, rzmzg::completed(c0.N, c0.q, vm, lo, hi)) : -INFINITY;
    L.s1 = h1 ? rzmzg::logit_score(c1.logit, scale, rzmzg::completed(c1.N, c1.q, vm, lo, hi)) : -INFINITY;
    return L;
}
// pi' of the lane's two children
__device__ __forceinline__ void mzg_policy(const MzgLane &L, int l, double &pi0, double &pi1) {
    double mx = L.s0 > L.s1 ? L.s0 : L.s1, o = mz_xor_f64<16>(mx, l);
    mx = o > mx ? o : mx;
    o = mz_xor_f64<32>(mx, l);
    mx = o > mx ? o : mx;
    const double e0 = exp(L.s0 - mx), e1 = exp(L.s1 - mx);
    const double den = mzg_sum(rzmzg::sum2(e0, e1), l);
    pi0 = e0 / den;
    pi1 = e1 / den;
}
// the best (score, action) of a game's children, with the winner's first child, in all four lanes
__device__ __forceinline__ void mzg_argmax(double sc0, int a0, int fc0, double sc1, int a1, int fc1, int l, int &act, int &fc) {
    bool take = rzmzg::better(sc1, a1, sc0, a0);
    double best = take ? sc1 : sc0;
    act = take ? a1 : a0;
    fc = take ? fc1 : fc0;
    double ob = mz_xor_f64<16>(best, l);
    int oa = (int)mz_xor_word<16>((unsigned)act, l), ofc = (int)mz_xor_word<16>((unsigned)fc, l);
    take = rzmzg::better(ob, oa, best, act);
    best = take ? ob : best;
    act = take ? oa : act;
    fc = take ? ofc : fc;
    ob = mz_xor_f64<32>(best, l);
    oa = (int)mz_xor_word<32>((unsigned)act, l);
    ofc = (int)mz_xor_word<32>((unsigned)fc, l);
    take = rzmzg::better(ob, oa, best, act);
    act = take ? oa : act;
    fc = take ? ofc : fc;
}

// the walk of one simulation: the root rule at depth 0 (eligible: N(a) == cv_s; score g + s), the deterministic rule below
template <typename Tree, typename PathP>
__device__ __forceinline__ int mzg_descend(const MzDev &E, const MzGumbel &Z, const Tree &tree, PathP path, int A, int q, int l, double lo, double hi,
                                           float g0, float g1, int cv_s, int &par_out, int &act_out, int &leaf_out) {
    const int a0 = 2 * q < A ? 2 * q : -1, a1 = 2 * q + 1 < A ? 2 * q + 1 : -1;   // (an action past A loses every comparison)
    int node = 0, depth = 0, par = 0, last = 0;
    path[0] = 0;
    int fc = tree.first_child(0);
    while (fc >= 0 && depth + 1 < E.path_stride) {
        const MzgLane L = mzg_scores(Z, tree, node, fc, A, q, l, lo, hi);
        double sc0, sc1;
        if (depth == 0) {
            sc0 = a0 >= 0 && L.n0 == cv_s ? rzmzg::root_score(g0, L.s0) : -INFINITY;
            sc1 = a1 >= 0 && L.n1 == cv_s ? rzmzg::root_score(g1, L.s1) : -INFINITY;
        } else {
            double pi0, pi1;
            mzg_policy(L, l, pi0, pi1);
            sc0 = a0 >= 0 ? rzmzg::below_score(pi0, L.n0, L.sum_n) : -INFINITY;
            sc1 = a1 >= 0 ? rzmzg::below_score(pi1, L.n1, L.sum_n) : -INFINITY;
        }
        int act, cfc;
        mzg_argmax(sc0, a0, L.fc0, sc1, a1, L.fc1, l, act, cfc);
        par = node;
        last = act;
        node = fc + act;
        fc = cfc;
        depth += 1;
        path[depth] = node;
    }
    par_out = par;
    act_out = last;
    leaf_out = node;
    return depth;
}

// the result of a search: the move (among the most visited, the best g + s) and the lane's two entries of pi'
template <typename Tree>
__device__ __forceinline__ int mzg_result(const MzGumbel &Z, const Tree &tree, int A, int q, int l, double lo, double hi, float g0, float g1,
                                          double &pi0, double &pi1) {
    const int a0 = 2 * q < A ? 2 * q : -1, a1 = 2 * q + 1 < A ? 2 * q + 1 : -1;
    const int fc = tree.first_child(0);
    if (fc < 0) {   // (a root rz_mz_init_roots never expanded: nothing to report)
        pi0 = pi1 = 0.0;
        return 0;
    }
    const MzgLane L = mzg_scores(Z, tree, 0, fc, A, q, l, lo, hi);
    mzg_policy(L, l, pi0, pi1);
    const double sc0 = a0 >= 0 && L.n0 == L.max_n ? rzmzg::root_score(g0, L.s0) : -INFINITY;
    const double sc1 = a1 >= 0 && L.n1 == L.max_n ? rzmzg::root_score(g1, L.s1) : -INFINITY;
    int act, cfc;
    mzg_argmax(sc0, a0, L.fc0, sc1, a1, L.fc1, l, act, cfc);
    return act;
}

// expand_node + backpropagate with mz_grow_backup's arithmetic (same operations on the same operands: same bits)
template <int MAXA, typename Tree, typename PathP>
__device__ __forceinline__ void mzg_grow_backup(const MzDev &E, const Tree &tree, PathP path, int A, int q, int depth, int &top, double &lo,
                                                double &hi, float reward_g, const float (&probs)[MAXA], float value_g) {
    const int leaf = path[depth];
    if (top + A > E.cap) {
        atomicOr(E.err, RZ_FLAG_ARENA_FULL);
    } else {
        tree.template expand<MAXA>(leaf, top, A, q, reward_g, probs, value_g);
        top += A;
    }
    double v = (double)value_g;
    for (int d = depth; d >= 0; --d) {
        double r;
        const double nv = tree.visit(path[d], v, r);
        hi = nv > hi ? nv : hi;   // MinMaxStats.update
        lo = nv < lo ? nv : lo;
        v = r + E.discount * v;
    }
}

// the environment step and observation of a whole move OUT of line, for the environments MzFarStep names: Acrobot's RK4 over double
// sin / cos takes 230 registers of its own, and inlined into k_mz_search they come out of the simulation loop's budget (the f16 weight
// fragments are live across the move: scratch loads inside the loop).  A call keeps the two apart: what is live across it is saved
// and reloaded in the move stage, once per move.
template <typename Env>
struct MzFarStep {
    static constexpr bool value = false;
};
template <>
struct MzFarStep<rzmze::EnvAcrobot> {
    static constexpr bool value = true;
};
template <typename Env>
__device__ __noinline__ int mz_env_step_far(typename Env::State &c, int action, long long max_episode_steps, double *reward) {
    return Env::step(c, action, max_episode_steps, reward);
}
template <typename Env>
__device__ __noinline__ void mz_env_observe_far(const typename Env::State &c, float *obs) {
    Env::observe(c, obs);
}

// Env: the environment of whole MOVES (a trait of rz_mz_env.h; unused without MOVES).
// MAXA: the action count the per-action loops are unrolled for (register arrays of that size): 8 in general, Env::kActions for whole
// MOVES -- 2 for CartPole, 3 for Acrobot: with 8-entry arrays the MOVES variants do not fit the 256 registers of two workgroups per
// CU (200 bytes of scratch per lane, ~20 scratch loads inside every simulation's serial chain)
// VT: the network's reward and value are in the transformed space of rz_mz_value.h (rz_mz_set_value_transform): wave 0 takes them
// through value_h_inv before the trace and the backup, so the tree, its MinMax bounds and the root value stay in raw units.
// GUMBEL (MOVES = false only): the search rule is Gumbel MuZero's (above; rz_mz_set_gumbel) instead of pUCT -- wave 0's tree phase
// is the (n, q) walk, the launch starts with the prediction of the roots' own states (their raw values) and ends with the move and
// pi' of every game in Z.action_out / Z.pi_out.  The matrix-pipe stages are the same code.  Z: MzGumbel, an empty record otherwise.
// CAT (MOVES = false, VT = true only): the reward and value heads are softmaxes over a support (above; rz_mz_set_support), read as
// h^-1 of their expectation.  C: MzSupport, an empty record otherwise.
// ROOTS (MOVES = false; CAT only with GUMBEL): the launch starts from raw observations (above; rz_mz_search_obs, rz_mz_search_obs_gumbel) --
// the trees it finds are not read, the roots are made in the launch, and the trace, when given, has a row 0 for the root in front of the
// simulations'.  With GUMBEL the stage also leaves what the GUMBEL preamble forms from records it finds -- log(prior) and v_hat of the
// root's slots -- and that preamble's second prediction on hidden[:, 0] does not run: three barriers and an L2 round trip less.
// R: MzRoots, an empty record otherwise.
template <bool TREE_LDS, bool MOVES, typename Env = rzmze::EnvCartPole, int MAXA = (MOVES ? Env::kActions : kMzMaxA), bool VT = false,
          bool GUMBEL = false, bool CAT = false, bool ROOTS = false>
__global__ __launch_bounds__(64 * kMzWaves, 2) void k_mz_search(MzDev E, MzModel M, float *hidden, int n_sims, int gpw, MzTrace T, MzPlay P,
                                                                 typename std::conditional<GUMBEL, MzGumbel, MzNoGumbel>::type Z,
                                                                 typename std::conditional<CAT, MzSupport, MzNoSupport>::type C,
                                                                 typename std::conditional<ROOTS, MzRoots, MzNoRoots>::type R) {
    static_assert(!(GUMBEL && MOVES), "whole moves keep the pUCT rule");
    static_assert(!CAT || (VT && !MOVES), "the support lies in h's space; whole moves keep scalar heads");
    static_assert(!ROOTS || (!MOVES && (GUMBEL || !CAT)), "the search from observations: pUCT with scalar heads, Gumbel with either kind");
    extern __shared__ __attribute__((aligned(16))) unsigned char mz_lds[];
    constexpr int AFIX = MOVES ? Env::kActions : 0;   // whole MOVES: the environment's action count (rz_mz_play_env checks the tree's)
    constexpr int W1C = mz_w1_cols(MOVES, Env::kActions);
    constexpr bool FAR_STEP = MzFarStep<Env>::value;   // the step and the observation as calls (mz_env_step_far)
    static_assert(Env::kState + 3 <= 8 && Env::kObs <= kMzObs && Env::kActions <= kMzMaxA, "the LDS record, OBS and the action arrays");
    const int A = AFIX > 0 ? AFIX : E.n_actions, KX = kMzH + A;
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, n = l & 15, q = l >> 4;
    const int g0 = blockIdx.x * gpw;
    float *XS = reinterpret_cast<float *>(mz_lds);   // [72][16]: parent state + one-hot action; later the scaled next state
    float *HP = XS + kMzKX * kMzTile;                // [64][16]: relu(dyn1) (relu(rep1) in the initial inference)
    float *RED = HP + kMzH * kMzTile + 128;          // [12][4 waves][16]: per-wave min / max / reward / value / logit partials
    float *HB = RED + kMzRedRows * kMzWaves * kMzTile;   // [0] rew2 bias, [1] val bias, [2 .. 2 + A) pol biases
    float *HW = HB + 16;                             // [10][64]: rew2 / val / pol weights
    float *OBS = HW + kMzHeadRows * kMzH;            // [8][16]: observations, [k][game] (MOVES)
    int *Gleaf = reinterpret_cast<int *>(OBS + kMzObs * kMzTile);   // [16]
    // MOVES: the environments (Env::kState doubles of state, steps, episode, episode start) wait in LDS between a move's first and
    // last stage -- 14 registers that the simulations in between would otherwise carry
    double *ENV = reinterpret_cast<double *>(Gleaf + 16);           // [16][8]
    float *W1A = reinterpret_cast<float *>(ENV + kMzTile * 8);       // [W1C][64]: dyn1's weights of the one-hot action rows (F16)
    int *Gact = reinterpret_cast<int *>(W1A + W1C * kMzH);           // [16]: the action of the edge into each game's leaf (F16)
    int32_t *PATH = Gact + kMzTile;                                  // [gpw][path_stride]
    unsigned char *pp = mz_lds + (mz_search_fixed_floats(W1C) * 4 + gpw * E.path_stride * 4 + 15) / 16 * 16;
    double *PBL = reinterpret_cast<double *>(pp);    // [n_sims + 2]: the host's log table
    pp += ((E.n_sims + 2) * 8 + 15) / 16 * 16;
    double *SQT = reinterpret_cast<double *>(pp);    // [n_sims + 2]: sqrt(n)
    pp += ((E.n_sims + 2) * 8 + 15) / 16 * 16;
    const int tcap = E.cap + 1;                      // slots per game in LDS: the tree + one spare record (mz_grow_backup_hot)
    MzHot *TREE = reinterpret_cast<MzHot *>(pp);     // [gpw][tcap] (TREE_LDS)
    float *REW = reinterpret_cast<float *>(pp + gpw * tcap * (int)sizeof(MzHot));   // [gpw][tcap] rewards (TREE_LDS)
    // GUMBEL, in the order of mz_search_lds_bytes: log(prior) and v_hat per node (TREE_LDS), the considered visits, the Gumbel rows
    if (TREE_LDS) pp += gpw * tcap * (int)sizeof(MzHot) + (gpw * tcap * 4 + 15) / 16 * 16;
    double *LGT = reinterpret_cast<double *>(pp);    // [gpw][tcap]
    float *VH = reinterpret_cast<float *>(pp + gpw * tcap * 8);   // [gpw][tcap]
    if (TREE_LDS) pp += gpw * tcap * 8 + (gpw * tcap * 4 + 15) / 16 * 16;
    int32_t *CV = reinterpret_cast<int32_t *>(pp);   // [n_sims]
    float *GB = reinterpret_cast<float *>(pp + (E.n_sims * 4 + 15) / 16 * 16);   // [gpw][8]
    // CAT, behind everything else (mz_search_lds_bytes): relu(rew1) [k][game] and the heads' logits [reward | value][game][kMzLgStride]
    float *RA = reinterpret_cast<float *>(mz_lds + (mz_search_lds_bytes(gpw, E.cap, E.path_stride, E.n_sims, TREE_LDS, W1C, GUMBEL, false) + 15) / 16 * 16);
    float *LG = RA + kMzH * kMzTile;
    float *WH = LG + 2 * kMzTile * kMzLgStride;      // [reward | value][k][64]: row k rotated by 16 k bins
    float *HBC = WH + 2 * kMzH * rzmzs::kLanes;      // [reward | value][64]: the heads' biases
    // ROOTS: the observation tile [feature][game] in RED and rep1's weights [k][64] in rows 0 .. 63 of XS, both dead before their hosts' first write
    static_assert(kMzRootObs * kMzTile <= kMzRedRows * kMzWaves * kMzTile && kMzRootObs <= kMzH, "the ROOTS stage's tiles fit RED and XS");
    float *OBT = RED, *W0 = XS;

    // ---- once: weight fragments into registers (A operand of 16x16x4: lane holds W[unit 16w + n][k = 4s + q])
    // (the representation network's fragments -- 18 + 8 registers, used once per MOVE -- are fetched at the start of every
    // move instead: kept for the whole launch they push the MOVES variants past the 256 registers of two workgroups per CU
    // and into scratch, in the middle of the per-simulation chain)
    // F16 (whole MOVES): the four 64 x 64 layers of a simulation on the f16 matrix pipe, v_mfma_f32_16x16x32_f16 with every
    // f32 operand a hi + lo pair of f16 values (three MFMAs per product, f32 accumulation: the network trunk's arithmetic,
    // rz_net.hip) -- 6 MFMAs of 16 cycles per layer instead of 16 .. 18 of 32.  The activations then live in LDS as
    // [game][hi: 64 f16 | lo: 64 f16 | 32 B pad] (a B fragment = one ds_read_b128: lane = 16 (k block) + game), the hidden
    // states in HBM as the same 256 bytes (the gather is a plain copy), dyn1's one-hot action rows are added as a column of
    // f32 weights.  Activation scales: 16 for states (they lie in [0, 1]), s1 for relu(dyn1) (rz_mz_load_model's bound).
    constexpr bool F16 = MOVES;
    constexpr int kRec = 288;   // bytes of a game's activation record
    float a1[F16 ? 1 : kMzKX / 4], a2[F16 ? 1 : kMzH / 4], ar[F16 ? 1 : kMzH / 4], ap[F16 ? 1 : kMzH / 4];
    mz_f16x8 f1[2][2], f2[2][2], fr[2][2], fp[2][2];   // (F16) [K-step of 32][hi | lo]: lane = 16 g + r holds W[k = 32 s + 8 g + j][unit 16 w + r]
    float d1 = 1.0f, d2 = 1.0f, dr = 1.0f, dp = 1.0f, s1 = 1.0f;
    const int unit = 16 * w + n;
    if constexpr (F16) {
        const float sw1 = M.f16_scales[0], sw2 = M.f16_scales[1], swr = M.f16_scales[2], swp = M.f16_scales[3];
        s1 = M.f16_scales[4];
        d1 = 1.0f / (16.0f * sw1);
        d2 = 1.0f / (s1 * sw2);
        dr = 1.0f / (s1 * swr);
        dp = 1.0f / (16.0f * swp);
        auto frag = [&](const float *wk, float sw, mz_f16x8 (&f)[2][2]) {
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float v = wk[(32 * st + 8 * q + j) * kMzH + unit] * sw;
                    const _Float16 hi = (_Float16)v;
                    f[st][0][j] = hi;
                    f[st][1][j] = (_Float16)(v - (float)hi);
                }
        };
        frag(M.dyn1_w, sw1, f1);
        frag(M.dyn2_w, sw2, f2);
        frag(M.rew1_w, swr, fr);
        frag(M.pre1_w, swp, fp);
        static_assert(!F16 || AFIX == W1C || AFIX < 2, "one column of dyn1 per action of the environment");
        for (int i = tid; i < AFIX * kMzH; i += 64 * kMzWaves) W1A[i] = M.dyn1_w[kMzH * kMzH + i];   // rows 64 .. 64 + A - 1 of [k][unit]
    } else {
#pragma unroll
        for (int s = 0; s < kMzKX / 4; ++s) {
            const int k = 4 * s + q;
            a1[s] = k < KX ? M.dyn1_w[k * kMzH + unit] : 0.0f;
        }
#pragma unroll
        for (int s = 0; s < kMzH / 4; ++s) {
            const int k = 4 * s + q;
            a2[s] = M.dyn2_w[k * kMzH + unit];
            ar[s] = M.rew1_w[k * kMzH + unit];
            ap[s] = M.pre1_w[k * kMzH + unit];
        }
    }
    // (F16) acc += W . X over the 64 state values of the games' records at `rec` (LDS), hi + lo pairs: 6 MFMAs
    auto mfma16 = [&](const mz_f16x8 (&f)[2][2], const unsigned char *rec, mz_f32x4 acc) {
        const unsigned char *p = rec + n * kRec + q * 16;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const mz_f16x8 bh = *reinterpret_cast<const mz_f16x8 *>(p + st * 64), bl = *reinterpret_cast<const mz_f16x8 *>(p + 128 + st * 64);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(f[st][0], bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(f[st][0], bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(f[st][1], bh, acc, 0, 0, 0);
        }
        return acc;
    };
    // (F16) the lane's 4 values (units 16 w + 4 q + i of game n), already scaled, as hi + lo pieces into the games' records
    auto store16 = [&](unsigned char *rec, const float (&z)[4], mz_f16x4 *hi_out = nullptr, mz_f16x4 *lo_out = nullptr) {
        mz_f16x4 hi, lo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            hi[i] = (_Float16)z[i];
            lo[i] = (_Float16)(z[i] - (float)hi[i]);
        }
        unsigned char *p = rec + n * kRec + (16 * w + 4 * q) * 2;
        *reinterpret_cast<mz_f16x4 *>(p) = hi;
        *reinterpret_cast<mz_f16x4 *>(p + 128) = lo;
        if (hi_out) {
            *hi_out = hi;
            *lo_out = lo;
        }
    };
    unsigned char *XS16 = reinterpret_cast<unsigned char *>(XS), *HP16 = reinterpret_cast<unsigned char *>(HP);
    mz_f32x4 b1, b2, br, bp;   // biases in the C/D layout: rows 16w + 4q + i
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 16 * w + 4 * q + i;
        b1[i] = M.dyn1_b[row];
        b2[i] = M.dyn2_b[row];
        br[i] = M.rew1_b[row];
        bp[i] = M.pre1_b[row];
    }
    if constexpr (CAT) {
        for (int i = tid; i < kMzH * rzmzs::kLanes; i += 64 * kMzWaves) {
            const int k = i >> 6, col = ((i & 63) + 16 * k) & 63;
            WH[k * rzmzs::kLanes + col] = C.rew2_w[i];
            WH[(kMzH + k) * rzmzs::kLanes + col] = C.val_w[i];
        }
        if (tid < rzmzs::kLanes) {
            HBC[tid] = C.rew2_b[tid];
            HBC[rzmzs::kLanes + tid] = C.val_b[tid];
        }
    }
    if (tid == 0) {
        HB[0] = CAT ? 0.0f : M.rew2_b[0];
        HB[1] = CAT ? 0.0f : M.val_b[0];
    }
    if (tid < A) HB[2 + tid] = M.pol_b[tid];
    for (int i = tid; i < kMzHeadRows * kMzH; i += 64 * kMzWaves) {
        const int row = i >> 6, k = i & 63;
        if constexpr (CAT) HW[i] = row >= 2 && row - 2 < A ? M.pol_w[(row - 2) * kMzH + k] : 0.0f;   // (rows 0, 1: the scalar heads, unused)
        else HW[i] = row == 0 ? M.rew2_w[k] : row == 1 ? M.val_w[k] : row - 2 < A ? M.pol_w[(row - 2) * kMzH + k] : 0.0f;
    }
    for (int i = tid; i < kMzKX * kMzTile; i += 64 * kMzWaves) XS[i] = 0.0f;   // (the padding rows 64 + A .. 71 stay zero)
    for (int i = tid; i < kMzObs * kMzTile; i += 64 * kMzWaves) OBS[i] = 0.0f;
    for (int i = tid; i < E.n_sims + 2; i += 64 * kMzWaves) {
        PBL[i] = E.pb_log[i];
        SQT[i] = sqrt((double)i);
    }
    if constexpr (GUMBEL) {
        for (int i = tid; i < n_sims; i += 64 * kMzWaves) CV[i] = Z.cv[i];
        for (int i = tid; i < gpw * rzmzg::kMaxA; i += 64 * kMzWaves) {
            const int ee = i >> 3, a = i & 7;
            GB[i] = g0 + ee < E.n_games && a < A ? Z.g[(long long)(g0 + ee) * A + a] : 0.0f;
        }
    }
    // the trees of this workgroup's games
    // wave 0 walks the trees: the four lanes of quad `ge` own game g0 + ge together -- they score different children in
    // the walk and otherwise run the same tree code on the same values (same LDS words, same bits); `lead` writes to HBM
    // (GUMBEL: lane 16 q + n works on game g0 + n -- `te` is the column of the game a lane's tree code serves)
    const int ge = l >> 2, ca = l & 3;
    const int te = GUMBEL ? n : ge;
    const bool mine = w == 0 && te < gpw && g0 + te < E.n_games;
    const bool lead = mine && (GUMBEL ? q == 0 : ca == 0);
    const int g = g0 + (te < gpw ? te : 0);
    const bool live_n = n < gpw && g0 + n < E.n_games;           // column n of the tiles is a game
    int top = 0, depth = 0;
    double lo = 0.0, hi = 0.0;
    double *env_g = ENV + 8 * ge;
    constexpr int KS = Env::kState;   // the LDS record: state | steps | episode | episode start
    typedef typename Env::State EnvState;
    auto env_load = [&](EnvState &c, long long &ep0) {
        Env::load(c, env_g, __double_as_longlong(env_g[KS]), __double_as_longlong(env_g[KS + 1]));
        ep0 = __double_as_longlong(env_g[KS + 2]);
    };
    auto env_store = [&](const EnvState &c, long long ep0) {   // (the four lanes of a quad write the same values)
        Env::store(c, env_g);
        env_g[KS] = __longlong_as_double(c.steps);
        env_g[KS + 1] = __longlong_as_double(c.episode);
        env_g[KS + 2] = __longlong_as_double(ep0);
    };
    // the observation of `c` into column `ge` of OBS (rows past Env::kObs stay zero, as rep1_w's rows past obs_dim)
    auto env_observe = [&](const EnvState &c) {
        float o[Env::kObs];
        if constexpr (FAR_STEP) mz_env_observe_far<Env>(c, o);
        else Env::observe(c, o);
#pragma unroll
        for (int i = 0; i < Env::kObs; ++i) OBS[i * kMzTile + ge] = o[i];
    };
    if (mine) {
        if (MOVES) {
            EnvState c0;
            Env::load(c0, P.state + (long long)KS * g, P.steps[g], P.episode[g]);
            env_store(c0, P.ep_start[g]);
        } else if (!ROOTS) {   // (ROOTS: the trees start in the launch)
            top = E.top[g];
            lo = E.vmin[g];
            hi = E.vmax[g];
            // (GUMBEL) the schedule counts from roots rz_mz_init_roots has just made: anything else is flagged, not searched on quietly
            if (GUMBEL && lead && top != 1 + A) atomicOr(E.err, RZ_FLAG_INTERNAL);
        }
    }
    if (TREE_LDS && !MOVES && !ROOTS) {
        for (int ee = 0; ee < gpw && g0 + ee < E.n_games; ++ee) {
            const MzNode *src = E.nodes + (long long)(g0 + ee) * E.cap;
            const int used = E.top[g0 + ee] < E.cap ? E.top[g0 + ee] : E.cap;
            for (int i = tid; i < used; i += 64 * kMzWaves) {
                const MzNode nd = src[i];
                TREE[ee * tcap + i] = MzHot{nd.N, nd.first_child, nd.value_sum, nd.prior,
                                            nd.N > 0 ? (double)nd.reward + E.discount * node_value(nd) : 0.0};
                REW[ee * tcap + i] = nd.reward;
            }
        }
    }
    MzNode *nodes = E.nodes + (long long)g * E.cap;                 // (!TREE_LDS)
    MzHot *hot = TREE + (te < gpw ? te : 0) * tcap;                 // (TREE_LDS)
    float *rew = REW + (te < gpw ? te : 0) * tcap;
    int32_t *path = PATH + (te < gpw ? te : 0) * E.path_stride;
    // (GUMBEL) the game's tree behind its accessors, log(prior) and v_hat of the nodes that are there already
    const auto gtree = [&]() {
        if constexpr (!GUMBEL) return 0;
        else if constexpr (TREE_LDS) return MzgLds{hot, rew, VH + (te < gpw ? te : 0) * tcap, LGT + (te < gpw ? te : 0) * tcap, E.discount};
        else return MzgHbm{nodes, Z.logit + (long long)g * E.cap, E.discount};
    }();
    (void)gtree;
    if constexpr (GUMBEL && !ROOTS) {   // (ROOTS: the stage that makes the roots writes both beside the records)
        for (int ee = 0; ee < gpw && g0 + ee < E.n_games; ++ee) {
            const MzNode *src = E.nodes + (long long)(g0 + ee) * E.cap;
            const int used = E.top[g0 + ee] < E.cap ? E.top[g0 + ee] : E.cap;
            for (int i = tid; i < used; i += 64 * kMzWaves) {
                if (TREE_LDS) {
                    LGT[ee * tcap + i] = log(src[i].prior);
                    VH[ee * tcap + i] = __int_as_float(src[i].pad);
                } else {
                    Z.logit[(long long)(g0 + ee) * E.cap + i] = log(src[i].prior);
                }
            }
        }
    }
    __syncthreads();
    if (MOVES && mine) {   // (after the zero fill of OBS)
        EnvState c0;
        long long ep0;
        env_load(c0, ep0);
        env_observe(c0);
    }

    // ---- the pieces the initial inference and a simulation share
    // per-sample min-max scaling of a new state t (network.py scale_hidden) from the per-wave extremes in RED: the scaled
    // rows go to XS (the next layer's input) and to the hidden-state slot Gleaf[game] of the game
    auto scale_and_store = [&](const mz_f32x4 &t) {
        float mn = RED[n], mx = RED[kMzWaves * kMzTile + n];
#pragma unroll
        for (int u = 1; u < kMzWaves; ++u) {
            mn = fminf(mn, RED[u * kMzTile + n]);
            mx = fmaxf(mx, RED[(kMzWaves + u) * kMzTile + n]);
        }
        const float inv = fmaxf(mx - mn, 1e-5f);
        float4 sv;
        if constexpr (F16) {   // one division per game and lane instead of four (1 ulp from x / inv: the pieces carry 1e-7 anyway)
            const float rinv = 1.0f / inv;
            sv.x = (t[0] - mn) * rinv;
            sv.y = (t[1] - mn) * rinv;
            sv.z = (t[2] - mn) * rinv;
            sv.w = (t[3] - mn) * rinv;
        } else {
            sv.x = (t[0] - mn) / inv;
            sv.y = (t[1] - mn) / inv;
            sv.z = (t[2] - mn) / inv;
            sv.w = (t[3] - mn) / inv;
        }
        if constexpr (F16) {
            const float z[4] = {sv.x * 16.0f, sv.y * 16.0f, sv.z * 16.0f, sv.w * 16.0f};
            mz_f16x4 hi, lo;
            store16(XS16, z, &hi, &lo);
            if (live_n) {   // the same 256 bytes as the game's hidden-state slot
                unsigned char *dst = reinterpret_cast<unsigned char *>(hidden + ((long long)(g0 + n) * E.cap + Gleaf[n]) * kMzH) + (16 * w + 4 * q) * 2;
                *reinterpret_cast<mz_f16x4 *>(dst) = hi;
                *reinterpret_cast<mz_f16x4 *>(dst + 128) = lo;
            }
        } else {
            XS[(16 * w + 4 * q + 0) * kMzTile + n] = sv.x;
            XS[(16 * w + 4 * q + 1) * kMzTile + n] = sv.y;
            XS[(16 * w + 4 * q + 2) * kMzTile + n] = sv.z;
            XS[(16 * w + 4 * q + 3) * kMzTile + n] = sv.w;
            if (live_n) *reinterpret_cast<float4 *>(hidden + ((long long)(g0 + n) * E.cap + Gleaf[n]) * kMzH + 16 * w + 4 * q) = sv;
        }
    };
    auto wave_extremes = [&](const mz_f32x4 &t) {
        float mn = fminf(fminf(t[0], t[1]), fminf(t[2], t[3])), mx = fmaxf(fmaxf(t[0], t[1]), fmaxf(t[2], t[3]));
        mn = fminf(mn, mz_xor16(mn, l));
        mx = fmaxf(mx, mz_xor16(mx, l));
        mn = fminf(mn, mz_xor32(mn, l));
        mx = fmaxf(mx, mz_xor32(mx, l));
        if (q == 0) {
            RED[(0 * kMzWaves + w) * kMzTile + n] = mn;
            RED[(1 * kMzWaves + w) * kMzTile + n] = mx;
        }
    };
    // prediction f(s) on the state in XS: p1 = relu(pre1 s), per-wave partial sums of the value and policy heads
    auto predict_partials = [&]() {
        mz_f32x4 p;
        if constexpr (F16) {
            p = mfma16(fp, XS16, mz_f32x4{0.0f, 0.0f, 0.0f, 0.0f});
#pragma unroll
            for (int i = 0; i < 4; ++i) p[i] = fmaxf(fmaf(p[i], dp, bp[i]), 0.0f);
        } else {
            p = mz_tile(ap, XS, q, n, bp);
#pragma unroll
            for (int i = 0; i < 4; ++i) p[i] = fmaxf(p[i], 0.0f);
        }
        if constexpr (CAT) {   // the value head is a layer of its own (value_logits): relu(pre1) takes relu(dyn1)'s place
#pragma unroll
            for (int i = 0; i < 4; ++i) HP[(16 * w + 4 * q + i) * kMzTile + n] = p[i];
        } else {
            const float pv = mz_head_partial(p, HW + 1 * kMzH, w, q, l);
            if (q == 0) RED[(3 * kMzWaves + w) * kMzTile + n] = pv;
        }
#pragma unroll
        for (int a = 0; a < MAXA; ++a) {
            if (a < A) {
                const float pl = mz_head_partial(p, HW + (2 + a) * kMzH, w, q, l);
                if (q == 0) RED[((4 + a) * kMzWaves + w) * kMzTile + n] = pl;
            }
        }
    };
    // (CAT) a head's logits for the tile from the activations `act` [k][game]: this wave's 16 bins of every game -> LG[head]
    auto head_logits = [&](const float *act, int head) {
        if constexpr (CAT) {
            const float4 bias = *reinterpret_cast<const float4 *>(HBC + head * rzmzs::kLanes + 16 * w + 4 * q);
            mz_f32x4 lg = {bias.x, bias.y, bias.z, bias.w};
            const float *wk = WH + (head * kMzH + q) * rzmzs::kLanes + ((16 * (w + q) + n) & 63);
#pragma unroll
            for (int s = 0; s < kMzH / 4; ++s)
                lg = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[4 * s * rzmzs::kLanes], act[(4 * s + q) * kMzTile + n], lg, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) LG[(head * kMzTile + n) * kMzLgStride + 16 * w + 4 * q + i] = lg[i];
        }
    };
    // (CAT, every lane of wave 0) h^-1 of the expectation of game `te`'s head: the lane's chunk of 16 bins, then the game's four lanes
    // combined in rzmzs::combine4's order -- two exchanges, c ^ 1 then c ^ 2 (GUMBEL: lanes 16 q + n; else the quad 4 ge + ca)
    auto cat_scalar = [&](int head) -> float {
        if constexpr (CAT) {
            const int c = GUMBEL ? q : (l & 3);
            const float *x = LG + (head * kMzTile + te) * kMzLgStride + rzmzs::kChunk * c;
            auto x1 = [&](double v) { return GUMBEL ? mz_xor_f64<16>(v, l) : mz_quad_f64<0xB1>(v); };
            auto x2 = [&](double v) { return GUMBEL ? mz_xor_f64<32>(v, l) : mz_quad_f64<0x4E>(v); };
            double m = rzmzs::chunk_max(x, c, C.S), o = x1(m);
            m = o > m ? o : m;
            o = x2(m);
            m = o > m ? o : m;
            double den, num;
            rzmzs::chunk_sums(x, c, C.S, m, &den, &num);
            den = den + x1(den);
            num = num + x1(num);
            den = den + x2(den);
            num = num + x2(num);
            return (float)rzmzv::value_h_inv(num / den);
        } else {
            return 0.0f;
        }
    };
    // (lane that owns a game) value and softmax(policy logits) from the partial sums, waves in order (CAT: the value is cat_scalar's)
    auto finish_prediction = [&](float &value, float (&probs)[MAXA]) {
        value = HB[1];
#pragma unroll
        for (int u = 0; u < (CAT ? 0 : kMzWaves); ++u) value += RED[(3 * kMzWaves + u) * kMzTile + te];
        float logit[MAXA], mxl = -INFINITY;
#pragma unroll
        for (int a = 0; a < MAXA; ++a) {
            logit[a] = -INFINITY;
            if (a < A) {
                float x = HB[2 + a];
#pragma unroll
                for (int u = 0; u < kMzWaves; ++u) x += RED[((4 + a) * kMzWaves + u) * kMzTile + te];
                logit[a] = x;
                mxl = fmaxf(mxl, x);
            }
        }
        float den = 0.0f;
#pragma unroll
        for (int a = 0; a < MAXA; ++a) {
            probs[a] = a < A ? expf(logit[a] - mxl) : 0.0f;
            den += probs[a];
        }
#pragma unroll
        for (int a = 0; a < MAXA; ++a) probs[a] = probs[a] / den;
    };

#ifdef RZ_MZ_PROFILE
    long long prof_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, prof_t = clock64();
#endif
    float touch_sink = 0.0f;   // mz_touch
    const int n_moves = MOVES ? P.n_moves : 1;
    for (int move = 0; move < n_moves; ++move) {
        if (MOVES) {
            // ---- initial inference: s0 = scale(rep2 relu(rep1 obs)) -> hidden slot 0; root priors = softmax(pol(relu(pre1 s0)))
            // the representation network's fragments and biases, from L2 (laundered pointers: the loads stay inside the move)
            float arep1[kMzObs / 4], arep2[kMzH / 4];
            mz_f32x4 brep1, brep2;
            {
                const float *r1w = M.rep1_w, *r2w = M.rep2_w, *r1b = M.rep1_b, *r2b = M.rep2_b;
                asm volatile("" : "+s"(r1w), "+s"(r2w), "+s"(r1b), "+s"(r2b));
#pragma unroll
                for (int s = 0; s < kMzObs / 4; ++s) arep1[s] = r1w[(4 * s + q) * kMzH + unit];
#pragma unroll
                for (int s = 0; s < kMzH / 4; ++s) arep2[s] = r2w[(4 * s + q) * kMzH + unit];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    brep1[i] = r1b[16 * w + 4 * q + i];
                    brep2[i] = r2b[16 * w + 4 * q + i];
                }
            }
            __syncthreads();   // (OBS of this move is written; the last move's reads of RED / XS are over)
            if (tid < kMzTile) Gleaf[tid] = 0;
            {
                mz_f32x4 h = mz_tile(arep1, OBS, q, n, brep1);
#pragma unroll
                for (int i = 0; i < 4; ++i) HP[(16 * w + 4 * q + i) * kMzTile + n] = fmaxf(h[i], 0.0f);
            }
            __syncthreads();
            const mz_f32x4 t0 = mz_tile(arep2, HP, q, n, brep2);
            wave_extremes(t0);
            __syncthreads();
            scale_and_store(t0);
            __syncthreads();
            predict_partials();
            __syncthreads();
            if (w == 0) {
                float value, probs[MAXA];
                finish_prediction(value, probs);
                if (mine) {
                    // expand_node(root) + add_exploration_noise: prior * (1 - frac) + noise * frac (k_mz_init), fresh MinMaxStats
                    // (`ns`: the seed of the keys, opaque per move -- hoisted out of the move loop the three hashes of seed and game lived
                    // in registers for the whole launch, and three of them in scratch memory)
                    unsigned long long ns = P.noise_seed;
                    asm volatile("" : "+v"(ns));
                    const uint64_t key = rzmze::move_key(ns, 0ull, g, __double_as_longlong(env_g[5]), __double_as_longlong(env_g[4]));
                    // Both distributions are normalised in fp64 here, once per move: the float32 softmax and a float32 sum of the
                    // gamma draws each add up to 1 only within a float32 ulp (6e-8), and the pseudocode's root priors are a
                    // distribution (they sum to 1 within 1e-12: tests/test_muzero_moves_tree.py)
                    float gam[MAXA];
                    const double gsum = mz_root_gammas(P.alpha, key, A, gam);
                    double psum = 0.0;
#pragma unroll
                    for (int a = 0; a < MAXA; ++a) psum += (double)probs[a];   // (0 past the last action: finish_prediction)
                    if (TREE_LDS) {
                        hot[0] = MzHot{0, 1, 0.0, 0.0, 0.0};
                        rew[0] = 0.0f;
                    } else {
                        nodes[0] = MzNode{0, 1, 0.0, 0.0, 0.0f, 0};
                    }
#pragma unroll
                    for (int a = 0; a < MAXA; ++a) {
                        if (a < A) {
                            double pr = (double)probs[a] / psum;
                            if (P.noise_frac > 0.0) {
                                double nf = P.noise_frac;
                                asm volatile("" : "+v"(nf));   // (1 - nf formed here, not carried through the launch)
                                pr = pr * (1.0 - nf) + ((double)gam[a] / gsum) * nf;
                            }
                            if (TREE_LDS) {
                                hot[1 + a] = MzHot{0, -1, 0.0, pr, 0.0};
                                rew[1 + a] = 0.0f;
                            } else {
                                nodes[1 + a] = MzNode{0, -1, 0.0, pr, 0.0f, 0};
                            }
                        }
                    }
                    top = 1 + A;
                    lo = INFINITY;
                    hi = -INFINITY;
                    depth = 0;
                }
            }
            MZ_TICK(13);
        }
        if constexpr (ROOTS) {
            // ---- the roots from raw observations (MzRoots, above): s0 = scale(rep2 relu(rep1 obs)) -> XS and hidden slot 0; f(s0) -> the roots
            OBT[(tid >> 4) * kMzTile + n] =   // 256 threads = 16 features x 16 games: feature tid / 16 of game g0 + n
                (tid >> 4) < R.obs_dim && live_n ? R.obs[(long long)(g0 + n) * R.obs_dim + (tid >> 4)] : 0.0f;
            reinterpret_cast<float4 *>(W0)[tid] = reinterpret_cast<const float4 *>(R.rep1_w)[tid];   // (after the preamble's barrier: XS is zeroed)
            if (tid < kMzTile) Gleaf[tid] = 0;
            float arep2[kMzH / 4];
            mz_f32x4 brep1, brep2;
#pragma unroll
            for (int s = 0; s < kMzH / 4; ++s) arep2[s] = R.rep2_w[(4 * s + q) * kMzH + unit];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                brep1[i] = R.rep1_b[16 * w + 4 * q + i];
                brep2[i] = R.rep2_b[16 * w + 4 * q + i];
            }
            __syncthreads();
            {
                float arep1[kMzRootObs / 4];
#pragma unroll
                for (int s = 0; s < kMzRootObs / 4; ++s) arep1[s] = W0[(4 * s + q) * kMzH + unit];
                const mz_f32x4 h = mz_tile(arep1, OBT, q, n, brep1);
#pragma unroll
                for (int i = 0; i < 4; ++i) HP[(16 * w + 4 * q + i) * kMzTile + n] = fmaxf(h[i], 0.0f);
            }
            __syncthreads();
            const mz_f32x4 t0 = mz_tile(arep2, HP, q, n, brep2);
            wave_extremes(t0);
            __syncthreads();
            scale_and_store(t0);
            __syncthreads();
            predict_partials();
            __syncthreads();
            if constexpr (CAT) {   // (as S4b: the value head on relu(pre1) of the root tile; WH and HBC stand since the preamble's barrier)
                head_logits(HP, 1);
                __syncthreads();
            }
            if (w == 0) {
                float value, probs[MAXA];
                finish_prediction(value, probs);
                if constexpr (CAT) value = cat_scalar(1);
                else if constexpr (VT) value = (float)rzmzv::value_h_inv((double)value);   // (as any other node's)
                if (mine) {
                    if (lead) {
#pragma unroll
                        for (int a = 0; a < MAXA; ++a)
                            if (a < A && R.root_probs != nullptr) R.root_probs[(long long)g * A + a] = probs[a];
                        if (T.reward != nullptr) {   // row 0 of the trace: the root (no edge leads to it)
                            T.parent[g] = -1;
                            T.action[g] = -1;
                            T.leaf[g] = 0;
                            T.reward[g] = 0.0f;
                            T.value[g] = value;
#pragma unroll
                            for (int a = 0; a < MAXA; ++a)
                                if (a < A) T.probs[(long long)g * A + a] = probs[a];
                        }
                    }
                    // expand_node(root) + add_exploration_noise with k_mz_init's rule (rz_mz_roots.h); an LDS tree takes the record as
                    // the preamble of the other instantiations would have read it from HBM
                    auto put = [&](int slot, const MzNode &nd) {
                        if (TREE_LDS) {
                            hot[slot] = MzHot{nd.N, nd.first_child, nd.value_sum, nd.prior, 0.0};
                            rew[slot] = nd.reward;
                        } else {
                            nodes[slot] = nd;
                        }
                    };
                    if constexpr (GUMBEL) {
                        // the (n, q) layout: the four lanes 16 q + n of game n hold the same row and value (finish_prediction and cat_scalar
                        // leave the same bits in each) and all take the start below, so they step down together from simulation 0; the root's
                        // v_hat is this stage's own value -- the preamble's second prediction on hidden[:, 0] does not run
                        gtree.template make_root<MAXA>(A, q, probs, value);
                    } else {
                        const double *noise_row = R.noise != nullptr ? R.noise + (long long)g * A : nullptr;
                        put(0, mz_root_record());
#pragma unroll
                        for (int a = 0; a < MAXA; ++a)
                            if (a < A) put(1 + a, mz_root_child(mz_root_prior(probs[a], noise_row, a, R.noise_frac)));
                    }
                    const MzRootStart start = mz_root_start(A);
                    top = start.top;
                    depth = start.depth;
                    lo = start.lo;
                    hi = start.hi;
                }
            }
        }
        // (GUMBEL) the quad of a game is live: the gathers below run in the quad layout whichever lanes walk
        const bool live_quad = GUMBEL ? ge < gpw && g0 + ge < E.n_games : mine;
        float gum0 = 0.0f, gum1 = 0.0f;   // (GUMBEL) the Gumbel draws of the lane's two actions
        if constexpr (GUMBEL && !ROOTS) {
            // ---- the roots' raw values: the prediction on the states the search starts from (v_mix of the root needs v_hat)
            // (ROOTS: the stage above has predicted on these very states, still in XS, and set the root's v_hat from wave 0's registers)
            if (w == 0) {
                const float4 *src = reinterpret_cast<const float4 *>(hidden + (long long)(g0 + (live_quad ? ge : 0)) * E.cap * kMzH);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = ca + 4 * j;
                    const float4 v = live_quad ? src[c] : float4{0.0f, 0.0f, 0.0f, 0.0f};
                    XS[(4 * c + 0) * kMzTile + ge] = v.x;
                    XS[(4 * c + 1) * kMzTile + ge] = v.y;
                    XS[(4 * c + 2) * kMzTile + ge] = v.z;
                    XS[(4 * c + 3) * kMzTile + ge] = v.w;
                }
            }
            __syncthreads();
            predict_partials();
            __syncthreads();
            if constexpr (CAT) {
                head_logits(HP, 1);
                __syncthreads();
            }
            if (w == 0) {
                float value, probs[MAXA];
                finish_prediction(value, probs);
                if constexpr (CAT) value = cat_scalar(1);
                else if constexpr (VT) value = (float)rzmzv::value_h_inv((double)value);
                if (mine) gtree.set_v_hat(0, value);
            }
        }
        if constexpr (GUMBEL) {
            if (w == 0) {
                gum0 = GB[(te < gpw ? te : 0) * rzmzg::kMaxA + 2 * q];
                gum1 = GB[(te < gpw ? te : 0) * rzmzg::kMaxA + 2 * q + 1];
            }
        }
    for (int sim = 0; sim < n_sims; ++sim) {
        // S0 (wave 0): select, one lane per game; then the gather of the parents' hidden states into XS[k][game]
        // (lane -> game l / 4, four 16-byte pieces of its 256-byte row) and the one-hot action rows
        int par = 0, act = 0, lf = 0;
        if (w == 0) {
            if constexpr (GUMBEL) {
                if (mine) depth = mzg_descend(E, Z, gtree, path, A, q, l, lo, hi, gum0, gum1, CV[sim], par, act, lf);
            } else {
                if (mine)
                    depth = TREE_LDS ? mz_descend_hot<AFIX>(E, hot, path, PBL, SQT, lo, hi, ca, hidden + (long long)g * E.cap * kMzH, touch_sink, par, act, lf)
                                     : mz_descend(E, nodes, path, PBL, lo, hi, par, act, lf);
            }
            MZ_TICK(0);
#ifdef RZ_MZ_PROFILE
            {   // the wave walks as long as its deepest game
                int md = mine ? depth : 0;
                for (int off = 32; off >= 1; off >>= 1) md = max(md, __shfl_xor(md, off));
                prof_acc[15] += md;
            }
#endif
            if (GUMBEL ? q == 0 : ca == 0) Gleaf[te] = lf;
            // (the quad of a game also gathers its parent's state: 4 x 64 bytes per lane; GUMBEL: lane `ge` walked that game)
            const int ee = ge, pe = GUMBEL ? __shfl(par, ge) : par;
            const bool live_e = live_quad;
            const float4 *src = reinterpret_cast<const float4 *>(hidden + ((long long)(g0 + (live_e ? ee : 0)) * E.cap + pe) * kMzH);
            if constexpr (F16) {   // the slot holds the record's 256 bytes as they are: a copy (16 games x 4 lanes x 4 pieces)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = (l & 3) + 4 * j;
                    const float4 v = live_e ? src[c] : float4{0.0f, 0.0f, 0.0f, 0.0f};
                    *reinterpret_cast<float4 *>(XS16 + ee * kRec + c * 16) = v;
                }
                if (ca == 0) Gact[ge] = mine ? act : 0;
            } else {
                // (ROOTS: every game's parent in simulation 0 is its root, whose state the ROOTS stage left in XS)
                if (!(ROOTS && sim == 0)) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int c = (l & 3) + 4 * j;
                        const float4 v = live_e ? src[c] : float4{0.0f, 0.0f, 0.0f, 0.0f};
                        XS[(4 * c + 0) * kMzTile + ee] = v.x;
                        XS[(4 * c + 1) * kMzTile + ee] = v.y;
                        XS[(4 * c + 2) * kMzTile + ee] = v.z;
                        XS[(4 * c + 3) * kMzTile + ee] = v.w;
                    }
                }
                const int an = GUMBEL ? act : __shfl(act, 4 * n);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int a = q + 4 * j;
                    if (a < A) XS[(kMzH + a) * kMzTile + n] = (live_n && an == a) ? 1.0f : 0.0f;
                }
            }
            mz_touch_done(touch_sink);
            MZ_TICK(1);
        }
        __syncthreads();
        MZ_TICK(2);
        // S1: h1 = relu(dyn1 [x, onehot(a)])
        if constexpr (F16) {
            const mz_f32x4 acc = mfma16(f1, XS16, mz_f32x4{0.0f, 0.0f, 0.0f, 0.0f});
            const float4 wa = *reinterpret_cast<const float4 *>(W1A + Gact[n] * kMzH + 16 * w + 4 * q);   // the one-hot action's row of weights
            const float col[4] = {wa.x, wa.y, wa.z, wa.w};
            float z[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = fmaxf(fmaf(acc[i], d1, col[i] + b1[i]), 0.0f) * s1;
            store16(HP16, z);
        } else {
            const mz_f32x4 acc = mz_tile(a1, XS, q, n, b1);
#pragma unroll
            for (int i = 0; i < 4; ++i) HP[(16 * w + 4 * q + i) * kMzTile + n] = fmaxf(acc[i], 0.0f);
        }
        MZ_TICK(3);
        __syncthreads();
        MZ_TICK(4);
        // S2: next state (dyn2, before scaling) and the reward head (rew2 relu(rew1 h1)) from the same activations
        mz_f32x4 t = b2;
        {
            mz_f32x4 r = br;
            if constexpr (F16) {
                t = mfma16(f2, HP16, mz_f32x4{0.0f, 0.0f, 0.0f, 0.0f});
                r = mfma16(fr, HP16, mz_f32x4{0.0f, 0.0f, 0.0f, 0.0f});
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    t[i] = fmaf(t[i], d2, b2[i]);
                    r[i] = fmaf(r[i], dr, br[i]);
                }
            } else {
#pragma unroll
                for (int s = 0; s < kMzH / 4; ++s) {
                    const float x = HP[(4 * s + q) * kMzTile + n];
                    t = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[s], x, t, 0, 0, 0);
                    r = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[s], x, r, 0, 0, 0);
                }
            }
            wave_extremes(t);
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = fmaxf(r[i], 0.0f);
            if constexpr (CAT) {   // the reward head runs beside S3, on these activations
#pragma unroll
                for (int i = 0; i < 4; ++i) RA[(16 * w + 4 * q + i) * kMzTile + n] = r[i];
            } else {
                const float pr = mz_head_partial(r, HW, w, q, l);
                if (q == 0) RED[(2 * kMzWaves + w) * kMzTile + n] = pr;
            }
        }
        MZ_TICK(5);
        __syncthreads();
        MZ_TICK(6);
        // S3: per-sample min-max scaling of the new state, stored for the leaf
        scale_and_store(t);
        head_logits(RA, 0);
        MZ_TICK(7);
        __syncthreads();
        MZ_TICK(8);
        // S4: prediction on the new state
        predict_partials();
        MZ_TICK(9);
        __syncthreads();
        if constexpr (CAT) {   // S4b: the value head on relu(pre1)
            head_logits(HP, 1);
            __syncthreads();
        }
        MZ_TICK(10);
        // S5 (wave 0): finish the heads, expand + backup
        if (w == 0) {
            float reward = HB[0];
#pragma unroll
            for (int u = 0; u < (CAT ? 0 : kMzWaves); ++u) reward += RED[(2 * kMzWaves + u) * kMzTile + te];
            float value, probs[MAXA];
            finish_prediction(value, probs);
            if constexpr (CAT) {
                reward = cat_scalar(0);
                value = cat_scalar(1);
            } else if constexpr (VT) {   // widened, inverted in fp64, rounded once
                reward = (float)rzmzv::value_h_inv((double)reward);
                value = (float)rzmzv::value_h_inv((double)value);
            }
            MZ_TICK(11);
            if (mine) {
                if (!MOVES && lead && T.reward != nullptr) {
                    const long long o = (long long)(sim + (ROOTS ? 1 : 0)) * E.n_games + g;   // (ROOTS: row 0 is the root's)
                    T.parent[o] = par;
                    T.action[o] = act;
                    T.leaf[o] = lf;
                    T.reward[o] = reward;
                    T.value[o] = value;
#pragma unroll
                    for (int a = 0; a < MAXA; ++a)
                        if (a < A) T.probs[o * A + a] = probs[a];
                }
                if constexpr (GUMBEL) mzg_grow_backup<MAXA>(E, gtree, path, A, q, depth, top, lo, hi, reward, probs, value);
                else if (TREE_LDS) mz_grow_backup_hot<MAXA, AFIX>(E, hot, rew, path, E.cap, ca, depth, top, lo, hi, reward, probs, value);
                else mz_grow_backup<MAXA>(E, nodes, path, depth, top, lo, hi, reward, probs, value);
            }
            MZ_TICK(12);
        }
        // (no barrier: the next select and gather are wave 0's too; XS -- which the gather rewrites -- was last read
        // before the barrier behind S4, and RED, which wave 0 reads above, is rewritten only after the next S0 barrier)
    }
        if constexpr (GUMBEL) {
            // ---- the result: the move and pi' of every game, a lane its two entries (no launch behind this one)
            if (mine) {
                double pi0, pi1;
                const int move_g = mzg_result(Z, gtree, A, q, l, lo, hi, gum0, gum1, pi0, pi1);
                if (q == 0) Z.action_out[g] = move_g;
                if (2 * q < A) Z.pi_out[(long long)g * A + 2 * q] = (float)pi0;
                if (2 * q + 1 < A) Z.pi_out[(long long)g * A + 2 * q + 1] = (float)pi1;
            }
        }
        if (MOVES && mine) {
            // ---- the move: action ~ visits ^ (1 / T) (select_action), record for the host, environment step
            EnvState env;
            long long ep_start;
            env_load(env, ep_start);
            double wgt[MAXA], total;
            int visits[MAXA];
#pragma unroll
            for (int a = 0; a < MAXA; ++a) visits[a] = a < A ? (TREE_LDS ? hot[1 + a].N : nodes[1 + a].N) : 0;
            int action = rzmze::move_weights(visits, A, P.inv_temperature, wgt, &total);
            if (P.inv_temperature > 0.0) {
                unsigned long long ns = P.noise_seed;
                asm volatile("" : "+v"(ns));   // (as at the root noise)
                action = rzmze::move_draw(wgt, A, total, rzmze::move_key(ns, 0xA5A5A5A5ull, g, env.episode, env.steps));
            }
            const double root_sum = TREE_LDS ? hot[0].value_sum : nodes[0].value_sum;
            const int root_n = TREE_LDS ? hot[0].N : nodes[0].N;
            const long long t = P.t0 + move;
            double *ring_g = P.ring + (long long)g * P.hist * P.row;
            double *rec = ring_g + (t % P.hist) * P.row;
            constexpr rzmze::RecordLayout R = rzmze::record_layout(Env::kObs, MAXA);   // (MOVES: MAXA is the environment's action count)
            constexpr int NLAST = R.root_value;   // obs | action | reward | visits
            double last[NLAST];
#pragma unroll
            for (int i = 0; i < Env::kObs; ++i) last[i] = (double)OBS[i * kMzTile + ge];   // the observation the search started from
            last[R.action] = (double)action;
#pragma unroll
            for (int a = 0; a < MAXA; ++a) last[R.visits + a] = (double)visits[a];
            const double root_value = root_sum / (double)(root_n > 1 ? root_n : 1);
            double step_reward = 0.0;
            const int done = FAR_STEP ? mz_env_step_far<Env>(env, action, P.max_episode_steps, &step_reward)
                                      : Env::step(env, action, P.max_episode_steps, &step_reward);
            last[R.reward] = step_reward;
            if (lead) {
#pragma unroll
                for (int c = 0; c < NLAST; ++c)
                    if (c < R.root_value) rec[c] = last[c];
                rec[R.root_value] = root_value;
                rec[R.done] = done ? 1.0 : 0.0;
            }
            if (done) {
                // the episode's records as one run in the arena: the quad copies the earlier moves from the ring, the
                // lead adds this move's from its registers
                const long long len = t + 1 - ep_start;
                long long off = -1;
                if (lead) off = mz_claim_episode<false>(P.counters, P.arena_rows, P.entries, P.max_entries, g, t + 1, len);
                off = __shfl(off, l & ~3);
                if (off >= 0) {
                    for (long long j = ca; j < len - 1; j += 4) {
                        const double *src = ring_g + ((ep_start + j) % P.hist) * P.row;
                        double *dst = P.arena + (off + j) * P.row;
                        for (int c = 0; c < P.row; ++c)
                            dst[c] = __hip_atomic_load(src + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (past the L1: written by other launches / moves)
                    }
                    if (lead) {
                        double *dst = P.arena + (off + len - 1) * P.row;
#pragma unroll
                        for (int c = 0; c < NLAST; ++c)
                            if (c < R.root_value) dst[c] = last[c];
                        dst[R.root_value] = root_value;
                        dst[R.done] = 1.0;
                    }
                }
                ep_start = t + 1;
                env.episode += 1;
                int g_reset = g;
                asm volatile("" : "+v"(g_reset));   // (as `ns` above: the reset's key is formed when an episode ends)
                Env::reset(env, P.env_seed, g_reset);
            }
            env_observe(env);
            env_store(env, ep_start);
        }
        MZ_TICK(14);
    }
#ifdef RZ_MZ_PROFILE
    if (blockIdx.x == 0 && tid == 0)
        for (int i = 0; i < 16; ++i) mz_prof[i] = prof_acc[i];
#endif
    if (lead) {
        E.top[g] = top;
        E.vmin[g] = lo;
        E.vmax[g] = hi;
        E.depth[g] = depth;
        if (MOVES) {
#pragma unroll
            for (int i = 0; i < KS; ++i) P.state[KS * g + i] = env_g[i];
            P.steps[g] = __double_as_longlong(env_g[KS]);
            P.episode[g] = __double_as_longlong(env_g[KS + 1]);
            P.ep_start[g] = __double_as_longlong(env_g[KS + 2]);
        }
    }
    if (TREE_LDS) {
        __syncthreads();
        if (w == 0 && (GUMBEL ? q == 0 : ca == 0)) Gleaf[te] = top;   // (every wave needs the final tops)
        __syncthreads();
        for (int ee = 0; ee < gpw && g0 + ee < E.n_games; ++ee) {
            MzNode *dst = E.nodes + (long long)(g0 + ee) * E.cap;
            const int used = Gleaf[ee];
            for (int i = tid; i < used; i += 64 * kMzWaves) {
                const MzHot h = TREE[ee * tcap + i];
                dst[i] = MzNode{h.N, h.first_child, h.value_sum, h.prior, REW[ee * tcap + i], GUMBEL ? __float_as_int(VH[ee * tcap + i]) : 0};
            }
        }
    }
}

}  // namespace
