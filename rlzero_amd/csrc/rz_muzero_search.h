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
//   * TREE_LDS trees use their own record: MzHot (N, first_child, value_sum, prior and q = reward + discount * value(),
//     refreshed by the backup that changes it, so the walk does not divide value_sum / N again at every visit) plus one
//     float of reward per node; sqrt(N) of the walk comes from a table filled with the same IEEE sqrt.  Same operations on
//     the same operands as mz_descend / mz_grow_backup: same bits (tests: fused search == step-by-step == CPython).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rlzero_hip.h"
#include "rz_muzero_hot.h"
#include "rz_muzero_noise.h"
#include "rz_muzero_tree.h"
#include "rz_mz_env.h"
#include "rz_mz_pack.h"
#include "rz_mz_value.h"

#pragma clang fp contract(off)

namespace {

using rzmp::kMzH, rzmp::kMzMaxA, rzmp::kMzObs;   // the model's sizes: defined once, beside the packing of its weights
constexpr int kMzWaves = 4, kMzTile = 16, kMzKX = kMzH + kMzMaxA, kMzMaxGpw = 16;
constexpr int kMzRedRows = 4 + kMzMaxA;   // min, max, reward, value, logits
constexpr int kMzHeadRows = 2 + kMzMaxA;  // rew2, val, pol rows
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
__host__ __device__ inline int mz_search_lds_bytes(int gpw, int cap, int path_stride, int n_sims_cfg, bool tree_lds, int w1_cols) {
    int bytes = mz_search_fixed_floats(w1_cols) * 4 + gpw * path_stride * 4;
    bytes = (bytes + 15) / 16 * 16;
    bytes += 2 * (((n_sims_cfg + 2) * 8 + 15) / 16 * 16);   // log and sqrt tables
    if (tree_lds) bytes += gpw * (cap + 1) * (int)sizeof(MzHot) + (gpw * (cap + 1) * 4 + 15) / 16 * 16;   // records (+ a spare per game) + rewards
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
template <bool TREE_LDS, bool MOVES, typename Env = rzmze::EnvCartPole, int MAXA = (MOVES ? Env::kActions : kMzMaxA), bool VT = false>
__global__ __launch_bounds__(64 * kMzWaves, 2) void k_mz_search(MzDev E, MzModel M, float *hidden, int n_sims, int gpw, MzTrace T, MzPlay P) {
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
    if (tid == 0) {
        HB[0] = M.rew2_b[0];
        HB[1] = M.val_b[0];
    }
    if (tid < A) HB[2 + tid] = M.pol_b[tid];
    for (int i = tid; i < kMzHeadRows * kMzH; i += 64 * kMzWaves) {
        const int row = i >> 6, k = i & 63;
        HW[i] = row == 0 ? M.rew2_w[k] : row == 1 ? M.val_w[k] : row - 2 < A ? M.pol_w[(row - 2) * kMzH + k] : 0.0f;
    }
    for (int i = tid; i < kMzKX * kMzTile; i += 64 * kMzWaves) XS[i] = 0.0f;   // (the padding rows 64 + A .. 71 stay zero)
    for (int i = tid; i < kMzObs * kMzTile; i += 64 * kMzWaves) OBS[i] = 0.0f;
    for (int i = tid; i < E.n_sims + 2; i += 64 * kMzWaves) {
        PBL[i] = E.pb_log[i];
        SQT[i] = sqrt((double)i);
    }
    // the trees of this workgroup's games
    // wave 0 walks the trees: the four lanes of quad `ge` own game g0 + ge together -- they score different children in
    // the walk and otherwise run the same tree code on the same values (same LDS words, same bits); `lead` writes to HBM
    const int ge = l >> 2, ca = l & 3;
    const bool mine = w == 0 && ge < gpw && g0 + ge < E.n_games;
    const bool lead = mine && ca == 0;
    const int g = g0 + (ge < gpw ? ge : 0);
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
        } else {
            top = E.top[g];
            lo = E.vmin[g];
            hi = E.vmax[g];
        }
    }
    if (TREE_LDS && !MOVES) {
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
    MzHot *hot = TREE + (ge < gpw ? ge : 0) * tcap;                 // (TREE_LDS)
    float *rew = REW + (ge < gpw ? ge : 0) * tcap;
    int32_t *path = PATH + (ge < gpw ? ge : 0) * E.path_stride;
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
        const float pv = mz_head_partial(p, HW + 1 * kMzH, w, q, l);
        if (q == 0) RED[(3 * kMzWaves + w) * kMzTile + n] = pv;
#pragma unroll
        for (int a = 0; a < MAXA; ++a) {
            if (a < A) {
                const float pl = mz_head_partial(p, HW + (2 + a) * kMzH, w, q, l);
                if (q == 0) RED[((4 + a) * kMzWaves + w) * kMzTile + n] = pl;
            }
        }
    };
    // (lane that owns a game) value and softmax(policy logits) from the partial sums, waves in order
    auto finish_prediction = [&](float &value, float (&probs)[MAXA]) {
        value = HB[1];
#pragma unroll
        for (int u = 0; u < kMzWaves; ++u) value += RED[(3 * kMzWaves + u) * kMzTile + ge];
        float logit[MAXA], mxl = -INFINITY;
#pragma unroll
        for (int a = 0; a < MAXA; ++a) {
            logit[a] = -INFINITY;
            if (a < A) {
                float x = HB[2 + a];
#pragma unroll
                for (int u = 0; u < kMzWaves; ++u) x += RED[((4 + a) * kMzWaves + u) * kMzTile + ge];
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
    for (int sim = 0; sim < n_sims; ++sim) {
        // S0 (wave 0): select, one lane per game; then the gather of the parents' hidden states into XS[k][game]
        // (lane -> game l / 4, four 16-byte pieces of its 256-byte row) and the one-hot action rows
        int par = 0, act = 0, lf = 0;
        if (w == 0) {
            if (mine)
                depth = TREE_LDS ? mz_descend_hot<AFIX>(E, hot, path, PBL, SQT, lo, hi, ca, hidden + (long long)g * E.cap * kMzH, touch_sink, par, act, lf)
                                 : mz_descend(E, nodes, path, PBL, lo, hi, par, act, lf);
            MZ_TICK(0);
#ifdef RZ_MZ_PROFILE
            {   // the wave walks as long as its deepest game
                int md = mine ? depth : 0;
                for (int off = 32; off >= 1; off >>= 1) md = max(md, __shfl_xor(md, off));
                prof_acc[15] += md;
            }
#endif
            if (ca == 0) Gleaf[ge] = lf;
            const int ee = ge, pe = par;   // (the quad of a game also gathers its parent's state: 4 x 64 bytes per lane)
            const bool live_e = mine;
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
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = (l & 3) + 4 * j;
                    const float4 v = live_e ? src[c] : float4{0.0f, 0.0f, 0.0f, 0.0f};
                    XS[(4 * c + 0) * kMzTile + ee] = v.x;
                    XS[(4 * c + 1) * kMzTile + ee] = v.y;
                    XS[(4 * c + 2) * kMzTile + ee] = v.z;
                    XS[(4 * c + 3) * kMzTile + ee] = v.w;
                }
                const int an = __shfl(act, 4 * n);
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
            const float pr = mz_head_partial(r, HW, w, q, l);
            if (q == 0) RED[(2 * kMzWaves + w) * kMzTile + n] = pr;
        }
        MZ_TICK(5);
        __syncthreads();
        MZ_TICK(6);
        // S3: per-sample min-max scaling of the new state, stored for the leaf
        scale_and_store(t);
        MZ_TICK(7);
        __syncthreads();
        MZ_TICK(8);
        // S4: prediction on the new state
        predict_partials();
        MZ_TICK(9);
        __syncthreads();
        MZ_TICK(10);
        // S5 (wave 0): finish the heads, expand + backup
        if (w == 0) {
            float reward = HB[0];
#pragma unroll
            for (int u = 0; u < kMzWaves; ++u) reward += RED[(2 * kMzWaves + u) * kMzTile + ge];
            float value, probs[MAXA];
            finish_prediction(value, probs);
            if constexpr (VT) {   // widened, inverted in fp64, rounded once
                reward = (float)rzmzv::value_h_inv((double)reward);
                value = (float)rzmzv::value_h_inv((double)value);
            }
            MZ_TICK(11);
            if (mine) {
                if (!MOVES && lead && T.reward != nullptr) {
                    const long long o = (long long)sim * E.n_games + g;
                    T.parent[o] = par;
                    T.action[o] = act;
                    T.leaf[o] = lf;
                    T.reward[o] = reward;
                    T.value[o] = value;
#pragma unroll
                    for (int a = 0; a < MAXA; ++a)
                        if (a < A) T.probs[o * A + a] = probs[a];
                }
                if (TREE_LDS) mz_grow_backup_hot<MAXA, AFIX>(E, hot, rew, path, E.cap, ca, depth, top, lo, hi, reward, probs, value);
                else mz_grow_backup<MAXA>(E, nodes, path, depth, top, lo, hi, reward, probs, value);
            }
            MZ_TICK(12);
        }
        // (no barrier: the next select and gather are wave 0's too; XS -- which the gather rewrites -- was last read
        // before the barrier behind S4, and RED, which wave 0 reads above, is rewritten only after the next S0 barrier)
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
        if (w == 0 && ca == 0) Gleaf[ge] = top;   // (every wave needs the final tops)
        __syncthreads();
        for (int ee = 0; ee < gpw && g0 + ee < E.n_games; ++ee) {
            MzNode *dst = E.nodes + (long long)(g0 + ee) * E.cap;
            const int used = Gleaf[ee];
            for (int i = tid; i < used; i += 64 * kMzWaves) {
                const MzHot h = TREE[ee * tcap + i];
                dst[i] = MzNode{h.N, h.first_child, h.value_sum, h.prior, REW[ee * tcap + i], 0};
            }
        }
    }
}

}  // namespace
