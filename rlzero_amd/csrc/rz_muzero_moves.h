// rz_muzero_moves.h -- moves kept on the device, generic over the environment: k_mz_env_step, k_mz_env_move (MzEnvPlay), k_mz_root_noise.
// The layer between a finished search and the replay -- action draw, environment step, record, hand-over of finished episodes --
// as launches of their own behind rz_mz_search (k_mz_search is not involved: its MOVES stages are the other route, under the same rules).
// An environment is a trait (rz_mz_env.h); k_mz_env_step and k_mz_env_move are instantiated once per kind.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rz_muzero_noise.h"
#include "rz_muzero_tree.h"
#include "rz_mz_env.h"
#include "rz_mz_pack.h"

#pragma clang fp contract(off)

namespace {

using rzmp::kMzMaxA;   // the most actions the root noise serves: the fused search's limit

// one step of every environment with auto-reset; actions == nullptr: no step, the observation only
template <typename Env>
__global__ __launch_bounds__(128) void k_mz_env_step(double *state, long long *steps, long long *episode, const long long *actions, int n_envs,
                              unsigned long long seed, long long max_episode_steps, float *obs, float *reward, uint8_t *terminated,
                              uint8_t *truncated) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_envs) return;
    typename Env::State c;
    Env::load(c, state + (long long)Env::kState * g, steps[g], episode[g]);
    if (actions != nullptr) {
        long long a = actions[g];
        a = a < 0 ? 0 : (a >= Env::kActions ? Env::kActions - 1 : a);
        double r = 0.0;
        const int done = Env::step(c, (int)a, max_episode_steps, &r);
        if (done) {
            c.episode += 1;
            Env::reset(c, seed, g);
        }
        Env::store(c, state + (long long)Env::kState * g);
        steps[g] = c.steps;
        episode[g] = c.episode;
        reward[g] = (float)r;
        terminated[g] = (uint8_t)(done & RZ_MZE_TERMINATED ? 1 : 0);
        truncated[g] = (uint8_t)(done & RZ_MZE_TRUNCATED ? 1 : 0);
    }
    float o[Env::kObs];
    Env::observe(c, o);
#pragma unroll
    for (int i = 0; i < Env::kObs; ++i) obs[(long long)Env::kObs * g + i] = o[i];
}

struct MzEnvPlay {      // rz_mz_env_move: MzPlay's history (same layout of ring, arena, entries, counters) around ONE move
    double *state;                          // [G][kState]
    long long *steps, *episode, *ep_start;  // [G]
    unsigned long long env_seed, noise_seed;
    double inv_temperature;                 // <= 0: the first maximum of the visit counts
    long long max_episode_steps;
    double *ring;                           // [G][hist][row]
    int hist;
    long long t;                            // global step index of this move
    double *arena;                          // [arena_rows][row]
    long long arena_rows;
    long long *counters, *entries;          // [4]; [max_entries][4]
    long long max_entries;
    float *obs;                             // [G][kObs]: the observation the next search starts from
};

// the move behind a finished search: what the MOVES stage of k_mz_search does at "the move", from the tree in HBM; a thread per
// environment.  Plain stores and the two counters' atomics; a finished episode's earlier records were written by earlier launches.
template <typename Env>
__global__ __launch_bounds__(128) void k_mz_env_move(MzDev E, MzEnvPlay P) {
    constexpr int D = Env::kObs, A = Env::kActions;
    constexpr rzmze::RecordLayout R = rzmze::record_layout(D, A);
    constexpr int ROW = R.row;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    const MzNode *nodes = E.nodes + (long long)g * E.cap;
    const MzNode root = nodes[0];
    const bool grown = root.first_child >= 1 && root.first_child + A <= E.cap;
    int visits[A];
#pragma unroll
    for (int a = 0; a < A; ++a) visits[a] = grown ? nodes[root.first_child + a].N : 0;
    typename Env::State env;
    Env::load(env, P.state + (long long)Env::kState * g, P.steps[g], P.episode[g]);
    long long ep_start = P.ep_start[g];
    // 1, 2: the weights and the draw
    double wgt[A], total;
    int action = rzmze::move_weights(visits, A, P.inv_temperature, wgt, &total);
    if (P.inv_temperature > 0.0)
        action = rzmze::move_draw(wgt, A, total, rzmze::move_key(P.noise_seed, 0xA5A5A5A5ull, g, env.episode, env.steps));
    // 3, 4: the record (the observation is the one the search started from) and the step
    double rec[ROW];
    {
        float o[D];
        Env::observe(env, o);
#pragma unroll
        for (int i = 0; i < D; ++i) rec[i] = (double)o[i];
    }
    double reward = 0.0;
    const int done = Env::step(env, action, P.max_episode_steps, &reward);
    rec[R.action] = (double)action;
    rec[R.reward] = reward;
#pragma unroll
    for (int a = 0; a < A; ++a) rec[R.visits + a] = (double)visits[a];
    rec[R.root_value] = root.value_sum / (double)(root.N > 1 ? root.N : 1);
    rec[R.done] = done ? 1.0 : 0.0;
    double *ring_g = P.ring + (long long)g * P.hist * ROW;
    {
        double *dst = ring_g + (P.t % P.hist) * ROW;
#pragma unroll
        for (int c = 0; c < ROW; ++c) dst[c] = rec[c];
    }
    if (done) {
        // 5: the episode's records as one run in the arena, its entry, the next episode
        long long len = P.t + 1 - ep_start;
        const long long most = P.t + 1 < P.hist ? P.t + 1 : P.hist;
        len = len < 1 ? 1 : (len > most ? most : len);   // (an episode longer than the ring cannot be: rz_mz_env_move sizes it)
        const long long off = mz_claim_episode<true>(P.counters, P.arena_rows, P.entries, P.max_entries, g, P.t + 1, len);
        if (off >= 0) {
            for (long long j = 0; j < len - 1; ++j) {
                const double *src = ring_g + ((P.t + 1 - len + j) % P.hist) * ROW;
                double *dst = P.arena + (off + j) * ROW;
#pragma unroll
                for (int c = 0; c < ROW; ++c) dst[c] = src[c];
            }
            double *dst = P.arena + (off + len - 1) * ROW;
#pragma unroll
            for (int c = 0; c < ROW; ++c) dst[c] = rec[c];
        }
        ep_start = P.t + 1;
        env.episode += 1;
        Env::reset(env, P.env_seed, g);
    }
    // 6, 7: the state and the next observation
    Env::store(env, P.state + (long long)Env::kState * g);
    P.steps[g] = env.steps;
    P.episode[g] = env.episode;
    P.ep_start[g] = ep_start;
    float o[D];
    Env::observe(env, o);
#pragma unroll
    for (int i = 0; i < D; ++i) P.obs[(long long)D * g + i] = o[i];
}

// the normalised root noise of a move, eta [G][A], under the whole moves' key (noise_seed, g, episode, steps): mz_root_gammas as
// k_mz_search's MOVES stage calls it, in the form k_mz_init takes
__global__ void k_mz_root_noise(int n_games, int n_actions, const long long *episode, const long long *steps, unsigned long long noise_seed,
                                float alpha, double *eta) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_games) return;
    float gam[kMzMaxA];
    const double gsum = mz_root_gammas(alpha, rzmze::move_key(noise_seed, 0ull, g, episode[g], steps[g]), n_actions, gam);
#pragma unroll
    for (int a = 0; a < kMzMaxA; ++a)
        if (a < n_actions) eta[(long long)g * n_actions + a] = (double)gam[a] / gsum;
}

}  // namespace
