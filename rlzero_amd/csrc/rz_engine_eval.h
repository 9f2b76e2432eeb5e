// rz_engine_eval.h -- the evaluators rz_engine.hip brings itself, one wave per leaf: k_eval_synth (uniform priors, a value that is zero
// or a function of the leaf's stones: the tests' stand-in for a network) and k_eval_rollout (RolloutMCTS's random play-outs).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "rlzero_hip.h"
#include "rz_tree.h"

namespace {

using namespace rzt;   // rz_tree.h: Dev and the bitboard rules

// ------------------------------------------------------------------ synthetic evaluators
__global__ __launch_bounds__(kWave) void k_eval_synth(Dev E, int kind, float *logp, float *value) {
    const int g = blockIdx.x;  // leaf index: game * K + slot (K = 1: the game)
    const int lane = threadIdx.x;
    if (!E.active[g / E.K]) return;
    const int S = E.S;
    uint64_t st[2][kWords];
    load_board(E.leaf_stones, g, st);
    int acc = 0;
#pragma unroll
    for (int j = 0; j < kWords; ++j) {
        const int c = 64 * j + lane;
        if (c < S) {
            const int a = (int)((st[0][j] >> lane) & 1ull), b = (int)((st[1][j] >> lane) & 1ull);
            acc += (c + 1) * (a + 3 * b);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) {
        float v = 0.0f;
        if (kind == RZ_EVAL_VLIN) {
            const int s = acc + 5 * E.leaf_to_move[g];
            v = (float)((s % 17) - 8) / 8.0f;
        }
        value[g] = v;
    }
    if (logp != nullptr) {
        uint64_t occ[kWords];
#pragma unroll
        for (int j = 0; j < kWords; ++j) occ[j] = st[0][j] | st[1][j];
        const Legal L = legal_of(E, occ, lane);
        const float lp = L.k > 0 ? logf(1.0f / (float)L.k) : 0.0f;
        int before = 0;
#pragma unroll
        for (int j = 0; j < kWords; ++j) {
            const int r = lane_action_rank(E, occ, L, j, lane, before);
            const int a = 64 * j + lane;
            if (a < E.A) logp[(long long)g * E.A + a] = r >= 0 ? lp : -INFINITY;
        }
    }
}

// ------------------------------------------------------------------ random rollouts
// RolloutMCTS._evaluate (rlzero/mcts/rollout_mcts.py:49-74): from the leaf play uniformly random
// legal moves (the reference takes the arg-max of k fresh uniforms, :99-100 = a uniform choice)
// until the game ends or n_limit plies, then value = 0 on a tie / limit, else +1 if the winner
// is the player to move AFTER the rollout else -1 (the reference's perspective quirk, :68-72:
// the winner has just moved, so a decisive rollout always yields -1).  The move index of ply p
// is floor(u * k) with u = the high 32 bits of splitmix64(seed, game, sim, ply) -- reproducible
// on the host (rlzero_amd.mcts.rollout_mcts.rollout_pick) so parity tests can drive the checker
// with the very same choices.
__global__ __launch_bounds__(kWave) void k_eval_rollout(Dev E, uint64_t seed, uint32_t sim, int n_limit,
                                                        float *value) {
    const int g = blockIdx.x;  // leaf index: game * K + slot (K = 1: the game)
    const int lane = threadIdx.x;
    if (!E.active[g / E.K]) return;
    const int S = E.S;
    uint64_t st[2][kWords];
    load_board(E.leaf_stones, g, st);
    int to_move = E.leaf_to_move[g];
    int nst = count_bits(st[0]) + count_bits(st[1]);
    int term = E.leaf_term[g];  // 0 running, 1 tie, 2 won by the player who just moved
    int winner = term == 2 ? (to_move ^ 1) : -1;
    const uint64_t key = mix64(mix64(seed ^ (uint64_t)g) ^ (uint64_t)sim);
    for (int ply = 0; ply < n_limit && term == 0; ++ply) {
        uint64_t occ[kWords];
#pragma unroll
        for (int j = 0; j < kWords; ++j) occ[j] = st[0][j] | st[1][j];
        const Legal L = legal_of(E, occ, lane);
        const uint32_t u = (uint32_t)(mix64(key ^ (uint64_t)ply) >> 32);
        const int r = (int)(((uint64_t)u * (uint64_t)L.k) >> 32);
        int action, cell;
        if (!nth_legal(E, occ, L, r, lane, action, cell)) {
            flag(E, g, RZ_FLAG_INTERNAL, lane);
            break;
        }
        if (to_move == 0) set_bit(st[0], cell); else set_bit(st[1], cell);
        nst += 1;
        if (line_through(to_move == 0 ? st[0] : st[1], cell, E.BH, E.BW, E.n_row, lane, E.bw_rcp, E.n_rcp)) {
            term = 2;
            winner = to_move;
        } else if (nst == S) {
            term = 1;
        }
        to_move ^= 1;
    }
    if (lane == 0) value[g] = (winner < 0) ? 0.0f : (winner == to_move ? 1.0f : -1.0f);
}

}  // namespace
