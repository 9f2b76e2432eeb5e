// rz_engine_roots.h -- what rz_engine.hip reads from and does to the roots: the root readers (k_root_children, k_root_stats,
// k_root_values), tree reuse (fresh_root, advance_body, k_advance), the game step (step_body, k_step_games) and the small kernels that
// set or copy per-game state (k_set_roots, k_get_roots, k_get_leaves, k_set_noise_keys, k_set_active, k_encode, k_uct_scores).
// advance_body, step_body and fresh_root are also the device move step's (rz_engine_play.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "rlzero_hip.h"
#include "rz_tree.h"

namespace {

using namespace rzt;   // rz_tree.h: Dev, the record accessors and the bitboard rules

// ------------------------------------------------------------------ root read-out
// what: 0 = visits (int32), 1 = W (double), 2 = prior (float); output [n_games][A] by action
__global__ __launch_bounds__(kWave) void k_root_children(Dev E, int what, void *out) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const int arena = E.cur_arena[g];
    const int4 *R = arena_records(E, g, arena);
    const float *P = arena_priors(E, g, arena);
    uint64_t st[2][kWords], occ[kWords];
    load_board(E.root_stones, g, st);
#pragma unroll
    for (int j = 0; j < kWords; ++j) occ[j] = st[0][j] | st[1][j];
    const Legal L = legal_of(E, occ, lane);
    const int4 lo = R[0], hi = R[1];
    const bool expanded = rec_k(lo) > 0;
    const int fc = lo.y;
    const int nv = expanded ? lo.z : 0;
    int before = 0;
#pragma unroll
    for (int j = 0; j < kWords; ++j) {
        const int r = lane_action_rank(E, occ, L, j, lane, before);
        const int a = 64 * j + lane;
        if (a >= E.A) continue;
        const bool seen = r >= 0 && r < nv;
        const long long o = (long long)g * E.A + a;
        if (what == 0) ((int32_t *)out)[o] = seen ? R[2 * (fc + r)].x : 0;
        else if (what == 1) ((double *)out)[o] = seen ? rec_w(R[2 * (fc + r) + 1]) : 0.0;
        else ((float *)out)[o] = (r >= 0 && expanded) ? P[hi.z + r] : 0.0f;
    }
}

__global__ void k_root_stats(Dev E, int32_t *n, double *w) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    const int4 *R = arena_records(E, g, E.cur_arena[g]);
    n[g] = R[0].x;
    w[g] = rec_w(R[1]);
}

// {v_root, q_best} per game (rz_root_values): -W / N of the root, max W / N over the root's children with N > 0; NaN where undefined
__global__ __launch_bounds__(kWave) void k_root_values(Dev E, double *out) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const int4 *R = arena_records(E, g, E.cur_arena[g]);
    const int4 lo = R[0];
    const int fc = lo.y;
    const int nv = rec_k(lo) > 0 ? lo.z : 0;
    double qb = -INFINITY;
    for (int r = lane; r < nv; r += kWave) {   // (visited child records: fc .. fc + nv, in rank order; the maximum needs no order)
        const int n = R[2 * (fc + r)].x;
        if (n > 0) qb = fmax(qb, rec_w(R[2 * (fc + r) + 1]) / (double)n);
    }
    for (int off = 32; off >= 1; off >>= 1) qb = fmax(qb, __shfl_xor(qb, off));
    if (lane == 0) {
        out[2 * (long long)g] = lo.x > 0 ? -(rec_w(R[1]) / (double)lo.x) : NAN;
        out[2 * (long long)g + 1] = qb > -INFINITY ? qb : NAN;
    }
}

// ------------------------------------------------------------------ tree reuse
__device__ __forceinline__ void fresh_root(const Dev &E, int g, int arena, int lane) {
    if (lane == 0) {
        int4 *R = arena_records(E, g, arena);
        R[0] = make_int4(0, -1, 0, 0);
        R[1] = make_hi(0.0, -1, 1.0f);  // TreeNode(None, 1.0), alphazero_mcts.py:35,103
        E.cur_arena[g] = arena;
        E.top[g] = 1;
        E.ptop[g] = 0;
        E.nblk[g] = 0;
    }
}

// AlphaZeroMCTS.update_with_move (alphazero_mcts.py:96-103).  The kept subtree is copied
// breadth-first into the game's other arena (per expanded node: its prior block, and the visited
// prefix of its child records into a block of the same capacity), which also recycles the slots
// of the discarded siblings and of every outgrown child block.  A copied record keeps its SOURCE
// first-child / prior-block offsets until the node itself is taken from the queue, so the queue
// holds destination slots only.
__device__ __forceinline__ void advance_body(const Dev &E, int g, int lane, int mv) {
    if (mv == -2) return;
    const int src_arena = E.cur_arena[g], dst_arena = src_arena ^ 1;
    const int4 *Rs = arena_records(E, g, src_arena);
    int4 *Rd = arena_records(E, g, dst_arena);
    const float *Ps = arena_priors(E, g, src_arena);
    float *Pd = arena_priors(E, g, dst_arena);
    if (mv < 0) {
        if (mv != -1) flag(E, g, RZ_FLAG_ILLEGAL_MOVE, lane);
        fresh_root(E, g, dst_arena, lane);
        return;
    }
    uint64_t st[2][kWords], occ[kWords];
    load_board(E.root_stones, g, st);
#pragma unroll
    for (int j = 0; j < kWords; ++j) occ[j] = st[0][j] | st[1][j];
    const Legal L = legal_of(E, occ, lane);
    int rank = 0, cell = 0;
    if (!locate_action(E, occ, L, mv, rank, cell)) {
        flag(E, g, RZ_FLAG_ILLEGAL_MOVE, lane);
        fresh_root(E, g, dst_arena, lane);
        return;
    }
    const int4 rlo = Rs[0], rhi = Rs[1];
    if (rec_k(rlo) == 0 || rank >= rlo.z) {
        // the chosen child was never visited: it is a TreeNode with N = 0 and no children
        fresh_root(E, g, dst_arena, lane);
        return;
    }
    const int src = rlo.y + rank;
    const int4 slo = Rs[2 * src], shi = Rs[2 * src + 1];
    const float prior = Ps[rhi.z + rank];
    int32_t *queue = E.queue + (long long)g * E.qcap;
    if (lane == 0) {
        Rd[0] = slo;
        Rd[1] = make_int4(shi.x, shi.y, shi.z, __float_as_int(prior));
        queue[0] = 0;
    }
    int q_tail = rec_k(slo) > 0 ? 1 : 0;
    __syncthreads();
    int dtop = 1, dptop = 0, nblk = 0;
    bool full = false;
    for (int q_head = 0; q_head < q_tail; ++q_head) {
        const int dst = queue[q_head];
        const int4 lo = Rd[2 * dst], hi = Rd[2 * dst + 1];
        const int k = rec_k(lo), cap = rec_cap(lo), nv = lo.z, sfc = lo.y, spb = hi.z;
        // the carried subtree must leave room for the n_playout expansions of the coming search
        if ((long long)dptop + k > E.pcap - (long long)(E.n_playout + 1) * E.A ||
            (long long)dtop + cap > E.cap - (long long)(E.n_playout + 1) * 8 - 2 * E.A || nblk >= E.qcap - E.n_playout - 1) {
            full = true;
            break;
        }
        for (int r = lane; r < k; r += kWave) Pd[dptop + r] = Ps[spb + r];
        for (int r0 = 0; r0 < nv; r0 += kWave) {
            const int r = r0 + lane;
            bool expanded = false;
            if (r < nv) {
                const int4 a = Rs[2 * (sfc + r)], b = Rs[2 * (sfc + r) + 1];
                Rd[2 * (dtop + r)] = a;
                Rd[2 * (dtop + r) + 1] = b;
                expanded = rec_k(a) > 0;
            }
            const unsigned long long has = __ballot(expanded);
            if (expanded) {
                const int pos = q_tail + __popcll(has & ((1ull << lane) - 1ull));
                if (pos < E.qcap) queue[pos] = dtop + r;
            }
            q_tail += __popcll(has);
        }
        if (q_tail > E.qcap) {
            full = true;
            break;
        }
        if (lane == 0) {
            Rd[2 * dst] = make_int4(lo.x, cap > 0 ? dtop : -1, nv, lo.w);
            *rec_pb(Rd, dst) = dptop;
        }
        dtop += cap;
        dptop += k;
        nblk += 1;
        __syncthreads();  // records and queue entries written by other lanes are read next iteration
    }
    if (full) {
        // The reference's tree is unbounded; here the kept subtree is limited to qcap - n_playout - 1 expanded nodes
        // (and the prior floats / record slots tested above).  A larger one is DROPPED (the search restarts from a fresh root, like update_with_move(-1)):
        // a deviation from the reference that is counted (rz_stats.reuse_dropped) and flagged per game with the
        // non-fatal RZ_FLAG_REUSE_DROPPED, never silent and never fatal for the rest of the batch.
        if (lane == 0) {
            atomicOr(&E.err[g], RZ_FLAG_REUSE_DROPPED);
            atomicOr(E.err_any, RZ_FLAG_REUSE_DROPPED);   // (rz_stats.error_flags is the OR over the games: this bit too)
            atomicAdd(E.reuse_drops, 1);
        }
        fresh_root(E, g, dst_arena, lane);
        return;
    }
    if (lane == 0) {
        E.cur_arena[g] = dst_arena;
        E.top[g] = dtop;
        E.ptop[g] = dptop;
        E.nblk[g] = nblk;
    }
}

__global__ __launch_bounds__(kWave) void k_advance(Dev E, const int32_t *moves) {
    advance_body(E, blockIdx.x, threadIdx.x, moves[blockIdx.x]);
}

// ------------------------------------------------------------------ game step
// -> the winner (player id or -1) and whether the game is over, wave-uniform
__device__ __forceinline__ void step_body(const Dev &E, int g, int lane, int mv, int &who, bool &over) {
    const int S = E.S;
    uint64_t st[2][kWords];
    load_board(E.root_stones, g, st);
    int to_move = E.root_to_move[g];
    if (mv >= 0) {
        uint64_t occ[kWords];
#pragma unroll
        for (int j = 0; j < kWords; ++j) occ[j] = st[0][j] | st[1][j];
        const Legal L = legal_of(E, occ, lane);
        int rank = 0, cell = 0;
        if (!locate_action(E, occ, L, mv, rank, cell)) {
            flag(E, g, RZ_FLAG_ILLEGAL_MOVE, lane);
        } else {
            if (to_move == 0) set_bit(st[0], cell); else set_bit(st[1], cell);
            to_move ^= 1;
            if (lane == 0) {
                E.root_to_move[g] = to_move;
                E.root_last[g] = cell;
            }
            store_board(E.root_stones, g, st, lane);
        }
    }
    who = -1;
    if (line_anywhere(st[0], S, E.BH, E.BW, E.n_row, lane, E.bw_rcp)) who = 0;
    else if (line_anywhere(st[1], S, E.BH, E.BW, E.n_row, lane, E.bw_rcp)) who = 1;
    over = who >= 0 || count_bits(st[0]) + count_bits(st[1]) == S;
}

__global__ __launch_bounds__(kWave) void k_step_games(Dev E, const int32_t *moves, int32_t *winner,
                                                      uint8_t *ended) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    int who = -1;
    bool over = false;
    step_body(E, g, lane, moves[g], who, over);
    if (lane == 0) {
        if (winner) winner[g] = who;
        if (ended) ended[g] = over ? 1 : 0;
    }
}

__global__ void k_set_roots(Dev E, const uint64_t *stones, const int32_t *to_move,
                            const int32_t *last_move, const uint8_t *mask, int reset_trees) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    if (mask != nullptr && !mask[g]) return;
    for (int j = 0; j < 2 * kWords; ++j) {
        const uint64_t v = stones[(long long)g * 2 * kWords + j];
        E.root_stones[(long long)g * 2 * kWords + j] = v & E.valid[j % kWords];
    }
    E.root_to_move[g] = to_move[g] & 1;
    E.root_last[g] = last_move[g];
    if (reset_trees) fresh_root(E, g, E.cur_arena[g], 0);
}

__global__ void k_get_roots(Dev E, uint64_t *stones, int32_t *to_move, int32_t *last_move) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    for (int j = 0; j < 2 * kWords; ++j)
        stones[(long long)g * 2 * kWords + j] = E.root_stones[(long long)g * 2 * kWords + j];
    to_move[g] = E.root_to_move[g];
    last_move[g] = E.root_last[g];
}

__global__ void k_get_leaves(Dev E, uint64_t *stones, int32_t *to_move, int32_t *last_move,
                             int32_t *terminal) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    for (int j = 0; j < 2 * kWords; ++j)
        stones[(long long)g * 2 * kWords + j] = E.leaf_stones[(long long)g * 2 * kWords + j];
    to_move[g] = E.leaf_to_move[g];
    last_move[g] = E.leaf_last[g];
    terminal[g] = E.leaf_term[g];
}

// keys == nullptr: the default keys (noise_seed ^ game << 20) for the selected games
__global__ void k_set_noise_keys(Dev E, const uint64_t *keys, const uint8_t *mask) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games || (mask != nullptr && !mask[g])) return;
    E.noise_key[g] = keys != nullptr ? keys[g] : (E.noise_seed ^ ((uint64_t)g << 20));
    E.noise_ctr[g] = 0;
}

__global__ void k_set_active(Dev E, const uint8_t *active) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < E.n_games) E.active[g] = active ? (active[g] ? 1 : 0) : 1;
}

// which: 0 = leaf boards, 1 = root boards
__global__ __launch_bounds__(kWave) void k_encode(Dev E, int which, float *obs) {
    const int g = blockIdx.x;  // which == 0: leaf index (game * K + slot); which == 1: game
    const int lane = threadIdx.x;
    uint64_t st[2][kWords];
    load_board(which == 0 ? E.leaf_stones : E.root_stones, g, st);
    const int to_move = which == 0 ? E.leaf_to_move[g] : E.root_to_move[g];
    const int last = which == 0 ? E.leaf_last[g] : E.root_last[g];
    const int nst = count_bits(st[0]) + count_bits(st[1]);
    write_obs(obs + (long long)g * 4 * E.S, to_move == 0 ? st[0] : st[1],
              to_move == 0 ? st[1] : st[0], last, nst, E.S, lane);
}

__global__ void k_uct_scores(const double *w, const int32_t *n, const int32_t *np, double c,
                             const double *logtab, long long logtab_n, double *out, long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int pn = np[i];
    if (pn == 0 || n[i] == 0 || pn >= logtab_n) {
        out[i] = INFINITY;
        return;
    }
    out[i] = uct_ref(w[i], n[i], logtab[pn], c);
}

}  // namespace
