// rz_engine_play.h -- the whole device move step of rz_engine.hip (include/rlzero_hip.h: rz_play_*): its device record Play, the draw
// (k_play_draw), policy target pruning (k_root_pruned), the rest of a move (k_play_apply: advance_body and step_body of
// rz_engine_roots.h, the end of a game, the refill) and the kernels behind the step's options -- the playout cap (cap_write,
// k_play_cap, k_play_order), the temperature schedule (TempChunk, k_play_set_temps), matches (k_play_side), resignation
// (k_play_set_resign), the stalled slots' mailbox (k_play_resolve), the queue of game ids (k_play_push), k_play_no_draw and k_play_stop.
// The rules themselves are rz_play.h's and rz_forced.h's, tested on the CPU.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "rlzero_hip.h"
#include "rz_engine_roots.h"
#include "rz_forced.h"
#include "rz_play.h"
#include "rz_tree.h"

namespace {

using namespace rzt;   // rz_tree.h: Dev, the record accessors and the bitboard rules

// ------------------------------------------------------------------ the move step on the device (include/rlzero_hip.h: rz_play_*)
struct Play {
    int64_t *game_id;          // [G] -1: idle
    int32_t *ply, *state;      // state: ry::kIdle, kRunning, kStalled
    int32_t *mailbox;          // [G] the host's move for a stalled slot, -1: none
    int32_t *keep, *stepm;     // [G] the moves of this step (update_with_move / env.step), written by k_play_draw
    int32_t *top_hwm;          // [G] the fullest a game's arena has been at the end of a search (read before update_with_move compacts it)
    int32_t *step_ab;          // [2]: k_play_draw reads [0] and writes [1], k_play_apply reads [1] and writes [0] = [1] + 1
    const int64_t *queue_ids;
    int32_t *queue_ctl;        // [0] head, [1] entries valid
    int32_t *log;
    // per-ply temperature (rz_play_set_temperatures): 1 / T before ply p, padded with its last entry to the board's cell count S,
    // then the stall margin of each ply (rz_play.h: temp_entry)
    const double *inv_t_of;    // [2][S]
    int ring, words;
    uint64_t seed;
    double inv_t, margin;
    double *resign;            // [2] {threshold, disabled_frac} (rz_play_set_resign; NaN threshold: off)
    int resign_on;             // rz_play_set_resign called since rz_play_attach: k_play_draw reads `resign` (else never)
    int temp_on;               // rz_play_set_temperatures called since rz_play_attach: k_play_draw reads `inv_t_of` (else never)
    // playout cap randomization (rz_play_set_cap): a search has n_full simulations when cap_uniform(seed, game id, ply) < p_full,
    // else n_fast
    double *cap;               // [2] {n_fast, p_full} (NaN p_full: off -- every search has n_full)
    int32_t *sims_of;          // [G] simulations of the slot's COMING search (k_play_apply, k_play_cap); read by the resident search
    int32_t *order;            // [G] k_play_order's: the slots with a full search, those with a fast one, the inactive ones
    int n_full;                // the engine's n_playout
    int cap_on;                // rz_play_set_cap called since rz_play_attach: the kernels read `cap` (else never)
    // network-vs-network matches (rz_play_set_match): games 2k and 2k + 1 start from opening k % n_open, share their draw uniforms and
    // are searched from a fresh root by the network whose turn it is (k_play_side); the engine's own copies of the caller's table
    const uint64_t *open_stones;   // [n_open][2][kWords]
    const int32_t *open_to_move, *open_last;   // [n_open]
    int n_open;
    int match_on;              // rz_play_set_match in force: the kernels read the table and the pair's uniform (else never)
    int queue_cap;             // rz_play_queue_ring: queue_ids is a ring of this many entries (0: the linear queue)
};
namespace ry = rzplay;   // rz_play.h: the move step's rules, the record and a slot's decision (tested on the CPU)

// the budget of the slot's coming search (rz_play_set_cap), read by the resident search
__device__ __forceinline__ void cap_write(const Play &Y, int g, int64_t gid, int ply) {
    Y.sims_of[g] = ry::budget(Y.n_full, (int)Y.cap[0], Y.cap[1], Y.seed, (uint64_t)gid, (uint64_t)ply);
}

// One wave per slot: the root's visit counts into the log, then the draw of alphazero_mcts.py:88-92,147-148 in fp64 -- taken only
// when the uniform lies farther than `margin` from both edges of its interval (the host's numpy evaluation is the arbiter).
// In a match (rz_play_set_match) the uniform is the pair's -- (seed, game id >> 1, 2 ply + 1) -- and the move keeps no subtree:
// keep = -1, so k_play_apply starts the next search of the game from a fresh root; stepm stays the move.
// The kernel gathers the counts and computes log, the wave maximum and exp; the draw, the resignation rule and what the step
// changes are rz_play.h's (ry::draw, ry::resign_rule, ry::decide), and lane 0 writes all of it at the end.
// `vring` (rz_play_set_root_values; nullptr: off, nothing more is read or written): float32 [Y.ring][n_games], the root value the
// mover's search saw (ry::root_value: rz_root_values' [0]) into the row of this step for every slot that holds a game -- a stalled
// slot's root does not change, so its rows repeat the searched one's value --, NaN for an idle slot.
__global__ __launch_bounds__(kWave) void k_play_draw(Dev E, Play Y, float *__restrict__ vring) {
    __shared__ double sh_e[kWave * kWords];
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const int step = Y.step_ab[0];
    if (g == 0 && lane == 0) Y.step_ab[1] = step;
    int32_t *rec = Y.log + ((long long)(step % Y.ring) * E.n_games + g) * Y.words;
    ry::SlotIn in = {};
    in.state = Y.state[g];
    double v_root = NAN;
    if (in.state != ry::kIdle) {
        // the root's children by action (k_root_children)
        const int arena = E.cur_arena[g];
        const int4 *R = arena_records(E, g, arena);
        uint64_t st[2][kWords], occ[kWords];
        load_board(E.root_stones, g, st);
#pragma unroll
        for (int j = 0; j < kWords; ++j) occ[j] = st[0][j] | st[1][j];
        const Legal L = legal_of(E, occ, lane);
        const int4 lo = R[0];
        if (vring != nullptr) v_root = ry::root_value(lo.x, rec_w(R[1]));
        const bool expanded = rec_k(lo) > 0;
        const int fc = lo.y;
        const int nv = expanded ? lo.z : 0;
        int before = 0;
        int cnt[kWords];
        bool legal[kWords];
        double x[kWords];
        double mx = -INFINITY;
        // the ply's temperature (rz_play_set_temperatures): the table is read only once it has been set; a stalled slot keeps its ply,
        // so its move is judged at the same T
        const int ply = Y.ply[g];
        const int tp = ply < 0 ? 0 : (ply < E.S ? ply : E.S - 1);   // (ply < S always holds)
        const double inv_t = Y.temp_on ? Y.inv_t_of[tp] : Y.inv_t;
        const double margin = Y.temp_on ? Y.inv_t_of[E.S + tp] : Y.margin;
        // resignation (rz_play_set_resign): read only once it has been configured -- the rule-free path has no extra memory traffic
        const double thr = Y.resign_on ? Y.resign[0] : NAN;
        const bool rs = !isnan(thr) && in.state == ry::kRunning;
        double qb = -INFINITY;   // max W / N over the visited children (rz_root_values)
#pragma unroll
        for (int j = 0; j < kWords; ++j) {
            const int r = lane_action_rank(E, occ, L, j, lane, before);
            const int a = 64 * j + lane;
            legal[j] = a < E.A && r >= 0;
            cnt[j] = (legal[j] && r < nv) ? R[2 * (fc + r)].x : 0;
            if (a < E.A) rec[RZ_PLAY_RECORD_WORDS + a] = legal[j] ? cnt[j] : -1;
            x[j] = legal[j] ? inv_t * log((double)cnt[j] + 1e-10) : -INFINITY;   // alphazero_mcts.py:91
            mx = fmax(mx, x[j]);
            if (rs && cnt[j] > 0) qb = fmax(qb, rec_w(R[2 * (fc + r) + 1]) / (double)cnt[j]);
        }
        const uint64_t gid = (uint64_t)Y.game_id[g];
        in.game = (int64_t)gid;
        in.ply = ply;
        in.root_n = lo.x;
        in.match = Y.match_on != 0;
        if (in.state == ry::kStalled) {
            in.mail = Y.mailbox[g];
        } else {
            // wave maximum of x (doubles: two 32-bit halves through the shuffle)
            for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
#pragma unroll
            for (int j = 0; j < kWords; ++j) sh_e[64 * j + lane] = legal[j] ? exp(x[j] - mx) : 0.0;   // :12
            if (rs)
                for (int off = 32; off >= 1; off >>= 1) qb = fmax(qb, __shfl_xor(qb, off));
            __syncthreads();
            if (lane == 0) {
                // (rz_play_set_cap: the budget of the search behind this record -- what k_play_apply / k_play_cap wrote into sims_of)
                in.full = Y.cap_on ? ry::full_flag(Y.cap[1], Y.seed, gid, (uint64_t)ply) : 0;
                in.resign_on = rs;
                if (rs) {
                    in.resign = ry::resign_rule(lo.x, rec_w(R[1]), qb, thr);
                    in.calibration = ry::resign_uniform(Y.seed, gid) < Y.resign[1];
                }
                if (ry::needs_draw(in)) {
                    const double u = in.match ? ry::match_uniform(Y.seed, gid, (uint64_t)ply) : ry::move_uniform(Y.seed, gid, (uint64_t)ply);
                    in.draw = ry::draw(sh_e, E.A, u, margin);
                }
            }
        }
    }
    if (lane != 0) return;
    const ry::SlotOut o = ry::decide(in);
    ry::write_record(rec, in, o);
    if (vring != nullptr) vring[(long long)(step % Y.ring) * E.n_games + g] = (float)v_root;
    Y.keep[g] = o.keep;
    Y.stepm[g] = o.stepm;
    if (o.clear_mail) Y.mailbox[g] = -1;
    if (o.state != in.state) Y.state[g] = o.state;
    if (o.ply != in.ply) Y.ply[g] = o.ply;
    if (o.active >= 0) E.active[g] = (uint8_t)o.active;
}

// Policy target pruning (rz_forced.h; rz_root_pruned_visits, rz_play_set_pruned_visits), one wave per game: the root's children by
// action exactly as k_play_draw gathers them, their priors from P[pb + r]; the best child -- the first with the largest count, found
// with the selection's first-maximum vote over (count, action) -- keeps its count, every other visited child gets rzf::pruned_child
// against the best child's PUCT.  int32 [A] per game: the pruned count of a legal action, -1 of an illegal one.  forced_k == 0: the
// raw counts.  `ring` != 0 (the launch in front of k_play_draw): the row of this move step in the side ring [Y.ring][G][A], -1 all
// over for an idle slot; a stalled slot's root has not changed, so its rows repeat the searched one.  ring == 0: row g of [G][A].
__global__ __launch_bounds__(kWave) void k_root_pruned(Dev E, Play Y, int32_t *__restrict__ out, int ring) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    int32_t *row = out + (long long)g * E.A;
    bool idle = false;
    if (ring) {
        row += (long long)(Y.step_ab[0] % Y.ring) * E.n_games * E.A;
        idle = Y.state[g] == ry::kIdle;
    }
    if (idle) {
        for (int a = lane; a < E.A; a += kWave) row[a] = -1;
        return;
    }
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
    const int fc = lo.y, pb = hi.z;
    const int nv = expanded ? lo.z : 0;
    const double k = E.forced_k;
    const bool prune = k > 0.0 && pb >= 0;
    int before = 0;
    int cnt[kWords];
    bool legal[kWords];
    double w[kWords];
    float p[kWords];
    // the lane's own best child: the first of its (up to four) actions with the largest count
    double best = -INFINITY, bw = 0.0;
    int besti = 0x7fffffff, bn = 0;
    float bp = 0.0f;
#pragma unroll
    for (int j = 0; j < kWords; ++j) {
        const int r = lane_action_rank(E, occ, L, j, lane, before);
        const int a = 64 * j + lane;
        legal[j] = a < E.A && r >= 0;
        const bool seen = legal[j] && r < nv;
        cnt[j] = seen ? R[2 * (fc + r)].x : 0;
        w[j] = seen ? rec_w(R[2 * (fc + r) + 1]) : 0.0;
        p[j] = seen && prune ? P[pb + r] : 0.0f;
        if (legal[j] && (double)cnt[j] > best) {
            best = (double)cnt[j];
            besti = a;
            bw = w[j];
            bn = cnt[j];
            bp = p[j];
        }
    }
    const int bi = __builtin_amdgcn_readfirstlane(wave_first_max(best, besti));
    double s_best = 0.0;
    if (bi != 0x7fffffff) {   // (a root without a legal action has no best child: its row is -1 all over)
        const int l = bi & 63;
        const long long wb = __double_as_longlong(bw);
        const double w_best = __hiloint2double(__builtin_amdgcn_readlane((int)(wb >> 32), l), __builtin_amdgcn_readlane((int)wb, l));
        const int n_best = __builtin_amdgcn_readlane(bn, l);
        const float p_best = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bp), l));
        s_best = rzf::puct(w_best, n_best, p_best, sqrt((double)lo.x), E.c_puct);
    }
#pragma unroll
    for (int j = 0; j < kWords; ++j) {
        const int a = 64 * j + lane;
        if (a >= E.A) continue;
        int m = -1;
        if (legal[j]) m = (!prune || a == bi) ? cnt[j] : rzf::pruned_child(cnt[j], w[j], p[j], lo.x, sqrt((double)lo.x), k, E.c_puct, s_best);
        row[a] = m;
    }
}

// The rest of a move in ONE launch, one wave per slot: update_with_move with the move just drawn (advance_body: before the board
// changes), env.step + game_end_winner (step_body), then the end of a finished game (reset_player, game.py:128) and the refill of an
// idle slot from the queue of game ids (GomokuEnv.reset, gomoku_env.py:33-47: empty board, player 0; a fresh tree; the game's
// noise key; in a match -- rz_play_set_match -- the opening of the game's pair instead of the empty board).  drawn == 0 (no
// k_play_draw before it): only the refill.  The pending-priors counter of the game restarts here
// (the flush of the move's search ran just before: rz_deferred_flush leaves its own reset launch out between draw and apply).
__global__ __launch_bounds__(kWave) void k_play_apply(Dev E, Play Y, int drawn) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int step = Y.step_ab[1];
    if (g == 0 && lane == 0) Y.step_ab[0] = step + 1;
    const int keep = drawn ? Y.keep[g] : -2, mv = drawn ? Y.stepm[g] : -1;
    int state = Y.state[g];
    if (lane == 0 && drawn) {   // (rz_get_stats: after the move the arena holds the kept subtree only)
        const int top = E.top[g];
        if (top > Y.top_hwm[g]) Y.top_hwm[g] = top;
    }
    advance_body(E, g, lane, keep);
    __syncthreads();
    int who = -1;
    bool over = false;
    if (mv >= 0) step_body(E, g, lane, mv, who, over);   // (idle and stalled slots make no move)
    if (lane != 0) return;
    if (drawn && E.pend != nullptr) E.pend[g] = 0;
    if (state == ry::kRunning && ((mv >= 0 && over) || mv == ry::kStepResign)) {
        int32_t *rec = Y.log + ((long long)(step % Y.ring) * E.n_games + g) * Y.words;
        if (mv >= 0) rec[ry::kRecFlags] |= ry::ended_flags(who);   // (a resignation's record is complete: k_play_draw)
        state = ry::kIdle;
        Y.state[g] = state;
        Y.game_id[g] = -1;
        E.active[g] = 0;
        fresh_root(E, g, E.cur_arena[g], 0);
    }
    Y.stepm[g] = -1;
    Y.keep[g] = -2;
    if (state != ry::kIdle) {
        // the budget of the slot's coming search (a stalled slot is not searched; k_play_draw has counted the ply already)
        if (Y.cap_on && state == ry::kRunning) cap_write(Y, g, Y.game_id[g], Y.ply[g]);
        return;
    }
    int head = Y.queue_ctl[0];
    int64_t gid = -1;
    while (head < Y.queue_ctl[1]) {
        const int seen = atomicCAS(&Y.queue_ctl[0], head, head + 1);
        if (seen == head) {
            gid = Y.queue_ids[ry::queue_slot(head, Y.queue_cap)];
            break;
        }
        head = seen;
    }
    if (gid < 0) return;
    Y.game_id[g] = gid;
    Y.ply[g] = 0;
    Y.state[g] = ry::kRunning;
    Y.mailbox[g] = -1;
    if (Y.match_on) {   // the pair's opening; plies count from it
        const long long o = (long long)((gid >> 1) % Y.n_open);
        for (int j = 0; j < 2 * kWords; ++j) E.root_stones[(long long)g * 2 * kWords + j] = Y.open_stones[o * 2 * kWords + j] & E.valid[j % kWords];
        E.root_to_move[g] = Y.open_to_move[o] & 1;
        E.root_last[g] = Y.open_last[o];
    } else {
        for (int j = 0; j < 2 * kWords; ++j) E.root_stones[(long long)g * 2 * kWords + j] = 0ull;
        E.root_to_move[g] = 0;
        E.root_last[g] = -1;
    }
    fresh_root(E, g, E.cur_arena[g], 0);
    E.noise_key[g] = ry::noise_key(Y.seed, (uint64_t)gid);
    E.noise_ctr[g] = 0;
    E.active[g] = 1;
    if (Y.cap_on) cap_write(Y, g, gid, 0);
}

// rz_play_set_cap: the rule into its device array, then the budgets of the searches that are coming under it
__global__ void k_play_cap(Dev E, Play Y, double n_fast, double p_full) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    const int64_t gid = Y.game_id[g];
    const int ply = Y.ply[g];
    Y.sims_of[g] = gid < 0 ? Y.n_full : ry::budget(Y.n_full, (int)n_fast, p_full, Y.seed, (uint64_t)gid, (uint64_t)ply);   // (an idle slot: no draw)
    if (g == 0) {
        Y.cap[0] = n_fast;
        Y.cap[1] = p_full;
    }
}

// rz_play_set_temperatures: up to kTempChunk entries of the engine's table (1 / T per ply, then the margins), handed over by value -- a
// write in stream order, so a move graph captured earlier reads the new table from its next replay on
constexpr int kTempChunk = 64;
struct TempChunk {
    double v[kTempChunk];
};
__global__ __launch_bounds__(kTempChunk) void k_play_set_temps(double *inv_t_of, TempChunk c, int base, int count) {
    const int i = threadIdx.x;
    if (i < kTempChunk && base + i < count) inv_t_of[base + i] = c.v[i];
}

// The order of k_delta_res's workgroups under per-game budgets: a STABLE partition of the slots -- full budget (>= n_full), fewer
// simulations, inactive -- so that no full search starts in the last round of a grid of more than two games per CU.  ONE workgroup,
// any number of games in chunks of 256: ballot + mbcnt prefix per wave, the waves' totals through LDS.
__global__ __launch_bounds__(256) void k_play_order(const uint8_t *__restrict__ active, const int32_t *__restrict__ sims_of, int n_full,
                                                    int n_games, int32_t *__restrict__ order) {
    __shared__ int cnt[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int run[3] = {0, 0, 0};   // the next free place of each class (uniform)
    // pass 1: the classes' totals -> where each begins
    int t0 = 0, t1 = 0;
    for (int c0 = 0; c0 < n_games; c0 += 256) {
        const int g = c0 + tid;
        const bool act = g < n_games && active[g] != 0;
        const bool full = act && sims_of[g] >= n_full;
        t0 += __popcll(__ballot(full));
        t1 += __popcll(__ballot(act && !full));
    }
    if (lane == 0) cnt[wave][0] = t0, cnt[wave][1] = t1;
    __syncthreads();
    for (int w = 0; w < 4; ++w) run[1] += cnt[w][0], run[2] += cnt[w][0] + cnt[w][1];
    __syncthreads();
    // pass 2: every slot to its place
    for (int c0 = 0; c0 < n_games; c0 += 256) {
        const int g = c0 + tid;
        const bool act = g < n_games && active[g] != 0;
        const int cls = g >= n_games ? -1 : !act ? 2 : sims_of[g] >= n_full ? 0 : 1;
        int before = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned long long m = __ballot(cls == c);
            const int pre = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
            if (cls == c) before = pre;
            if (lane == 0) cnt[wave][c] = __popcll(m);
        }
        __syncthreads();
        if (cls >= 0) {
            int at = run[cls] + before;
            for (int w = 0; w < wave; ++w) at += cnt[w][cls];
            order[at] = g;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            for (int w = 0; w < 4; ++w) run[c] += cnt[w][c];
        __syncthreads();
    }
}

// rz_play_side: the slots the coming search takes -- the running games whose mover is network `side` (0 = A: player 0 of the even
// game of a pair, player 1 of the odd one).  side < 0: every running game (what k_play_apply leaves; match mode turned off).
__global__ void k_play_side(Dev E, Play Y, int side) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    const bool a_moves = (E.root_to_move[g] == 0) == ((Y.game_id[g] & 1) == 0);
    E.active[g] = (Y.state[g] == ry::kRunning && (side < 0 || side == (a_moves ? 0 : 1))) ? 1 : 0;
}

__global__ void k_play_resolve(Play Y, int slot, int move) { Y.mailbox[slot] = move; }
__global__ void k_play_set_resign(double *resign, double threshold, double disabled_frac) {
    if (threadIdx.x == 0) {
        resign[0] = threshold;
        resign[1] = disabled_frac;
    }
}
// rz_play_queue_push: ids first .. first + count - 1 behind the valid count of the ring, then the count raised -- one workgroup; the ids
// are written, fenced, and only then counted, so a k_play_apply that sees the new count reads them.  A push that would overwrite an
// id no slot has claimed (ry::queue_room) writes nothing and raises RZ_FLAG_QUEUE_FULL.
__global__ __launch_bounds__(256) void k_play_push(Dev E, Play Y, int64_t first, int count) {
    int64_t *ids = const_cast<int64_t *>(Y.queue_ids);
    const int head = Y.queue_ctl[0], valid = Y.queue_ctl[1];
    if (count > ry::queue_room(head, valid, Y.queue_cap)) {
        if (threadIdx.x == 0) {
            atomicOr(&E.err[0], RZ_FLAG_QUEUE_FULL);
            atomicOr(E.err_any, RZ_FLAG_QUEUE_FULL);
        }
        return;
    }
    for (int i = threadIdx.x; i < count; i += blockDim.x) ids[ry::queue_slot(valid + i, Y.queue_cap)] = first + i;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) Y.queue_ctl[1] = valid + count;
}

__global__ void k_play_no_draw(Play Y) { Y.step_ab[1] = Y.step_ab[0]; }   // rz_play_apply without a draw: the step k_play_apply reads

__global__ void k_play_stop(Dev E, Play Y) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.n_games) return;
    Y.state[g] = ry::kIdle;
    Y.game_id[g] = -1;
    Y.mailbox[g] = -1;
    Y.keep[g] = -2;
    Y.stepm[g] = -1;
    E.active[g] = 0;
    fresh_root(E, g, E.cur_arena[g], 0);
}

}  // namespace
