// rz_play.h -- the move step on the device (rz_engine_play.h: k_play_draw, k_play_apply, k_play_cap; include/rlzero_hip.h: rz_play_*):
// everything about it that is neither a kernel launch nor a memory access.  Plain C++, no HIP include, so that the CPU can test it
// against the host's side of the same rules (tests/test_play_host.py: rlzero_amd/selfplay.py and rlzero_amd/playlog.py); the kernels
// and the host entry points call these functions.  Apart from the kernel's own log and exp everything here is integer arithmetic or
// fp64 add, compare and divide: with -ffp-contract=off the host computes the device's bits.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rlzero_hip.h"
#include "rz_rng.h"

#if defined(__HIPCC__)
#define RZY_FN __host__ __device__ __forceinline__
#else
#define RZY_FN inline
#endif

namespace rzplay {

// ---- keyed values: 53 high bits of a splitmix64 chain (rz_rng.h; rlzero_amd/selfplay.py: the same bits)
using rzrng::mix64;
using rzrng::unit;

constexpr uint64_t kResignSalt = 0x72657369676E0000ull;   // "resign": the calibration draw, apart from the move and noise streams
constexpr uint64_t kCapSalt = 0x706C61796F757400ull;      // "playout": the budget draw's own stream
constexpr uint64_t kNoiseSalt = 0x6E6F697365000000ull;    // "noise": a game's Dirichlet noise key

// selfplay.move_uniform(seed, game id, ply)
RZY_FN double move_uniform(uint64_t seed, uint64_t game, uint64_t ply) { return unit(mix64(mix64(mix64(seed) ^ game) ^ ply)); }
// a match (rz_play_set_match): the uniform of the PAIR and of the second of get_action's two draws, alphazero_mcts.py:157
RZY_FN double match_uniform(uint64_t seed, uint64_t game, uint64_t ply) { return move_uniform(seed, game >> 1, 2ull * ply + 1ull); }
// selfplay.resign_uniform(seed, game id): a game is a calibration game (resignation disabled) when it is below disabled_frac
RZY_FN double resign_uniform(uint64_t seed, uint64_t game) { return unit(mix64(mix64(seed ^ kResignSalt) ^ game)); }
// selfplay.cap_uniform(seed, game id, ply): the search before ply `ply` of a game has the full budget when it is below p_full
RZY_FN double cap_uniform(uint64_t seed, uint64_t game, uint64_t ply) { return unit(mix64(mix64(mix64(seed ^ kCapSalt) ^ game) ^ ply)); }
// selfplay.BatchedSelfPlay._start: the key of a game's Dirichlet noise
RZY_FN uint64_t noise_key(uint64_t seed, uint64_t game) { return mix64(mix64(seed ^ kNoiseSalt) ^ game); }

// ---- playout cap randomization (rz_play_set_cap): the budget of the search before ply `ply` of a game.  NaN p_full: the cap is off.
RZY_FN bool full_search(double p_full, uint64_t seed, uint64_t game, uint64_t ply) { return isnan(p_full) || cap_uniform(seed, game, ply) < p_full; }
RZY_FN int budget(int n_full, int n_fast, double p_full, uint64_t seed, uint64_t game, uint64_t ply) {
    return full_search(p_full, seed, game, ply) ? n_full : n_fast;
}
// RZ_PLAY_FULL of the record behind that search: never set without a cap
RZY_FN int full_flag(double p_full, uint64_t seed, uint64_t game, uint64_t ply) {
    return (!isnan(p_full) && full_search(p_full, seed, game, ply)) ? RZ_PLAY_FULL : 0;
}

// ---- temperature: the stall margin at 1 / T -- the configured one if positive, else it follows the temperature
RZY_FN double stall_margin(double configured, double inv_t) { return configured > 0.0 ? configured : 1e-10 * (inv_t > 1.0 ? inv_t : 1.0); }
// entry i of the [2][S] table of rz_play_set_temperatures: 1 / T before ply i (the division on the host) from `temps[0 .. n)` padded with
// its last entry -- n == 0: the temperature of rz_play_attach, `attach_inv_t` --, then the stall margin of every ply
RZY_FN double temp_entry(int i, int S, const double *temps, int n, double attach_inv_t, double margin_configured) {
    const int p = i % S;
    const double inv_t = n == 0 ? attach_inv_t : 1.0 / temps[p < n ? p : n - 1];
    return i < S ? inv_t : stall_margin(margin_configured, inv_t);
}

// ---- the record's header words (include/rlzero_hip.h, "The log: ..."); the visit counts by action follow
enum { kRecGameLo = 0, kRecGameHi = 1, kRecPly = 2, kRecMove = 3, kRecFlags = 4, kRecRootN = 5, kRecEdge = 6, kRecStat = 7 };
static_assert(kRecStat + 1 == RZ_PLAY_RECORD_WORDS, "the header words of a record");
RZY_FN int winner_bits(int winner) { return (winner + 1) << 16; }   // player id, or -1: none / a tie
RZY_FN int32_t float_bits(float v) { return __builtin_bit_cast(int32_t, v); }

// ---- resignation: from N(root), W(root) and the best W / N over the visited children (-inf: none visited), the statistic
// s = max(v_root, q_best) -- NaN when either is missing -- and whether both lie below the threshold (never with a NaN among them)
struct Resign {
    double s;
    bool fire;
};
// the value the mover sees at the root (rz_root_values' [0]; float32 of it is what rz_play_set_root_values logs): NaN at an unvisited root
RZY_FN double root_value(int n_root, double w_root) { return n_root > 0 ? -(w_root / (double)n_root) : NAN; }
RZY_FN Resign resign_rule(int n_root, double w_root, double q_children, double threshold) {
    const double v_root = root_value(n_root, w_root);
    const double q_best = q_children > -INFINITY ? q_children : NAN;
    Resign r;
    r.s = (isnan(v_root) || isnan(q_best)) ? NAN : fmax(v_root, q_best);
    r.fire = v_root < threshold && q_best < threshold;
    return r;
}

// ---- the draw of alphazero_mcts.py:88-92,147-148 from e[a] = exp(x[a] - max x) (0 at illegal actions): cumsum in action order (numpy's
// cumsum is sequential too), then the first interval whose upper edge exceeds u x total.  `rel`: the distance of u x total to the
// nearer edge of that interval, as a share of the total; the draw is taken (`ok`) only when it exceeds the margin -- else the host's
// numpy evaluation is the arbiter.
struct Draw {
    int action;   // -1: none
    double rel;
    bool ok;
};
RZY_FN Draw draw(const double *e, int A, double u, double margin) {
    double total = 0.0;
    for (int a = 0; a < A; ++a) total += e[a];
    const double target = u * total;
    double c = 0.0, below = 0.0;
    Draw d;
    d.action = -1;
    for (int a = 0; a < A; ++a) {
        const double ea = e[a];
        if (ea > 0.0 && c + ea > target) {
            d.action = a;
            below = c;
            c += ea;
            break;
        }
        c += ea;
    }
    d.rel = d.action >= 0 ? fmin(target - below, c - target) / total : 0.0;
    d.ok = d.action >= 0 && total > 0.0 && d.rel > margin;
    return d;
}

// ---- the queue of game ids (rz_play_queue_ring): head and valid count are ever-growing int32 counts, 0 <= head <= valid; with a
// capacity the entry of count c is c mod capacity, without one (0: the linear queue) it is c itself
RZY_FN int queue_slot(int count, int capacity) { return capacity > 0 ? count % capacity : count; }
// how many ids rz_play_queue_push may write behind `valid`: the ring's entries that hold no unclaimed id, and never more than the
// counts have left below the int32 limit (a push beyond either writes nothing); 0 for counts that are no queue's
RZY_FN int queue_room(int head, int valid, int capacity) {
    if (capacity <= 0 || head < 0 || valid < head) return 0;
    const int64_t free_entries = (int64_t)capacity - ((int64_t)valid - (int64_t)head);
    const int64_t counts_left = (int64_t)INT32_MAX - (int64_t)valid;
    const int64_t room = free_entries < counts_left ? free_entries : counts_left;
    return room > 0 ? (int)room : 0;
}

// ---- a slot's move step
enum { kIdle = 0, kRunning = 1, kStalled = 2 };   // Play::state
constexpr int kKeepAll = -2;      // Play::keep: no move -- the whole tree stays
constexpr int kKeepNone = -1;     // ... the move keeps no subtree: the next search starts from a fresh root
constexpr int kStepNone = -1;     // Play::stepm: no env.step
constexpr int kStepResign = -3;   // ... the mover resigned: k_play_apply ends the game without a step

struct SlotIn {
    int state;          // kIdle / kRunning / kStalled
    int64_t game;       // (the record's; an idle slot has none)
    int ply, root_n;
    int mail;           // a stalled slot's move from the host (rz_play_resolve), -1: none
    bool match;         // rz_play_set_match: a move keeps no subtree
    int full;           // RZ_PLAY_FULL or 0 (full_flag)
    bool resign_on;     // the resignation rule applies to this search: `resign` and `calibration` hold values
    Resign resign;
    bool calibration;   // resign_uniform < disabled_frac: the game never resigns
    Draw draw;          // read only where needs_draw()
};
// whether the slot's move is drawn at all: a running game whose mover does not resign
RZY_FN bool needs_draw(const SlotIn &in) { return in.state == kRunning && !(in.resign_on && in.resign.fire && !in.calibration); }

struct SlotOut {
    int move, flags;    // the record's: the move or -1; RZ_PLAY_* | winner_bits
    float edge, stat;   // ... the draw's distance to the nearer edge, the resignation statistic (0 where there is none)
    int keep, stepm;    // Play::keep, Play::stepm: update_with_move's and env.step's move
    int state, ply;     // the slot's state and ply after the step
    int active;         // Dev::active after the step, -1: as it is
    bool clear_mail;
};
RZY_FN SlotOut decide(const SlotIn &in) {
    SlotOut o;
    o.move = -1, o.flags = 0, o.edge = 0.0f, o.stat = 0.0f;
    o.keep = kKeepAll, o.stepm = kStepNone;
    o.state = in.state, o.ply = in.ply, o.active = -1, o.clear_mail = false;
    if (in.state == kIdle) return o;
    o.flags = RZ_PLAY_RUNNING;
    int move = -1;
    if (in.state == kStalled) {
        if (in.mail < 0) {   // still waiting for the host
            o.flags |= RZ_PLAY_STALLED;
            return o;
        }
        move = in.mail;      // the host has decided
        o.flags |= RZ_PLAY_RESOLVED;
        o.clear_mail = true;
        o.state = kRunning;
        o.active = 1;
    } else {
        o.flags |= RZ_PLAY_SEARCHED | in.full;
        if (in.resign_on) {
            o.stat = (float)in.resign.s;
            if (in.calibration) o.flags |= RZ_PLAY_NO_RESIGN | (in.resign.fire ? RZ_PLAY_WOULD_RESIGN : 0);
        }
        if (!needs_draw(in)) {   // the mover resigns: the other player wins; k_play_apply ends the game
            o.flags |= RZ_PLAY_ENDED | RZ_PLAY_RESIGNED | winner_bits(1 - in.ply % 2);
            o.stepm = kStepResign;
            return o;
        }
        o.edge = (float)in.draw.rel;
        if (!in.draw.ok) {   // too close to an edge: the coming searches skip the slot until the host has decided
            o.flags |= RZ_PLAY_STALLED;
            o.state = kStalled;
            o.active = 0;
            return o;
        }
        move = in.draw.action;
    }
    o.move = move;
    o.ply = in.ply + 1;
    o.keep = in.match ? kKeepNone : move;   // (a match searches every move from a fresh root: reset_player, alphazero_mcts.py:158)
    o.stepm = move;
    return o;
}

// the header words of the slot's record; an idle slot's says only that it holds no game
RZY_FN void write_record(int32_t *rec, const SlotIn &in, const SlotOut &o) {
    rec[kRecFlags] = o.flags;
    if (in.state == kIdle) return;
    rec[kRecGameLo] = (int32_t)(uint32_t)(uint64_t)in.game;
    rec[kRecGameHi] = (int32_t)((uint64_t)in.game >> 32);
    rec[kRecPly] = in.ply;
    rec[kRecMove] = o.move;
    rec[kRecRootN] = in.root_n;
    rec[kRecEdge] = float_bits(o.edge);
    rec[kRecStat] = float_bits(o.stat);
}
// k_play_apply's part: the game ended with the record's move (a resignation's record is complete already)
RZY_FN int ended_flags(int winner) { return RZ_PLAY_ENDED | winner_bits(winner); }

}  // namespace rzplay
