"""The move step's rules (rlzero_amd/csrc/rz_play.h) on the CPU, against the host's side of them.

A driver with its own main is compiled against the header with ROCm's clang++ (by tests/host_driver.py) with
-ffp-contract=off, fed binary inputs and compared in numpy: the keyed uniforms and the noise key with rlzero_amd/selfplay.py bit for
bit, the budget rule, the temperature table, the draw with selfplay.batch_pi_and_moves (the arbiter), the resignation rule with the
host's, and -- scripted slots played through rzplay::decide and rzplay::write_record into a log -- the device's writer with the
host's reader, rlzero_amd/playlog.py.  The same driver is also built with -fsanitize=address,undefined and run over all inputs."""
import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import host_driver
from rlzero_amd import playlog
from rlzero_amd._hip import (PLAY_ENDED, PLAY_FULL, PLAY_NO_RESIGN, PLAY_RECORD_WORDS, PLAY_RESIGNED, PLAY_RESOLVED, PLAY_RUNNING,
                             PLAY_SEARCHED, PLAY_STALLED, PLAY_WOULD_RESIGN)
from rlzero_amd.selfplay import _splitmix64, batch_pi_and_moves, cap_uniform, move_uniform, resign_uniform

W0 = PLAY_RECORD_WORDS
IDLE, RUNNING, STALLED = 0, 1, 2

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rz_play.h"

namespace ry = rzplay;

template <typename T>
static std::vector<T> load(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (bytes && fread(v.data(), 1, (size_t)bytes, f) != (size_t)bytes) exit(2);
    fclose(f);
    return v;
}
template <typename T>
static void store(const char *path, const std::vector<T> &v) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror(path); exit(2); }
    fclose(f);
}
static uint64_t bits(double v) { return __builtin_bit_cast(uint64_t, v); }

// keys in.u64 [N][3] (seed, game, ply) -> out.u64 [N][11]: move, match, resign, cap uniform, noise key, then for p_full = NaN, 0.25, 1:
// the budget of (n_full 40, n_fast 7) and the RZ_PLAY_FULL flag
static int keys(char **a) {
    const std::vector<uint64_t> in = load<uint64_t>(a[0]);
    const size_t n = in.size() / 3;
    std::vector<uint64_t> out(n * 11);
    const double ps[3] = {NAN, 0.25, 1.0};
    for (size_t i = 0; i < n; ++i) {
        const uint64_t seed = in[3 * i], game = in[3 * i + 1], ply = in[3 * i + 2];
        uint64_t *o = out.data() + 11 * i;
        o[0] = bits(ry::move_uniform(seed, game, ply));
        o[1] = bits(ry::match_uniform(seed, game, ply));
        o[2] = bits(ry::resign_uniform(seed, game));
        o[3] = bits(ry::cap_uniform(seed, game, ply));
        o[4] = ry::noise_key(seed, game);
        for (int k = 0; k < 3; ++k) {
            o[5 + 2 * k] = (uint64_t)ry::budget(40, 7, ps[k], seed, game, ply);
            o[6 + 2 * k] = (uint64_t)ry::full_flag(ps[k], seed, game, ply);
        }
    }
    store(a[1], out);
    return 0;
}

// table S n attach_inv_t margin temps.f64 -> out.f64 [2 S]
static int table(char **a) {
    const int S = atoi(a[0]), n = atoi(a[1]);
    const double attach_inv_t = atof(a[2]), margin = atof(a[3]);
    const std::vector<double> temps = load<double>(a[4]);   // exactly n entries (none: an empty vector, never read)
    if ((int)temps.size() != n) return 4;
    std::vector<double> out(2 * (size_t)S);
    for (int i = 0; i < 2 * S; ++i) out[i] = ry::temp_entry(i, S, temps.data(), n, attach_inv_t, margin);
    store(a[5], out);
    return 0;
}

// draw A in.f64 [R][2 + A] (u, margin, e) -> out.f64 [R][3] (action, ok, rel)
static int draws(char **a) {
    const int A = atoi(a[0]);
    const std::vector<double> in = load<double>(a[1]);
    const size_t R = in.size() / (2 + A);
    std::vector<double> out(R * 3);
    for (size_t r = 0; r < R; ++r) {
        const double *row = in.data() + r * (2 + A);
        const std::vector<double> e(row + 2, row + 2 + A);   // (a heap array of exactly A entries)
        const ry::Draw d = ry::draw(e.data(), A, row[0], row[1]);
        out[3 * r] = d.action, out[3 * r + 1] = d.ok ? 1.0 : 0.0, out[3 * r + 2] = d.rel;
    }
    store(a[2], out);
    return 0;
}

// resign in.f64 [R][4] (N, W, best child W / N or -inf, threshold) -> out.i32 [R][2] (float bits of s, fire)
static int resign(char **a) {
    const std::vector<double> in = load<double>(a[0]);
    const size_t R = in.size() / 4;
    std::vector<int32_t> out(R * 2);
    for (size_t r = 0; r < R; ++r) {
        const ry::Resign g = ry::resign_rule((int)in[4 * r], in[4 * r + 1], in[4 * r + 2], in[4 * r + 3]);
        out[2 * r] = ry::float_bits((float)g.s), out[2 * r + 1] = g.fire ? 1 : 0;
    }
    store(a[1], out);
    return 0;
}

// script steps G A seed disabled_frac p_full events.f64 [steps][G][kEv + A] counts.i32 [steps][G][A] -> log.i32 [steps][G][8 + A],
// outs.i32 [steps][G][8].  The slots as k_play_draw and k_play_apply keep them: state, game, ply, mailbox.
enum { kPost, kMargin, kRootN, kRootW, kBest, kThreshold, kOver, kWinner, kRefill, kMatch, kCapOn, kEv };
static int script(char **a) {
    const int steps = atoi(a[0]), G = atoi(a[1]), A = atoi(a[2]);
    const uint64_t seed = strtoull(a[3], nullptr, 10);
    const double frac = atof(a[4]), p_full = atof(a[5]);
    const std::vector<double> ev = load<double>(a[6]);
    const std::vector<int32_t> counts = load<int32_t>(a[7]);
    const int words = RZ_PLAY_RECORD_WORDS + A;
    if (ev.size() != (size_t)steps * G * (kEv + A) || counts.size() != (size_t)steps * G * A) return 4;
    std::vector<int32_t> log((size_t)steps * G * words, 0x5A5A5A5A), outs((size_t)steps * G * 8);
    std::vector<int> state(G, ry::kIdle), ply(G, 0), mail(G, -1);
    std::vector<int64_t> game(G, -1);
    for (int s = 0; s < steps; ++s)
        for (int g = 0; g < G; ++g) {
            const double *v = ev.data() + ((size_t)s * G + g) * (kEv + A);
            const int32_t *cnt = counts.data() + ((size_t)s * G + g) * A;
            int32_t *rec = log.data() + ((size_t)s * G + g) * words, *out = outs.data() + ((size_t)s * G + g) * 8;
            if (v[kPost] >= 0.0) mail[g] = (int)v[kPost];   // rz_play_resolve before this step
            // k_play_draw
            ry::SlotIn in = {};
            in.state = state[g];
            if (in.state != ry::kIdle) {
                for (int i = 0; i < A; ++i) rec[RZ_PLAY_RECORD_WORDS + i] = cnt[i];
                const uint64_t gid = (uint64_t)game[g];
                in.game = game[g], in.ply = ply[g], in.root_n = (int)v[kRootN], in.match = v[kMatch] != 0.0;
                if (in.state == ry::kStalled) {
                    in.mail = mail[g];
                } else {
                    in.full = v[kCapOn] != 0.0 ? ry::full_flag(p_full, seed, gid, (uint64_t)in.ply) : 0;
                    in.resign_on = !isnan(v[kThreshold]);
                    if (in.resign_on) {
                        in.resign = ry::resign_rule(in.root_n, v[kRootW], v[kBest], v[kThreshold]);
                        in.calibration = ry::resign_uniform(seed, gid) < frac;
                    }
                    if (ry::needs_draw(in)) {
                        const double u = in.match ? ry::match_uniform(seed, gid, (uint64_t)in.ply) : ry::move_uniform(seed, gid, (uint64_t)in.ply);
                        const std::vector<double> e(v + kEv, v + kEv + A);
                        in.draw = ry::draw(e.data(), A, u, v[kMargin]);
                    }
                }
            }
            const ry::SlotOut o = ry::decide(in);
            ry::write_record(rec, in, o);
            if (o.clear_mail) mail[g] = -1;
            state[g] = o.state, ply[g] = o.ply;
            out[0] = o.keep, out[1] = o.stepm, out[2] = o.state, out[3] = o.ply, out[4] = o.active, out[5] = o.clear_mail ? 1 : 0, out[6] = -1;
            // k_play_apply: the end of a game, the budget of the coming search, the refill
            if (state[g] == ry::kRunning && ((o.stepm >= 0 && v[kOver] != 0.0) || o.stepm == ry::kStepResign)) {
                if (o.stepm >= 0) rec[ry::kRecFlags] |= ry::ended_flags((int)v[kWinner]);
                state[g] = ry::kIdle, game[g] = -1;
            }
            if (state[g] == ry::kIdle && v[kRefill] >= 0.0) game[g] = (int64_t)v[kRefill], ply[g] = 0, state[g] = ry::kRunning, mail[g] = -1;
            if (v[kCapOn] != 0.0 && state[g] == ry::kRunning) out[6] = ry::budget(40, 7, p_full, seed, (uint64_t)game[g], (uint64_t)ply[g]);
            out[7] = state[g];
        }
    store(a[8], log);
    store(a[9], outs);
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "keys" && argc == 4) return keys(argv + 2);
    if (what == "table" && argc == 8) return table(argv + 2);
    if (what == "draw" && argc == 5) return draws(argv + 2);
    if (what == "resign" && argc == 4) return resign(argv + 2);
    if (what == "script" && argc == 12) return script(argv + 2);
    return 4;
}
'''


drv = host_driver.fixture('play', DRIVER)


def f64(bits):
    return np.ascontiguousarray(bits).view(np.float64)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


# ----------------------------------------------------------------------------------------------- keys and the budget
SEEDS = [0, 13, 2 ** 64 - 1]
GAMES = [0, 1, 2 ** 31, 2 ** 40 + 3]


@pytest.fixture(scope='module')
def keyed(drv):
    keys = np.array([(s, g, p) for s in SEEDS for g in GAMES for p in range(256)], dtype=np.uint64)
    out, = drv.run('keys', [], [keys], [np.uint64])
    return keys, out.reshape(len(keys), 11)


def test_keys_are_the_hosts_bits(keyed):
    keys, out = keyed
    for seed in SEEDS:
        rows = keys[:, 0] == np.uint64(seed)
        game, ply = keys[rows, 1], keys[rows, 2]
        o = out[rows]
        assert np.array_equal(o[:, 0], move_uniform(seed, game, ply).view(np.uint64))
        assert np.array_equal(o[:, 1], move_uniform(seed, game >> np.uint64(1), np.uint64(2) * ply + np.uint64(1)).view(np.uint64))
        assert np.array_equal(o[:, 2], resign_uniform(seed, game).view(np.uint64))
        assert np.array_equal(o[:, 3], cap_uniform(seed, game, ply).view(np.uint64))
        with np.errstate(over='ignore'):   # the expression of BatchedSelfPlay._start
            noise = _splitmix64(_splitmix64(np.uint64(seed) ^ np.uint64(0x6E6F697365000000)) ^ game.astype(np.uint64))
        assert np.array_equal(o[:, 4], noise)
    u = f64(out[:, :4])
    assert (u >= 0.0).all() and (u < 1.0).all()


def test_budget_rule(keyed):
    keys, out = keyed
    cap_u = f64(out[:, 3])
    for k, p in enumerate((np.nan, 0.25, 1.0)):
        full = np.full(len(keys), True) if np.isnan(p) else cap_u < p
        assert np.array_equal(out[:, 5 + 2 * k], np.where(full, 40, 7).astype(np.uint64))
        assert np.array_equal(out[:, 6 + 2 * k], np.where(full & ~np.isnan(p), PLAY_FULL, 0).astype(np.uint64))   # never set without a cap
    assert 0.15 < (cap_u < 0.25).mean() < 0.35   # (both budgets occur)


# ----------------------------------------------------------------------------------------------- the temperature table
@pytest.mark.parametrize('S', [9, 121, 225])
def test_temperature_table(drv, S):
    """1 / T on the host, padded with the last entry (no entry: the temperature of rz_play_attach); behind it every ply's stall
    margin: the configured one if positive, else 1e-10 * max(1 / T, 1)."""
    rng = np.random.RandomState(S)
    attach_t = 0.8
    for n in (0, 1, 7, S):
        temps = np.concatenate([rng.uniform(0.05, 2.0, size=n)[:max(n - 2, 0)], [1e-3, 1.0][:min(n, 2)]])   # (1 / T above and at 1)
        assert temps.size == n
        for cfg in (0.0, 0.02):
            got, = drv.run('table', [S, n, repr(1.0 / attach_t), repr(cfg)], [temps], [np.float64])
            inv_t = np.full(S, 1.0 / attach_t) if n == 0 else 1.0 / temps[np.minimum(np.arange(S), n - 1)]
            margin = np.full(S, cfg) if cfg > 0.0 else 1e-10 * np.maximum(inv_t, 1.0)
            assert got.shape == (2 * S, ) and same_bits(got, np.concatenate([inv_t, margin])), (S, n, cfg)


# ----------------------------------------------------------------------------------------------- the draw
def exp_rows(visits, legal, T):
    """e of batch_pi_and_moves: exp(1 / T log(visits + 1e-10) - max over the legal ones), 0 at illegal actions."""
    x = 1.0 / T * np.log(visits + 1e-10)
    mx = np.where(legal, x, -np.inf).max(axis=1)
    return np.exp(np.where(legal, x - mx[:, None], -np.inf))


def draw_restated(e, u, margin):
    """(action, ok, rel) of one row: the sequential cumsum, the first positive interval whose upper edge exceeds u x total."""
    c = np.cumsum(e)
    total = c[-1]
    target = u * total
    hit = np.nonzero((e > 0.0) & (c > target))[0]
    if hit.size == 0:
        return -1, False, 0.0
    a = int(hit[0])
    below = c[a - 1] if a > 0 else 0.0
    rel = np.minimum(target - below, c[a] - target) / total
    return a, bool(total > 0.0 and rel > margin), rel


def run_draw(drv, e, u, margin):
    e = np.asarray(e, dtype=np.float64)
    rows = np.concatenate([np.asarray(u, dtype=np.float64)[:, None], np.broadcast_to(np.float64(margin), (len(e), ))[:, None], e], axis=1)
    out, = drv.run('draw', [e.shape[1]], [rows], [np.float64])
    out = out.reshape(len(e), 3)
    return out[:, 0].astype(np.int64), out[:, 1] != 0.0, out[:, 2]


@pytest.mark.parametrize('A', [9, 36, 121, 225, 256])
def test_draw_is_the_arbiters(drv, A):
    """Random visit counts under random legal masks, 750 rows per (A, T): 11250 rows in all.  With the margin 1e-10 no row may stall
    (a uniform falls that close to one of at most A edges with a chance of order A 1e-10), and every move is batch_pi_and_moves'."""
    rng = np.random.RandomState(1000 + A)
    for T in (1.0, 0.25, 1e-3):
        R = 750
        legal = rng.uniform(size=(R, A)) < rng.uniform(0.1, 1.0, size=(R, 1))
        legal[np.arange(R), rng.randint(A, size=R)] = True
        visits = np.where(legal, rng.multinomial(400, rng.dirichlet(np.full(A, 0.3), size=R)[0], size=R), 0)
        visits[rng.uniform(size=(R, A)) < 0.3] = 0
        u = rng.uniform(size=R)
        e = exp_rows(visits, legal, T)
        action, ok, rel = run_draw(drv, e, u, 1e-10)
        _, moves = batch_pi_and_moves(visits, legal, T, u)
        assert ok.all(), (A, T, int((~ok).sum()))
        assert np.array_equal(action, moves)
        assert legal[np.arange(R), action].all()
        want = [draw_restated(e[r], u[r], 1e-10) for r in range(R)]
        assert np.array_equal(action, [w[0] for w in want]) and same_bits(rel, [w[2] for w in want])
        assert rel.min() > 1e-10


def test_draw_constructed_rows(drv):
    last = 1.0 - 2.0 ** -53
    # a single legal action; all counts zero (every legal action alike); u = 0 and the largest u
    legal = np.zeros((4, 9), dtype=bool)
    legal[0, 5] = True
    legal[1:, [1, 4, 7]] = True
    visits = np.zeros((4, 9), dtype=np.int64)
    visits[0, 5] = 17
    visits[2:, [1, 4, 7]] = [3, 9, 5]
    u = np.array([0.3, 0.5, 0.0, last])
    e = exp_rows(visits, legal, 1.0)
    action, ok, rel = run_draw(drv, e, u, 1e-10)
    _, moves = batch_pi_and_moves(visits, legal, 1.0, u)
    assert action.tolist() == [5, 4, 1, 7]
    # (u = 0 lies ON the lower edge of the first interval, the largest u one ulp below the upper edge of the last: the arbiter decides)
    assert ok.tolist() == [True, True, False, False]
    assert np.array_equal(action[ok], moves[ok])
    assert same_bits(rel, [draw_restated(e[r], u[r], 1e-10)[2] for r in range(4)])
    assert rel[2] == 0.0 and 0.0 < rel[3] < 1e-15
    # u on an edge must stall
    ones = np.ones((3, 4))
    action, ok, rel = run_draw(drv, ones, [0.25, 0.5, 0.75], 1e-10)
    assert not ok.any() and (rel == 0.0).all() and action.tolist() == [1, 2, 3]
    # margin 0.02: 0.01 from an edge stalls, 0.03 from it does not, on either side
    action, ok, rel = run_draw(drv, np.ones((4, 4)), [0.51, 0.49, 0.53, 0.47], 0.02)
    assert ok.tolist() == [False, False, True, True] and action.tolist() == [2, 1, 2, 1]
    assert same_bits(rel, [draw_restated(np.ones(4), x, 0.02)[2] for x in (0.51, 0.49, 0.53, 0.47)])
    assert np.allclose(rel, [0.01, 0.01, 0.03, 0.03], rtol=0, atol=1e-12)
    # no legal action at all: no draw
    action, ok, rel = run_draw(drv, np.zeros((1, 9)), [0.5], 1e-10)
    assert action.tolist() == [-1] and not ok.any() and rel.tolist() == [0.0]


# ----------------------------------------------------------------------------------------------- the resignation rule
def test_resign_rule_is_the_hosts(drv):
    """rz_root_values' {v_root, q_best} -- -W / N of the root, the best child's W / N, NaN where undefined -- and the host's rule on
    them (selfplay.py, "the rule of k_play_draw"): s = max of the two as float32, NaN when either is; fire = both below the threshold."""
    grid = np.array([(n, w, q, t) for n in (0, 1, 7, 400) for w in (-400.0, -6.5, 0.0, 0.3, 7.0)
                     for q in (-np.inf, -1.0, -0.85, -0.8, 0.0, 0.9) for t in (np.nan, -1.0, -0.8, -0.5, 0.95, np.inf)], dtype=np.float64)
    out, = drv.run('resign', [], [grid], [np.int32])
    out = out.reshape(len(grid), 2)
    n, w, q, thr = grid.T
    with np.errstate(invalid='ignore', divide='ignore'):
        v_root = np.where(n > 0, -(w / n), np.nan)
        q_best = np.where(q > -np.inf, q, np.nan)
        stat = np.maximum(v_root, q_best).astype(np.float32)
        fire = (v_root < thr) & (q_best < thr)
    got = np.ascontiguousarray(out[:, 0]).view(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(stat)) and np.array_equal(got[~np.isnan(stat)], stat[~np.isnan(stat)])
    assert np.array_equal(out[:, 1] != 0, fire)
    assert fire.any() and np.isnan(stat).any() and not fire[np.isnan(stat)].any()


# ----------------------------------------------------------------------------------------------- writer against reader
SEED, FRAC, P_FULL, A, THRESHOLD = 13, 0.3, 0.5, 9, -0.8
EV = dict(post=0, margin=1, root_n=2, root_w=3, best=4, threshold=5, over=6, winner=7, refill=8, match=9, cap_on=10)
N_EV = len(EV)
CALIB = [g for g in range(200) if resign_uniform(SEED, g) < FRAC]
PLAYED = [g for g in range(200) if resign_uniform(SEED, g) >= FRAC]
# a game whose first four searches hold a full and a fast one
CAPPED = next(g for g in range(200) if 0 < int((cap_uniform(SEED, g, np.arange(4)) < P_FULL).sum()) < 4)


class Slot(object):
    """The script of one slot: per step the event the driver reads and the record and slot state the header must make of it."""

    def __init__(self, rng, game=None, match=False, cap=False):
        self.rng, self.game, self.match, self.cap = rng, game, match, cap
        self.events, self.counts, self.want = [], [], []
        self.ply, self.taken = 0, np.zeros(A, dtype=bool)
        self.moves, self.searched, self.pending = [], 0, None
        self.step(refill=game)   # the slot's first step: idle, then the refill

    def u(self):
        return float(move_uniform(SEED, self.game >> 1, 2 * self.ply + 1) if self.match else move_uniform(SEED, self.game, self.ply))

    def step(self, kind='idle', refill=None, over=False, winner=-1, resign=None, post=None):
        """``kind``: idle, move, stall (searched, too close to an edge), wait (stalled, no mail), resolve (stalled, mail)."""
        ev = np.zeros(N_EV + A)
        ev[EV['post']], ev[EV['refill']], ev[EV['threshold']], ev[EV['best']] = -1, -1, np.nan, -np.inf
        ev[EV['match']], ev[EV['cap_on']] = self.match, self.cap
        cnt = np.full(A, -7, dtype=np.int32)
        want = dict(kind=kind, game=self.game, ply=self.ply)
        if refill is not None:
            ev[EV['refill']] = refill
        if kind != 'idle':
            legal = ~self.taken
            n = np.where(legal, self.rng.multinomial(39, self.rng.dirichlet(np.ones(A))), 0)
            cnt[:] = np.where(legal, n, -1)
            ev[EV['root_n']] = want['root_n'] = int(n.sum()) + 1
            ev[N_EV:] = exp_rows(n[None], legal[None], 1.0)[0]
            ev[EV['margin']] = 1.0 if kind == 'stall' else 1e-10
            want['counts'] = cnt.copy()
            want['chosen'] = int(batch_pi_and_moves(n[None], legal[None], 1.0, [self.u()])[1][0])
        if resign is not None:   # (v_root, q_best) the search is scripted to have left
            v_root, q_best = resign
            ev[EV['root_w']], ev[EV['best']], ev[EV['threshold']] = -v_root * ev[EV['root_n']], q_best, THRESHOLD
            want['stat'] = np.float32(max(-(ev[EV['root_w']] / ev[EV['root_n']]), q_best))
            want['fire'] = bool(-(ev[EV['root_w']] / ev[EV['root_n']]) < THRESHOLD and q_best < THRESHOLD)
        if kind == 'stall':
            self.pending = want['chosen']
        if post:
            ev[EV['post']] = self.pending
        if kind == 'resolve':
            want['chosen'] = self.pending
        want.update(over=over, winner=winner)
        ev[EV['over']], ev[EV['winner']] = over, winner
        self.events.append(ev)
        self.counts.append(cnt)
        self.want.append(want)
        resigned = resign is not None and want['fire'] and self.game not in CALIB
        if kind in ('move', 'stall'):
            self.searched += 1
        if kind in ('move', 'resolve') and not resigned:
            self.moves.append(want['chosen'])
            self.taken[want['chosen']] = True
            self.ply += 1
        want['resigned'] = resigned
        if resigned:
            want['winner'] = 1 - want['ply'] % 2
        return self


def scripts():
    rng = np.random.RandomState(5)
    idle = Slot(rng)
    plain = Slot(rng, game=3).step('move').step('move').step('move', over=True, winner=0)
    stall = Slot(rng, game=2 ** 40 + 3).step('move').step('stall').step('wait').step('resolve', post=True).step('move', over=True, winner=-1)
    resign = (Slot(rng, game=PLAYED[0]).step('move', resign=(0.1, 0.2)).step('move', resign=(-0.9, -0.7))
              .step('move', resign=(-0.9, -0.85)))
    calib = (Slot(rng, game=CALIB[0]).step('move', resign=(0.0, 0.3)).step('move', resign=(-0.95, -0.9))
             .step('move', resign=(0.5, 0.1), over=True, winner=1))
    capped = Slot(rng, game=CAPPED, cap=True).step('move').step('move').step('move').step('move', over=True, winner=1)
    pair = [Slot(rng, game=10, match=True).step('move').step('stall').step('resolve', post=True).step('move', over=True, winner=0),
            Slot(rng, game=11, match=True).step('move').step('move').step('move', over=True, winner=1)]
    slots = [idle, plain, stall, resign, calib, capped] + pair
    steps = max(len(s.events) for s in slots) + 1
    for s in slots:
        while len(s.events) < steps:
            s.step()
    return slots, steps


@pytest.fixture(scope='module')
def played(drv):
    slots, steps = scripts()
    G = len(slots)
    events = np.stack([np.stack([s.events[t] for s in slots]) for t in range(steps)])
    counts = np.stack([np.stack([s.counts[t] for s in slots]) for t in range(steps)])
    log, outs = drv.run('script', [steps, G, A, SEED, repr(FRAC), repr(P_FULL)], [events, counts], [np.int32, np.int32])
    return slots, log.reshape(steps, G, W0 + A), outs.reshape(steps, G, 8)


def test_script_holds_every_case():
    slots, _ = scripts()
    kinds = [[w['kind'] for w in s.want] for s in slots]
    assert set(kinds[0]) == {'idle'} and kinds[2].count('stall') == 1 and kinds[2].count('wait') == 1 and kinds[2].count('resolve') == 1
    assert [w['resigned'] for w in slots[3].want if w['kind'] == 'move'] == [False, False, True]
    assert [w['fire'] for w in slots[4].want if w['kind'] == 'move'] == [False, True, False] and slots[4].game in CALIB
    full = cap_uniform(SEED, CAPPED, np.arange(4)) < P_FULL
    assert full.any() and not full.all()
    assert slots[6].game >> 1 == slots[7].game >> 1 and slots[6].match and slots[7].match


def test_every_word_of_every_record(played):
    """The record decide and write_record leave, read with playlog.decode, and the slot's arrays, step by step."""
    slots, log, outs = played
    for g, s in enumerate(slots):
        state = IDLE
        for t, w in enumerate(s.want):
            rec, out = log[t, g], outs[t, g]
            d = playlog.Records(*[field[0] for field in playlog.decode(rec[None])])
            keep, stepm, new_state, new_ply, active, clear_mail, sims, after = out.tolist()
            where = (g, t, w['kind'])
            if w['kind'] == 'idle':   # only the flag word is written; nothing of the slot changes
                assert rec[4] == 0 and (np.delete(rec, 4) == 0x5A5A5A5A).all(), where
                assert (keep, stepm, new_state, active, clear_mail) == (-2, -1, IDLE, -1, 0), where
                assert state == IDLE
                state = after
                continue
            assert int(d.game) == s.game and int(d.ply) == w['ply'] and int(d.root_n) == w['root_n'], where
            assert np.array_equal(d.visits, w['counts']), where
            flags = int(d.flags)
            assert flags & PLAY_RUNNING
            searched = w['kind'] in ('move', 'stall')
            assert bool(flags & PLAY_SEARCHED) == searched, where
            if s.cap:
                assert bool(flags & PLAY_FULL) == (searched and bool(cap_uniform(SEED, s.game, w['ply']) < P_FULL)), where
            else:
                assert not flags & PLAY_FULL
            if 'stat' in w:
                assert float(d.stat) == float(w['stat']), where
                assert bool(flags & PLAY_NO_RESIGN) == (s.game in CALIB), where
                assert bool(flags & PLAY_WOULD_RESIGN) == (w['fire'] and s.game in CALIB), where
            else:
                assert int(rec[7]) == 0 and not flags & (PLAY_NO_RESIGN | PLAY_WOULD_RESIGN), where
            assert bool(flags & PLAY_RESIGNED) == w['resigned'], where
            if w['resigned']:
                assert flags & PLAY_ENDED and int(d.winner) == w['winner'] and int(d.move) == -1 and int(rec[6]) == 0, where
                assert (keep, stepm, new_state, new_ply, active, clear_mail, after) == (-2, -3, RUNNING, w['ply'], -1, 0, IDLE), where
            elif w['kind'] in ('stall', 'wait'):
                assert flags & PLAY_STALLED and not flags & (PLAY_RESOLVED | PLAY_ENDED) and int(d.move) == -1, where
                assert (keep, stepm, new_state, new_ply, clear_mail, after) == (-2, -1, STALLED, w['ply'], 0, STALLED), where
                assert active == (0 if w['kind'] == 'stall' else -1), where
                assert (float(d.edge) > 0.0) if w['kind'] == 'stall' else int(rec[6]) == 0, where
            else:
                assert not flags & PLAY_STALLED and int(d.move) == w['chosen'], where
                assert bool(flags & PLAY_RESOLVED) == (w['kind'] == 'resolve'), where
                assert (keep, stepm, new_state, new_ply) == (-1 if s.match else w['chosen'], w['chosen'], RUNNING, w['ply'] + 1), where
                assert (active, clear_mail) == ((1, 1) if w['kind'] == 'resolve' else (-1, 0)), where
                assert (float(d.edge) > 1e-10) if w['kind'] == 'move' else int(rec[6]) == 0, where
                assert bool(flags & PLAY_ENDED) == w['over'] and int(d.winner) == (w['winner'] if w['over'] else -1), where
                assert after == (IDLE if w['over'] else RUNNING), where
            if s.cap and after == RUNNING:   # the budget of the coming search: the flag its record will carry
                assert sims == (40 if cap_uniform(SEED, s.game, new_ply) < P_FULL else 7), where
            else:
                assert sims == -1, where
            state = after


def test_the_reader_finishes_the_scripted_games(played):
    """The log through playlog.running and SlotBook.feed, row by row: the stalls are handed back with the arbiter's moves, and the
    Finished games are the scripted ones."""
    slots, log, _ = played
    G = len(slots)
    calls = []
    book = playlog.SlotBook(G, A, lambda s, m: calls.append((s, m)), {'n': (np.int32, (), 'move'), 'stat': (np.float32, (), 'search')})
    done = []
    for t in range(len(log)):
        at, d, last = playlog.running(log[t:t + 1])
        assert last == len(at) == sum(1 for s in slots if s.want[t]['kind'] != 'idle')
        chosen = np.array([slots[g].want[t]['chosen'] for g in at], dtype=np.int64)
        playlog.check_moves(d, chosen)
        done.extend(book.feed(at, d, chosen, {'n': d.root_n, 'stat': d.stat}))
    assert book.stalls == {} and (book.slot_game == -1).all()
    assert calls == [(g, w['chosen']) for t in range(len(log)) for g, s in enumerate(slots) for w in [s.want[t]] if w['kind'] == 'stall']
    assert book.started == G - 1 and book.stalls_resolved == 2 and book.moves_done == sum(len(s.moves) for s in slots)
    assert sorted(f.slot for f in done) == list(range(1, G))
    for f in done:
        s = slots[f.slot]
        last = [w for w in s.want if w['kind'] != 'idle'][-1]
        assert f.game == s.game and f.moves.tolist() == s.moves and f.searched == s.searched, f.slot
        assert (f.winner, f.resigned) == (last['winner'], last['resigned']), f.slot
        assert len(f.columns['n']) == len(s.moves) and len(f.columns['stat']) == s.searched
    assert [f.resigned for f in sorted(done, key=lambda f: f.slot)] == [False, False, True, False, False, False, False]
