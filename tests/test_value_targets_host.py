"""Value targets from the search, on the CPU: the two rules the kernels call -- rz_replay_rules.h's ``value_target`` (the mix
(1 - lam) z + lam q that k_replay_gather / k_replay_sample write) and rz_play.h's ``root_value`` (what k_play_draw logs into the side
ring) -- against their Python statements, ``replay.mixed_value_targets`` and ``-(W / N)`` in Python floats, bit for bit; the reader of
the side ring (selfplay.SelfPlayReader) on a scripted log; and the host route (Trajectory.training_samples(value_mix=)).

A driver with its own main is compiled against both headers with ROCm's clang++ -- without fused contraction, as the library is --
and once more with -fsanitize=address,undefined (a stand-alone program); every call runs both and holds their outputs equal.

The contraction guard.  A fused multiply-add rounds lam * q + keep once where the rule rounds twice; the two differ in the last
bit of the fp64 sum, and the float32 cast hides that unless the sum lies within an fp64 ulp of a float32 TIE -- for triples drawn
uniformly that happens once in about 2^29.  So half of the random triples are drawn uniformly and half are drawn NEAR TIES: q and
z at random, a float32 tie M between them at random, lam = fp64((z - M) / (z - q)), which puts (1 - lam) z + lam q within rounding
of M.  Among those a few per cent come out differently under a fused evaluation (computed here in exact rationals), and the test
requires that at least one does: the bit comparison with numpy would catch a contracted build."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import host_driver
from rlzero_amd._hip import PLAY_RESOLVED, PLAY_RUNNING, PLAY_SEARCHED, PLAY_STALLED
from rlzero_amd.replay import kept_root_values, mixed_value_targets
from rlzero_amd.selfplay import Trajectory
from host_driver import CSRC
from test_mz_replay_host import same_bits
from test_playlog_host import Cfg, Game, Writer

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "rz_play.h"
#include "rz_replay_rules.h"

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

// mix z.f32 [n] q.f32 [n] lam.f64 [n] -> target.f32 [n]
static int mix(char **a) {
    const std::vector<float> z = load<float>(a[0]), q = load<float>(a[1]);
    const std::vector<double> lam = load<double>(a[2]);
    if (q.size() != z.size() || lam.size() != z.size()) return 4;
    std::vector<float> out(z.size());
    for (size_t i = 0; i < z.size(); ++i) out[i] = rzrr::value_target(z[i], q[i], lam[i]);
    store(a[3], out);
    return 0;
}

// vroot n.i32 [n] w.f64 [n] -> v.f64 [n] ring.f32 [n] (what k_play_draw writes) stat.f64 [n] (resign_rule's s with q_children = v:
// the rule still sees the same root value)
static int vroot(char **a) {
    const std::vector<int32_t> n = load<int32_t>(a[0]);
    const std::vector<double> w = load<double>(a[1]);
    if (w.size() != n.size()) return 4;
    std::vector<double> v(n.size()), stat(n.size());
    std::vector<float> ring(n.size());
    for (size_t i = 0; i < n.size(); ++i) {
        v[i] = rzplay::root_value(n[i], w[i]);
        ring[i] = (float)v[i];
        stat[i] = rzplay::resign_rule(n[i], w[i], -2.0, 0.0).s;   // max(v_root, -2) = v_root for values in [-1, 1]
    }
    store(a[2], v);
    store(a[3], ring);
    store(a[4], stat);
    return 0;
}

// written slot.i64 [n] v.f64 [n] capacity -> written.i32 [n]
static int written(char **a) {
    const long long capacity = atoll(a[0]);
    const std::vector<int64_t> slot = load<int64_t>(a[1]);
    const std::vector<double> v = load<double>(a[2]);
    std::vector<int32_t> out(slot.size());
    for (size_t i = 0; i < slot.size(); ++i) out[i] = rzrr::value_written(slot[i], capacity, v[i]) ? 1 : 0;
    store(a[3], out);
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "mix" && argc == 6) return mix(argv + 2);
    if (what == "vroot" && argc == 7) return vroot(argv + 2);
    if (what == "written" && argc == 6) return written(argv + 2);
    return 4;
}
'''


drv = host_driver.fixture('value_targets', DRIVER)


def test_the_library_is_built_without_contraction():
    """The rule's two roundings hold only without fused contraction: the build recipe says so for every source."""
    from rlzero_amd import _build
    assert '-ffp-contract=off' in _build.FLAGS
    with open(os.path.join(CSRC, 'rz_replay.hip')) as f:
        text = f.read()
    assert '#include "rz_replay_rules.h"' in text and '#include "rz_replay_dev.h"' in text
    with open(os.path.join(CSRC, 'rz_replay_dev.h')) as f:   # (replay_emit, which both mini-batch kernels of rz_replay.hip write through)
        text = f.read()
    assert '#include "rz_replay_rules.h"' in text and 'rzrr::value_target' in text
    with open(os.path.join(CSRC, 'rz_engine_play.h')) as f:
        assert 'ry::root_value' in f.read()


# ----------------------------------------------------------------------------------------------- the mix
def _bits32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def random_triples(n_uniform=2048, n_ties=2048, seed=20):
    """-> (z float32, q float32, lam float64): ``n_uniform`` triples drawn uniformly and up to ``n_ties`` drawn near float32 ties
    (the module docstring)."""
    rs = np.random.RandomState(seed)
    z = rs.choice(np.array([-1.0, 0.0, 1.0], dtype=np.float32), size=n_uniform)
    q = rs.uniform(-1.0, 1.0, size=n_uniform).astype(np.float32)
    lam = rs.uniform(0.0, 1.0, size=n_uniform)
    zs, qs, lams = list(z), list(q), list(lam)
    for _ in range(n_ties):
        zt = np.float32(rs.choice([-1.0, 1.0]))
        qt = np.float32(rs.uniform(-1.0, 1.0))
        if qt == zt:
            continue
        t = np.float32(rs.uniform(min(zt, qt), max(zt, qt)))
        tie = (float(t) + float(np.nextafter(t, np.float32(2.0), dtype=np.float32))) / 2.0   # (exact in fp64: 25 significant bits)
        lt = (float(zt) - tie) / (float(zt) - float(qt))
        if 0.0 <= lt <= 1.0:
            zs.append(zt), qs.append(qt), lams.append(lt)
    return np.array(zs, dtype=np.float32), np.array(qs, dtype=np.float32), np.array(lams, dtype=np.float64)


def fused_targets(z, q, lam):
    """The two evaluations a contracting compiler could make of keep + take -- fma(lam, q, keep) and fma(1 - lam, z, take) -- in exact
    rationals, rounded to fp64 once (float(Fraction) rounds to nearest even) and cast to float32."""
    a, b = [], []
    for zi, qi, li in zip(z.tolist(), q.tolist(), lam.tolist()):
        keep, take = (1.0 - li) * zi, li * qi
        a.append(np.float32(float(Fraction(li) * Fraction(qi) + Fraction(keep))))
        b.append(np.float32(float(Fraction(1.0 - li) * Fraction(zi) + Fraction(take))))
    return np.array(a, dtype=np.float32), np.array(b, dtype=np.float32)


def test_value_target_is_numpys_on_random_triples_and_contraction_would_show(drv):
    z, q, lam = random_triples()
    assert len(z) > 3000
    want = np.array([mixed_value_targets(z[i:i + 1], q[i:i + 1], lam[i])[0] for i in range(len(z))], dtype=np.float32)
    got, = drv.run('mix', [], [z, q, lam], [np.float32])
    assert same_bits(got, want)
    # the guard: a fused multiply-add gives other bits on some of these triples -- the comparison above would not have passed
    fused_a, fused_b = fused_targets(z, q, lam)
    differ_a, differ_b = int((_bits32(fused_a) != _bits32(want)).sum()), int((_bits32(fused_b) != _bits32(want)).sum())
    print('triples %d; under fma(lam, q, keep) %d differ, under fma(1 - lam, z, take) %d' % (len(z), differ_a, differ_b))
    assert differ_a >= 1


def test_value_target_on_crafted_triples(drv):
    tiny, sub = np.float32(1.1754944e-38), np.float32(1e-45)   # the smallest normal and the smallest denormal float32
    qs = np.array([1.0, -1.0, 0.0, -0.0, np.nan, tiny, -tiny, sub, -sub, 0.5, -0.3], dtype=np.float32)
    lams = [0.0, 1.0, 0.5, 0.25, 1.0 / 3.0]
    z, q, lam = [], [], []
    for zi in (-1.0, 0.0, 1.0):
        for qi in qs:
            for li in lams:
                z.append(zi), q.append(qi), lam.append(li)
    z, q, lam = np.array(z, dtype=np.float32), np.array(q, dtype=np.float32), np.array(lam, dtype=np.float64)
    got, = drv.run('mix', [], [z, q, lam], [np.float32])
    want = np.array([mixed_value_targets(z[i:i + 1], q[i:i + 1], lam[i])[0] for i in range(len(z))], dtype=np.float32)
    assert same_bits(got, want)
    # the invariants: lam = 0 returns z's bits for every q that is not NaN; a NaN q returns z at every lam
    at0, nan_q = (lam == 0.0) & ~np.isnan(q), np.isnan(q)
    assert at0.sum() == 3 * (len(qs) - 1) and nan_q.sum() == 3 * len(lams)
    assert same_bits(got[at0], z[at0]) and same_bits(got[nan_q], z[nan_q])
    assert same_bits(want[at0], z[at0]) and same_bits(want[nan_q], z[nan_q])
    # lam = 1 on a finite q returns q's value (z + (-z) ... no: 0 * z + q)
    at1 = (lam == 1.0) & ~np.isnan(q)
    assert np.array_equal(got[at1], q[at1])


def test_mixed_value_targets_refuses_bad_arguments():
    with pytest.raises(ValueError):
        mixed_value_targets([1.0], [0.5], 1.5)
    with pytest.raises(ValueError):
        mixed_value_targets([1.0], [0.5], float('nan'))
    with pytest.raises(ValueError):
        mixed_value_targets([1.0, 0.0], [0.5], 0.5)


# ----------------------------------------------------------------------------------------------- the root value
def test_root_value_is_minus_w_over_n(drv):
    rs = np.random.RandomState(3)
    n = np.concatenate([[0, 0, 1, 1, 800, 2 ** 31 - 1], rs.randint(1, 5000, size=500)]).astype(np.int32)
    w = np.concatenate([[0.0, 3.5, -1.0, 1.0, 123.456, -7.0], rs.uniform(-1.0, 1.0, size=500) * n[6:]]).astype(np.float64)
    v, ring, stat = drv.run('vroot', [], [n, w], [np.float64, np.float32, np.float64])
    want = np.array([-(wi / ni) if ni > 0 else float('nan') for ni, wi in zip(n.tolist(), w.tolist())], dtype=np.float64)
    assert same_bits(v, want)
    assert np.isnan(v[:2]).all() and not np.isnan(v[2:]).any()
    assert same_bits(ring, want.astype(np.float32))
    inside = ~np.isnan(want) & (want >= -2.0)   # resign_rule sees the same value: its statistic is max(v_root, q_best = -2)
    assert same_bits(stat[inside], want[inside]) and np.isnan(stat[np.isnan(want)]).all()


def test_a_refreshed_value_is_written_only_for_a_slot_and_a_number(drv):
    slot = np.array([-1, 0, 5, 63, 64, 1 << 40, 3, 3], dtype=np.int64)
    v = np.array([0.5, 0.5, -1.0, 0.0, 0.5, 0.5, np.nan, -0.0], dtype=np.float64)
    got, = drv.run('written', [64], [slot, v], [np.int32])
    assert got.tolist() == [0, 1, 1, 1, 0, 0, 0, 1]


# ----------------------------------------------------------------------------------------------- the reader of the side ring
def _side_rows(log, q_of, junk=7.0):
    """The side ring a device would write beside ``log`` [R, G, words]: for a SEARCHED record the root value of (game, ply); for the
    later records of a stalled ply -- still stalled, or resolved -- ``junk`` (the device repeats the value there; the reader must not
    take it from them); NaN for an idle slot."""
    R, G = log.shape[:2]
    side = np.full((R, G), np.nan, dtype=np.float32)
    for r in range(R):
        for g in range(G):
            flags = int(log[r, g, 4])
            if not flags & PLAY_RUNNING:
                continue
            gid = int(np.ascontiguousarray(log[r, g, 0:2]).view(np.int64)[0])
            side[r, g] = q_of[gid][int(log[r, g, 2])] if flags & PLAY_SEARCHED else junk
    return side


def _script():
    cfg = Cfg(resign=(-0.8, 0.3))
    from test_playlog_host import PLAYED
    rng = np.random.RandomState(17)
    games = [Game(cfg, rng, PLAYED[0], 5, 0, stalls=(2, )), Game(cfg, rng, PLAYED[1], 4, -1, resign=True),
             Game(cfg, rng, PLAYED[2], 6, 1, stalls=(0, 5)), Game(cfg, rng, PLAYED[3], 3, 0), Game(cfg, rng, PLAYED[4], 7, 1, stalls=(3, ))]
    q_of = dict((g.gid, rng.uniform(-1.0, 1.0, size=len(g.counts)).astype(np.float32)) for g in games)
    return cfg, games, q_of


@pytest.mark.parametrize('delay', [1, 3])
def test_reader_forms_root_values_from_the_side_ring(delay):
    """A scripted log with stalled-then-resolved plies and a resignation, read row by row with its side ring: root_values has the
    length of moves, every ply carries the value of its SEARCHED record -- a stalled ply too --, the resigning search is not recorded,
    and the games are those of a reader that never heard of the ring."""
    cfg, games, q_of = _script()
    w = Writer(cfg, games, 2, delay)
    reader, plain = cfg.reader(w.resolve, 2), cfg.reader(lambda s, m: None, 2)
    reader.root_values_on = True
    out, out_plain = [], []
    while w.busy():
        row = w.step()[None]
        out.extend(reader.read_rows(row, values=_side_rows(row, q_of))[0])
        out_plain.extend(plain.read_rows(row)[0])
    assert sorted(t.game_id for t in out) == sorted(g.gid for g in games)
    stalled_seen = 0
    for t in out:
        g = next(g for g in games if g.gid == t.game_id)
        assert t.moves == g.moves and t.root_values.dtype == np.float32 and len(t.root_values) == len(t.moves)
        assert same_bits(t.root_values, q_of[g.gid][:len(g.moves)])
        assert len(q_of[g.gid]) == len(g.moves) + (1 if g.resigned else 0)
        stalled_seen += len(g.stalls)
    assert stalled_seen == 4 and reader.stalls_resolved == 4 and any(t.resigned for t in out)
    for t, p in zip(sorted(out, key=lambda t: t.game_id), sorted(out_plain, key=lambda t: t.game_id)):
        assert p.root_values is None and t.moves == p.moves and t.winner == p.winner and same_bits(t.pis, p.pis)
        assert same_bits(t.resign_stats, p.resign_stats)
    # the whole log at once, stalls already answered in it: the same values
    log = np.stack(w.rows)
    again = cfg.reader(lambda s, m: None, 2)
    again.root_values_on = True
    whole = again.read_rows(log, values=_side_rows(log, q_of))[0]
    for t, u in zip(sorted(out, key=lambda t: t.game_id), sorted(whole, key=lambda t: t.game_id)):
        assert t.moves == u.moves and same_bits(t.root_values, u.root_values)
    assert (log[..., 4] & PLAY_STALLED).any() and (log[..., 4] & PLAY_RESOLVED).any()


def test_reader_refuses_rows_without_their_side_ring():
    cfg, games, q_of = _script()
    w = Writer(cfg, games, 2)
    reader = cfg.reader(w.resolve, 2)
    reader.root_values_on = True
    row = w.step()[None]
    with pytest.raises(ValueError):
        reader.read_rows(row)
    with pytest.raises(ValueError):
        reader.read_rows(row, values=np.zeros((1, 3), dtype=np.float32))


# ----------------------------------------------------------------------------------------------- the host route
def _trajectory(root_values=True, full=None, game='gomoku'):
    rs = np.random.RandomState(1)
    if game == 'connect4':
        board, moves, A = (4, 5), [0, 1, 0, 1, 2, 3, 2, 4, 4, 0], 5
    else:
        board, moves, A = 6, [0, 7, 14, 3, 21, 9, 28, 30, 35], 36
    P = len(moves)
    pis = rs.dirichlet(np.ones(A), size=P)
    q = rs.uniform(-1.0, 1.0, size=P).astype(np.float32) if root_values else None
    return Trajectory(5, board, 4, moves, pis, 0, game=game, full=full, root_values=q)


@pytest.mark.parametrize('game', ['gomoku', 'connect4'])
@pytest.mark.parametrize('lam', [0.25, 1.0])
def test_training_samples_mix_the_value_target(game, lam):
    t = _trajectory(game=game)
    plain = t.training_samples()
    mixed = t.training_samples(value_mix=lam)
    want = mixed_value_targets(t.z(), t.root_values, lam)
    assert len(mixed) == len(plain) == len(t.moves)
    assert same_bits(np.array([sm[2] for sm in mixed], dtype=np.float32), want)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(np.array([sm[2] for sm in mixed], dtype=np.float64), t.z())


def test_training_samples_without_values_or_mix_are_todays():
    for t in (_trajectory(), _trajectory(root_values=False)):
        plain = t.training_samples()
        for lam in ((0.0, ) if t.root_values is not None else (0.0, 0.5)):
            same = t.training_samples(value_mix=lam)
            assert len(same) == len(plain)
            for a, b in zip(plain, same):
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and type(a[2]) is type(b[2]) and a[2] == b[2]
    with pytest.raises(ValueError):
        _trajectory().training_samples(value_mix=1.5)


def test_training_samples_under_a_cap_keep_the_full_plies_values():
    full = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1], dtype=bool)
    t = _trajectory(full=full)
    mixed = t.training_samples(value_mix=0.5)
    assert len(mixed) == int(full.sum())
    assert same_bits(np.array([sm[2] for sm in mixed], dtype=np.float32), mixed_value_targets(t.z(), t.root_values, 0.5)[full])
    assert same_bits(kept_root_values([t, _trajectory(root_values=False)]),
                     np.concatenate([t.root_values[full], np.full(9, np.nan, dtype=np.float32)]))


def test_trajectory_refuses_values_of_another_length():
    with pytest.raises(ValueError):
        Trajectory(0, 6, 4, [0, 1, 2], np.full((3, 36), 1.0 / 36), -1, root_values=[0.1, 0.2])


# ----------------------------------------------------------------------------------------------- the trainer's parser
def test_trainer_refuses_the_value_mix_on_several_ranks(monkeypatch):
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import train_alphazero
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(ValueError, match='one rank'):
        train_alphazero.main(['--games-in-flight', '4', '--value-mix', '0.5', '--gpus', '2'])
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='one rank'):
        train_alphazero.main(['--games-in-flight', '4', '--value-mix', '0.5'])
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for bad in (['--value-mix', '0.5'], ['--games-in-flight', '4', '--value-mix', '1.5'],
                ['--games-in-flight', '4', '--reanalyse-targets', 'value'],
                ['--games-in-flight', '4', '--device-replay', '--reanalyse', '8', '--reanalyse-targets', 'both']):
        with pytest.raises(SystemExit):
            train_alphazero.parse_args(bad)
    args = train_alphazero.parse_args(['--games-in-flight', '4'])
    assert train_alphazero.value_mix_of(args) == 0.0 and train_alphazero.reanalyse_targets_of(args) == 'pi'
    args = train_alphazero.parse_args(['--games-in-flight', '4', '--value-mix', '0.25'])
    assert train_alphazero.value_mix_of(args) == 0.25
