"""Forced playouts and policy target pruning without a GPU: rlzero_amd/csrc/rz_forced.h -- the two rules the kernels call -- against
their Python statement, tests/forced_twin.py, bit for bit; the twin itself on the cases the GPU tests use (the rule must be live
there, or bit equality with the device would show nothing); the ABI text; the refusals on the Python side and the trainer's flags.

A driver with its own main is compiled against the header with ROCm's clang++ -- without fused contraction, as the library is -- and
once more with -fsanitize=address,undefined (a stand-alone program); every call runs both and holds their outputs equal."""
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import forced_twin as ft
import host_driver
from host_driver import CSRC
from oracle.gomoku_ref import RefGomoku
from oracle.mcts_ref import RefSearch, tree_dump
from rlzero_amd import _hip
from test_gpu_parity import _skewed

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "rz_forced.h"

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

// forced n.i32 [m] p.f32 [m] N.i32 [m] k.f64 [m] -> forced.i32 [m]
static int forced(char **a) {
    const std::vector<int32_t> n = load<int32_t>(a[0]), N = load<int32_t>(a[2]);
    const std::vector<float> p = load<float>(a[1]);
    const std::vector<double> k = load<double>(a[3]);
    if (p.size() != n.size() || N.size() != n.size() || k.size() != n.size()) return 4;
    std::vector<int32_t> out(n.size());
    for (size_t i = 0; i < n.size(); ++i) out[i] = rzf::forced(n[i], p[i], N[i], k[i]) ? 1 : 0;
    store(a[4], out);
    return 0;
}

// pruned first.i32 [R + 1] n.i32 [M] w.f64 [M] p.f32 [M] N.i32 [R] k.f64 [R] c.f64 [R] -> counts.i32 [M] best.i32 [R]
// (root r: the children first[r] .. first[r + 1] - 1, in rank order)
static int pruned(char **a) {
    const std::vector<int32_t> first = load<int32_t>(a[0]), n = load<int32_t>(a[1]), N = load<int32_t>(a[4]);
    const std::vector<double> w = load<double>(a[2]), k = load<double>(a[5]), c = load<double>(a[6]);
    const std::vector<float> p = load<float>(a[3]);
    const size_t R = N.size();
    if (first.size() != R + 1 || k.size() != R || c.size() != R || w.size() != n.size() || p.size() != n.size()) return 4;
    if (first[0] != 0 || (size_t)first[R] != n.size()) return 4;
    std::vector<int32_t> out(n.size()), best(R);
    for (size_t r = 0; r < R; ++r) {
        const int at = first[r], K = first[r + 1] - first[r];
        if (K < 1) return 4;
        best[r] = rzf::best_child(n.data() + at, K);
        rzf::pruned_counts(n.data() + at, w.data() + at, p.data() + at, K, N[r], std::sqrt((double)N[r]), k[r], c[r], out.data() + at);
    }
    store(a[7], out);
    store(a[8], best);
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "forced" && argc == 7) return forced(argv + 2);
    if (what == "pruned" && argc == 11) return pruned(argv + 2);
    return 4;
}
'''


driver = host_driver.fixture('forced', DRIVER)


def forced(driver, n, p, N, k):
    return driver.run('forced', [], [np.asarray(n, np.int32), np.asarray(p, np.float32), np.asarray(N, np.int32), np.asarray(k, np.float64)],
                      [np.int32])[0]


def pruned(driver, roots):
    """roots: [(n list, w list, p list, N, k, c)] -> ([counts per root], [best child per root])."""
    first = np.cumsum([0] + [len(r[0]) for r in roots]).astype(np.int32)
    cat = lambda i, dt: np.concatenate([np.asarray(r[i], dtype=dt) for r in roots])   # noqa: E731
    out, best = driver.run('pruned', [], [first, cat(0, np.int32), cat(1, np.float64), cat(2, np.float32), np.asarray([r[3] for r in roots], np.int32),
                                          np.asarray([r[4] for r in roots], np.float64), np.asarray([r[5] for r in roots], np.float64)],
                           [np.int32, np.int32])
    return [out[a:b].tolist() for a, b in zip(first[:-1], first[1:])], best.tolist()


def twin_pruned(root):
    n, w, p, N, k, c = root
    return ft.pruned_counts([int(x) for x in n], [float(x) for x in w], [np.float32(x) for x in p], int(N), float(k), float(c))


def first_best(n):
    return max(range(len(n)), key=lambda r: (n[r], -r))


# ------------------------------------------------------------------ the header against the twin
def random_roots(rs, count):
    """Roots as a search leaves them: 1 to 225 children, float32 priors that sum to about one, a few children holding most visits,
    value sums within [-n, n], N = the children's visits + 1 (a fresh root) or more (a kept subtree); k and c from a few values."""
    roots = []
    for _ in range(count):
        K = int(rs.randint(1, 226))
        p = rs.dirichlet(np.full(K, 0.3 if rs.rand() < 0.5 else 3.0)).astype(np.float32)
        total = int(rs.choice([3, 20, 80, 300, 1600]))
        n = rs.multinomial(total, rs.dirichlet(np.full(K, 0.2))).astype(np.int32)
        if rs.rand() < 0.3:   # (ties on the largest count, single playouts)
            n[rs.randint(K)] = n.max()
            n[rs.randint(K)] = 1
        w = np.where(rs.rand(K) < 0.5, rs.randint(-8, 9, K) / 8.0, rs.uniform(-1, 1, K)) * n
        N = int(n.sum()) + int(rs.choice([1, 1, 7]))
        roots.append((n, w, p, N, float(rs.choice([2.0, 0.5, 1.7, 8.0, 1e-3])), float(rs.choice([5.0, 1.5, 3.0, 0.0]))))
    return roots


def test_header_equals_twin_on_random_roots(driver):
    rs = np.random.RandomState(5)
    roots = random_roots(rs, 3000)
    got, best = pruned(driver, roots)
    lowered = zeroed = 0
    for root, g, b in zip(roots, got, best):
        assert g == twin_pruned(root)
        assert b == first_best(root[0].tolist())
        lowered += sum(1 for x, y in zip(g, root[0]) if x < y)
        zeroed += sum(1 for x, y in zip(g, root[0]) if x == 0 and y > 0)
    assert lowered > 1000 and zeroed > 100   # (the rule was at work)
    # forced(): every child of every root, under the root's k
    n = np.concatenate([r[0] for r in roots])
    p = np.concatenate([r[2] for r in roots])
    N = np.concatenate([np.full(len(r[0]), r[3]) for r in roots])
    k = np.concatenate([np.full(len(r[0]), r[4]) for r in roots])
    got_f = forced(driver, n, p, N, k)
    want_f = [1 if ft.forced(int(a), b, int(c), float(d)) else 0 for a, b, c, d in zip(n, p, N, k)]
    assert got_f.tolist() == want_f and 0 < sum(want_f) < len(want_f)


def test_forced_at_the_threshold(driver):
    """n n against (k p) N where they are equal, and one unit in the last place to either side (k is a double: a neighbour of 2 moves
    the product 2 * 0.5 * 16 = 16 by one ulp); a float32 neighbour of p; n = 0 is never forced."""
    up, down = math.nextafter(2.0, 3.0), math.nextafter(2.0, 0.0)
    p_up = np.nextafter(np.float32(0.5), np.float32(1.0))
    rows = [(4, 0.5, 16, 2.0, 0), (4, 0.5, 16, up, 1), (4, 0.5, 16, down, 0), (4, p_up, 16, 2.0, 1), (3, 0.5, 16, 2.0, 1), (5, 0.5, 16, 2.0, 0),
            (0, 0.5, 16, 2.0, 0), (0, 1.0, 1000, 8.0, 0), (1, 0.125, 4, 2.0, 0), (1, 0.125, 5, 2.0, 1), (2, 0.125, 16, 2.0, 0),
            (46340, 1.0, 2147483647, 1.0, 1), (46341, 1.0, 2147483647, 1.0, 0)]   # (46341^2 = 2147488281 > 2^31 - 1: squared as doubles)
    assert (2.0 * 0.5) * 16.0 == 16.0 and (up * 0.5) * 16.0 == math.nextafter(16.0, 17.0) and (down * 0.5) * 16.0 == math.nextafter(16.0, 0.0)
    got = forced(driver, *[[r[i] for r in rows] for i in range(4)])
    assert got.tolist() == [r[4] for r in rows]
    assert [1 if ft.forced(r[0], np.float32(r[1]), r[2], r[3]) else 0 for r in rows] == [r[4] for r in rows]
    # what a rule with <= would answer at the equalities
    assert [ft.forced(r[0], np.float32(r[1]), r[2], r[3], strict=False) for r in rows[:1] + rows[8:9] + rows[10:11]] == [True] * 3


def test_pruning_crafted_roots(driver):
    """Each root: (n, w, p, N, k, c) -> the counts wanted, worked out by hand below."""
    cases = [
        # the subtraction stops exactly at the score tie: S* = (0.5 * 4) / 8 = 0.25; the second child (q = 0, p = 0.25) scores
        # 1 / m at count m - 1: below 0.25 at m = 6, 5 and EQUAL at m = 4; f = 4 (4 * 4 <= (4 * 0.25) * 16) would allow more
        (([7, 6], [0.0, 0.0], [0.5, 0.25], 16, 4.0, 1.0), [7, 4]),
        # ... and stops at f = 2 first under k = 2 (2 * 2 <= 8 < 3 * 3): 6 -> 4 all the same, with a third child untouched by f = 0
        (([7, 6, 3], [0.0, 0.0, 0.0], [0.5, 0.25, 0.01], 16, 2.0, 1.0), [7, 4, 3]),
        # f = 0 ((k p) N = 0.32 < 1): nothing is subtracted, however low the child scores
        (([9, 5], [0.0, -5.0], [0.9, 0.01], 16, 2.0, 1.0), [9, 5]),
        # the best child tied on n: the FIRST one is the best and keeps its count; the second (q = -1, far below S* > 0) is pruned
        # against it and loses the f = 2 playouts it may lose (2 * 2 <= (2 * 0.4) * 11 = 8.8 < 3 * 3)
        (([5, 5, 0], [0.0, -5.0, 0.0], [0.4, 0.4, 0.2], 11, 2.0, 1.0), [5, 3, 0]),
        # 2 -> 1 -> 0: one playout is subtracted (f = 1: 1 <= (2 * 0.05) * 16 = 1.6 < 4), the single one left is dropped
        (([9, 2], [0.0, -2.0], [0.9, 0.05], 16, 2.0, 1.0), [9, 0]),
        # one unsubtracted visit (f = 0) becomes 0 as well; a child with n = 0 stays 0
        (([9, 1, 0], [0.0, 1.0, 0.0], [0.9, 0.01, 0.09], 16, 2.0, 1.0), [9, 0, 0]),
        # a single child, and a best child with one visit: both keep their counts
        (([1], [0.5], [1.0], 2, 2.0, 5.0), [1]),
        (([1, 1], [0.5, -1.0], [0.5, 0.5], 3, 2.0, 5.0), [1, 0]),
        # nothing visited
        (([0, 0], [0.0, 0.0], [0.5, 0.5], 1, 2.0, 5.0), [0, 0]),
        # a huge k: f is capped by n, the loop by m > 0 -- the child loses everything it may lose
        (([9, 4], [0.0, -4.0], [0.9, 0.1], 16, 1e300, 1.0), [9, 0]),
    ]
    got, best = pruned(driver, [c[0] for c in cases])
    for (root, want), g, b in zip(cases, got, best):
        assert twin_pruned(root) == want, root
        assert g == want, root
        assert b == first_best(root[0])
    # the same roots under a rule with <= (the tie is subtracted through) and without the singleton rule
    tie = cases[0][0]
    assert ft.pruned_counts(tie[0], tie[1], [np.float32(x) for x in tie[2]], tie[3], tie[4], tie[5], strict=False) == [7, 3]   # (1 / 4 <= 0.25 goes, 1 / 3 does not)
    single = cases[5][0]
    assert ft.pruned_counts(single[0], single[1], [np.float32(x) for x in single[2]], single[3], single[4], single[5], singleton=False) == [9, 1, 0]


# ------------------------------------------------------------------ the twin on the cases the GPU tests use
def twin_search(case, evaluator=_skewed, **kw):
    """-> (the search after its first move's simulations, a deep copy of nothing: the tree dump and the pruned counts of move one,
    then the same after the move to the most visited child with the kept subtree -- None where the game ended)."""
    B, n, pre, sims, c = case
    env = RefGomoku.from_moves(B, n, pre)
    s = ft.ForcedSearch(evaluator, sims, c, ft.K, **kw)
    s.simulate(env, 1.0)
    out = [(tree_dump(s.root), [kid.n for kid in s.root.kids], ft.pruned_root(s.root, ft.K, c), s.forced_selections, s.root)]
    best = s.root.acts[first_best([kid.n for kid in s.root.kids])]
    s.update_with_move(best)
    env.step(best)
    if not env.game_end_winner()[0]:
        s.simulate(env, 1.0)
        out.append((tree_dump(s.root), [kid.n for kid in s.root.kids], ft.pruned_root(s.root, ft.K, c), s.forced_selections, s.root))
    return out


@pytest.fixture(scope='module')
def twin_runs():
    return [twin_search(case) for case in ft.CASES]


# root selections the forced rule decided, root children whose count pruning lowers, of those set to 0 -- move one of each case
TABLE = [(20, 3, 1), (52, 6, 3), (51, 24, 10), (73, 55, 24), (56, 43, 24)]


def test_the_rule_is_live_on_the_gpu_cases(twin_runs):
    """Forced selections > 0, a tree other than plain PUCT's, at least one child lowered and one set to 0 -- and the figures of the
    table the cases were chosen by."""
    for case, runs, row in zip(ft.CASES, twin_runs, TABLE):
        B, n, pre, sims, c = case
        dump, raw, pruned, hits, root = runs[0]
        plain = RefSearch(_skewed, sims, c, score_mode='puct')
        plain.simulate(RefGomoku.from_moves(B, n, pre), 1.0)
        lowered = [a for a, x in zip(root.acts, raw) if pruned[a] < x]
        zeroed = [a for a in lowered if pruned[a] == 0]
        assert hits > 0 and dump != tree_dump(plain.root) and lowered and zeroed
        assert (hits, len(lowered), len(zeroed)) == row
        assert sum(pruned.values()) > 0 and sum(raw) == root.n - 1
    # 9 x 9 and 11 x 11 have more than 64 root children (two per lane of the device's scan); WIDE_CASE has more than 128 (three)
    assert 64 < len(twin_runs[3][0][1]) <= 128 and 64 < len(twin_runs[4][0][1]) <= 128
    B, n, pre, sims, c = ft.WIDE_CASE
    wide = twin_search(ft.WIDE_CASE)
    plain = RefSearch(_skewed, sims, c, score_mode='puct')
    plain.simulate(RefGomoku.from_moves(B, n, pre), 1.0)
    dump, raw, pruned, hits, root = wide[0]
    assert len(raw) > 128 and hits > 0 and dump != tree_dump(plain.root)
    assert any(pruned[a] < x for a, x in zip(root.acts, raw)) and any(pruned[a] == 0 < x for a, x in zip(root.acts, raw))
    assert any(x > 0 for x in raw[128:])   # (a visited child in the third slot of a lane)
    assert all(len(runs) == 2 for runs in twin_runs[1:])   # (the second move with the kept subtree exists)


def test_what_a_wrong_rule_changes_on_the_gpu_cases(twin_runs):
    """What the bit comparison with the device catches.  The sum of the children's visits for N and a missing singleton rule give
    other counts on the five cases.  A rule with <= for < cannot be told apart there -- n n never EQUALS (k p) N with those priors --
    so the GPU tests add TIE_CASE, where it builds another tree."""
    diff_sum = diff_single = 0
    for case, runs in zip(ft.CASES, twin_runs):
        c = case[4]
        for dump, raw, pruned, hits, root in runs:
            diff_sum += ft.pruned_root(root, ft.K, c, n_of='sum') != pruned
            diff_single += ft.pruned_root(root, ft.K, c, singleton=False) != pruned
    assert diff_sum >= 1 and diff_single >= len(ft.CASES)
    good, bad = twin_search(ft.TIE_CASE, ft.uniform32), twin_search(ft.TIE_CASE, ft.uniform32, strict=False)
    assert good[0][0] != bad[0][0] and good[0][3] > 0
    plain = RefSearch(ft.uniform32, ft.TIE_CASE[3], ft.TIE_CASE[4], score_mode='puct')
    plain.simulate(RefGomoku.from_moves(*ft.TIE_CASE[:3]), 1.0)
    assert good[0][0] != tree_dump(plain.root)


# ------------------------------------------------------------------ the ABI, the refusals, the trainer's flags
def test_header_declares_the_entries_and_the_binding_matches():
    header = open(os.path.join(REPO, 'include', 'rlzero_hip.h')).read()
    assert '#define RZ_ABI_VERSION %d' % _hip.ABI_VERSION in header and _hip.ABI_VERSION >= 47
    for name, args in (('rz_set_forced_playouts', 2), ('rz_root_pruned_visits', 3), ('rz_play_set_pruned_visits', 3)):
        m = re.search(r'int %s\(([^)]*)\);' % name, header)
        assert m is not None and len(m.group(1).split(',')) == args
        assert len(_hip._SIGNATURES[name][1]) == args
    text = header[header.index('FORCED PLAYOUTS AND POLICY TARGET PRUNING'):header.index('int rz_set_forced_playouts')]
    assert 'ABI 47' in text and 'attach again' in text and 'RZ_SCORE_PUCT' in text
    engine = open(os.path.join(CSRC, 'rz_engine.hip')).read()
    setter = engine[engine.index('int rz_set_forced_playouts'):engine.index('int rz_root_pruned_visits')]
    for reason in ('RZ_SCORE_PUCT', 'one simulation in flight', 'a match is on', 'not a finite number', 'attach again'):
        assert reason in setter and 'RZ_ERR_ARG' in setter


class _FakeEngine(object):
    def __init__(self, score_mode=_hip.SCORE_PUCT, sims_in_flight=1):
        self.score_mode, self.sims_in_flight, self.forced_k, self.play_match_on = score_mode, sims_in_flight, 0.0, False


class _FakeLane(object):
    def __init__(self, eng, evaluator=None):
        self.eng, self.evaluator = eng, evaluator


def _fake_selfplay(**kw):
    from rlzero_amd.selfplay import BatchedSelfPlay
    sp = BatchedSelfPlay.__new__(BatchedSelfPlay)
    sp.lanes = [_FakeLane(_FakeEngine(**kw))]
    sp.playout_cap, sp.forced_k, sp.forced_prune = None, 0.0, True
    return sp


def test_selfplay_refusals():
    from rlzero_amd.engine import RolloutEvaluator
    with pytest.raises(ValueError, match='uct_ref'):
        _fake_selfplay(score_mode=_hip.SCORE_UCT_REF).set_forced_playouts(2.0)
    with pytest.raises(ValueError, match='one simulation in flight'):
        _fake_selfplay(sims_in_flight=4).set_forced_playouts(2.0)
    sp = _fake_selfplay()
    sp.playout_cap = (10, 0.25)
    with pytest.raises(ValueError, match='playout cap'):
        sp.set_forced_playouts(2.0)
    sp = _fake_selfplay()
    sp.lanes[0].evaluator = RolloutEvaluator()
    with pytest.raises(ValueError, match='priors'):
        sp.set_forced_playouts(2.0)
    sp = _fake_selfplay()
    sp._streaming = True
    with pytest.raises(ValueError, match='stream'):
        sp.set_forced_playouts(2.0)
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='finite'):
            _fake_selfplay().set_forced_playouts(bad)
    # ... and the other way round: with forced playouts on, no playout cap and no stream
    sp = _fake_selfplay()
    sp.forced_k = 2.0
    with pytest.raises(ValueError, match='forced playouts'):
        sp.set_playout_cap(10, 0.25)
    with pytest.raises(ValueError, match='forced playouts'):
        sp.stream_start()


def test_reader_needs_the_pruned_rows():
    from rlzero_amd.selfplay import SelfPlayReader
    reader = SelfPlayReader(2, 9, 9, 10, (3, 3, 'gomoku'), lambda slot, move: None)
    reader.forced_k = 2.0
    with pytest.raises(ValueError, match='pruned'):
        reader.read_rows(np.zeros((1, 2, _hip.PLAY_RECORD_WORDS + 9), dtype=np.int32))


def test_trainer_flag_errors():
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import train_alphazero as ta
    base = ['--games-in-flight', '8', '--score-mode', 'puct']
    for extra, reason in ((['--playout-cap', '10:0.25'], 'playout-cap'), (['--device-replay', '--reanalyse', '64'], 'reanalyse'),
                          (['--continuous-selfplay'], 'continuous-selfplay')):
        if '--device-replay' in extra:   # (parse_args asks for a GPU with --device-replay: the rule itself is check_puct_options')
            with pytest.raises(ValueError, match=reason):
                ta.check_puct_options('puct', False, None, 8, None, 64, False)
            continue
        with pytest.raises(ValueError, match=reason):
            ta.main(base + extra)
    with pytest.raises(ValueError, match='score-mode puct'):
        ta.main(['--games-in-flight', '8', '--forced-playouts', '2'])
    with pytest.raises(ValueError, match='score-mode puct'):
        ta.main(['--games-in-flight', '8', '--resident-puct'])
    with pytest.raises(ValueError, match='games-in-flight'):
        ta.main(['--score-mode', 'puct'])
    with pytest.raises(ValueError, match='K > 0'):
        ta.main(base + ['--forced-playouts', '0'])
    args = ta.parse_args(base + ['--resident-puct', '--forced-playouts', '2'])
    assert ta.puct_options_of(args) == ('puct', True, 2.0)
    assert ta.puct_options_of(ta.parse_args([])) == ('uct_ref', False, None)   # (absent from the namespace unless given, like --value-mix)
    assert not {'score_mode', 'resident_puct', 'forced_playouts'} & set(vars(ta.parse_args([])))
    ta.check_puct_options('puct', True, 2.0, 8, None, None, False)   # (several ranks are served: nothing about them here)
    with pytest.raises(ValueError, match='uct_ref or puct'):
        ta.check_puct_options('ucb', False, None, 8, None, None, False)
