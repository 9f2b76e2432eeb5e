"""The host restatements of the device noise streams (tests/device_streams.py) on their own, without a GPU: they ARE the
distributions they claim to be, on the keys the device's schedules really use; no counter is hashed twice inside a node; the draws
that the schedules place next to each other are uncorrelated; and the figures behind the floor of the MuZero draw.

Bounds are derived, not tuned: the Kolmogorov statistic of N samples of the right distribution exceeds 1.95 / sqrt(N) with
probability 0.1 %; the sample correlation of N independent pairs has standard deviation 1 / sqrt(N) (|r| <= 4 / sqrt(N))."""
import math

import numpy as np
import pytest

import device_streams as ds

N_KS = 1 << 20
N_PAIRS = 1 << 18


# ---------------------------------------------------------------------------------------------------------------------- hashes
def test_hashes_are_the_sources():
    """mix64 against rz_rng.h, which rz_play.h names as rzplay::mix64 (the constants are read out of the header, the function evaluated
    with Python integers), hash32 against rz_tree.h, splitmix64 = mix64 (one definition, two names on the device)."""
    import glob
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rlzero_amd', 'csrc')
    assert 'using rzrng::mix64;' in open(os.path.join(csrc, 'rz_play.h')).read()
    play = open(os.path.join(csrc, 'rz_rng.h')).read()
    body = play[play.index('uint64_t mix64(uint64_t x)'):]
    body = body[:body.index('}')]
    inc, m1, m2 = (int(c, 16) for c in re.findall(r'0x([0-9A-Fa-f]{16})ull', body))
    s1, s2, s3 = (int(c) for c in re.findall(r'z >> (\d+)', body))
    M = (1 << 64) - 1

    def mix_py(x):
        z = (x + inc) & M
        z = ((z ^ (z >> s1)) * m1) & M
        z = ((z ^ (z >> s2)) * m2) & M
        return z ^ (z >> s3)

    tree = open(os.path.join(csrc, 'rz_tree.h')).read()
    hbody = tree[tree.index('uint32_t hash32(uint32_t x)'):]
    hbody = hbody[:hbody.index('}')]
    k1, k2 = (int(c, 16) for c in re.findall(r'x \*= 0x([0-9a-f]{8})u', hbody))
    h1, h2, h3 = (int(c) for c in re.findall(r'x \^= x >> (\d+)', hbody))

    def hash_py(x):
        x ^= x >> h1
        x = (x * k1) & 0xFFFFFFFF
        x ^= x >> h2
        x = (x * k2) & 0xFFFFFFFF
        return x ^ (x >> h3)

    xs = [0, 1, 3, 0x9E3779B9, 0xFFFFFFFF, 0x123456789ABCDEF0, M, 1 << 63, 11 ^ (5 << 20)]
    assert [int(v) for v in ds.mix64(np.array(xs, dtype=np.uint64))] == [mix_py(x) for x in xs]
    assert [int(v) for v in ds.splitmix64(np.array(xs, dtype=np.uint64))] == [mix_py(x) for x in xs]
    assert [int(v) for v in ds.hash32(np.array([x & 0xFFFFFFFF for x in xs], dtype=np.uint64))] == [hash_py(x & 0xFFFFFFFF) for x in xs]
    # ... and the noise constants of the three copies of the mix and of the MuZero key are the ones restated here
    # (the MuZero translation unit: the source and its family headers -- mz_gamma lies in rz_muzero_noise.h, the action draw's salt
    # in the two kernels that draw a move; every count below is over the whole unit)
    noise = open(os.path.join(csrc, 'rz_muzero_noise.h')).read()
    muzero = ''.join(open(p).read() for p in [os.path.join(csrc, 'rz_muzero.hip')] + sorted(glob.glob(os.path.join(csrc, 'rz_muzero_*.h'))))
    assert noise in muzero and 'float mz_gamma(float alpha, uint32_t key)' in noise
    assert tree.count('0x9E3779B9u * (uint32_t)(64 * j + lane + 1)') == 1

    def copies(name):
        text = open(os.path.join(csrc, name)).read()
        return text.count('0x9E3779B9u * (uint32_t)(64 * j + lane + 1)') + text.count('0x9E3779B9u * (uint32_t)(64 * i + lane + 1)')

    # (one in deferred_priors_body, one in the level-synchronous step -- and none anywhere else in the engine's translation unit)
    assert copies('rz_engine_deferred.h') == 1 and copies('rz_engine_ml.h') == 1
    assert copies('rz_engine.hip') + sum(copies(p) for p in glob.glob(os.path.join(csrc, 'rz_engine_*.h'))) == 2
    rules = open(os.path.join(csrc, 'rz_mz_env.h')).read()   # (the MuZero key has one home, which both of its kernels call)
    assert rules.count('0x9E3779B9u * (uint32_t)(a + 1) + (uint32_t)key') == 1 and '0x9E3779B9u' not in muzero and '0xA5A5A5A5ull' in muzero
    assert tree.count('key + 0x5bd1e995u') == 1 and muzero.count('key + 0x5bd1e995u') == 1 and noise.count('key + 0x5bd1e995u') == 1
    assert '0xA5A5A5A5ull' in open(os.path.join(csrc, 'rz_muzero_search.h')).read() and '0xA5A5A5A5ull' in open(os.path.join(csrc, 'rz_muzero_moves.h')).read()
    # gamma03's constants are literals; its c lies 2.2e-6 below 1 / sqrt(9 d), and the restatement takes the literal
    assert 'const float d = 1.3f - 1.0f / 3.0f, c = %sf;' % ds.GAMMA03_C in tree
    exact = 1.0 / math.sqrt(9.0 * (1.3 - 1.0 / 3.0))
    assert 2.0e-6 < (exact - ds.GAMMA03_C) / exact < 2.4e-6
    assert 'c = 1.0f / sqrtf(9.0f * d)' in muzero and 'c = 1.0f / sqrtf(9.0f * d)' in noise   # (mz_gamma computes its own)


# ---------------------------------------------------------------------------------------------------------------------- schedules
def _alphazero_keys(n, seed=11, children=256, counters=64):
    games = n // (children * counters)
    g, c, a = np.meshgrid(np.arange(games), np.arange(counters), np.arange(children), indexing='ij')
    return ds.alphazero_child_keys(ds.default_noise_key(seed, g.ravel()), c.ravel(), a.ravel())


def _muzero_keys(n, seed=9, A=2, steps=256, episodes=4):
    envs = n // (A * steps * episodes)
    g, e, s = np.meshgrid(np.arange(envs), np.arange(episodes), np.arange(steps), indexing='ij')
    return ds.muzero_action_keys(seed, g.ravel(), e.ravel(), s.ravel(), A).ravel()


def _ks(sample, alpha):
    x = np.sort(np.asarray(sample, dtype=np.float64))
    n = len(x)
    cdf = ds.gamma_cdf(x, alpha)
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n)))


@pytest.mark.parametrize('alpha', [0.3, 0.25, 1.0, 1.5])
def test_marginals_are_gamma(alpha):
    """2^20 keys of the real schedules (AlphaZero: games x counters x children with the default keys, for 0.3; MuZero: environments x
    episodes x steps x actions): the restatement is Gamma(alpha, 1) by Kolmogorov-Smirnov against torch.special.gammainc in float64,
    statistic <= 1.95 / sqrt(N) (the 0.1 % point).  1.0 is the first shape that takes no boost.  The eight rounds always suffice."""
    if alpha == 0.3:
        keys = _alphazero_keys(N_KS)
        sample, rounds, margin = ds.gamma(keys, 0.3, always_boost=True)
    else:
        keys = _muzero_keys(N_KS)
        sample, rounds, margin = ds.gamma(keys, alpha, floor=ds.MZ_FLOOR)
    assert keys.size == N_KS and sample.dtype == np.float64
    stat = _ks(sample, alpha)
    part = slice(0, N_KS // 4)   # (the float32 evaluation on a quarter of the keys: it sizes tolerances, it is not the subject here)
    _, r32, _ = ds.gamma(keys[part], alpha, dtype=np.float32, always_boost=alpha == 0.3, floor=0.0 if alpha == 0.3 else ds.MZ_FLOOR)
    other_branch = float(np.mean(r32 != rounds[part]))
    print('alpha %g: KS %.5f (limit %.5f), fallback taken %d times, rounds up to %d, float32 takes another branch on %.2e of the draws, '
          'margin < 1e-4 on %.2e' % (alpha, stat, 1.95 / math.sqrt(N_KS), int((rounds == ds.ROUNDS).sum()), int(rounds.max()) + 1,
                                     other_branch, float(np.mean(margin < 1e-4))))
    assert stat <= 1.95 / math.sqrt(N_KS)
    assert (rounds < ds.ROUNDS).all()          # the fallback g = d was never taken
    assert other_branch <= 1e-4                 # (what the margin-based exclusion of the GPU tests is for)
    assert np.mean(margin < 1e-4) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------- counters
def test_no_counter_twice_inside_a_node():
    """The 25 counters of a child (8 rounds x 3 uniforms + the boost) and those of every other child of the node are distinct:
    AlphaZero nodes of 256 actions, MuZero nodes of 8 -- exactly, as a set computation (every smaller node is a subset)."""
    g, c = np.meshgrid(np.arange(16), np.arange(64), indexing='ij')
    node = ds.alphazero_node_key(ds.default_noise_key(3, g.ravel()), c.ravel())            # [1024]
    a = np.arange(256, dtype=np.uint64)
    child = (node[:, None] + np.uint64(ds.GOLDEN32) * (a[None, :] + np.uint64(1))) & ds.M32
    ctr = ds.gamma_counters(child).reshape(len(node), -1)
    assert ctr.shape[1] == 256 * 25
    assert all(len(set(row.tolist())) == 256 * 25 for row in ctr)
    g, e, s = np.meshgrid(np.arange(64), np.arange(4), np.arange(64), indexing='ij')
    mz = ds.gamma_counters(ds.muzero_action_keys(9, g.ravel(), e.ravel(), s.ravel(), 8)).reshape(g.size, -1)
    assert mz.shape[1] == 8 * 25
    assert all(len(set(row.tolist())) == 8 * 25 for row in mz)


# ---------------------------------------------------------------------------------------------------------------------- independence
def _r(a, b):
    return float(np.corrcoef(np.log(a), np.log(b))[0, 1])


def _az(seed, g, c, a):
    return ds.gamma(ds.alphazero_child_keys(ds.default_noise_key(seed, g), c, a), 0.3, always_boost=True)[0]


def _mz(seed, g, e, s, alpha=0.25):
    return ds.gamma(ds.muzero_action_keys(seed, g, e, s, 2), alpha, floor=ds.MZ_FLOOR)[0]


def test_draws_next_to_each_other_are_uncorrelated():
    """Where a weak key schedule would show: log-domain correlation of 2^18 pairs, |r| <= 4 / sqrt(N)."""
    limit = 4.0 / math.sqrt(N_PAIRS)
    g, c, a = (x.ravel() for x in np.meshgrid(np.arange(64), np.arange(64), np.arange(64), indexing='ij'))
    assert g.size == N_PAIRS
    base = _az(11, g, c, a)
    got = {
        'children a, a + 1 of a node': _r(base, _az(11, g, c, a + 1)),
        'a child at counters c, c + 1': _r(base, _az(11, g, c + 1, a)),
        'a child and counter in games g, g + 1': _r(base, _az(11, g + 1, c, a)),
    }
    g, e, s = (x.ravel() for x in np.meshgrid(np.arange(512), np.arange(4), np.arange(128), indexing='ij'))
    assert g.size == N_PAIRS
    mz = _mz(9, g, e, s)
    got['MuZero: action 0 at steps s, s + 1'] = _r(mz[:, 0], _mz(9, g, e, s + 1)[:, 0])
    got['MuZero: action 1 at steps s, s + 1'] = _r(mz[:, 1], _mz(9, g, e, s + 1)[:, 1])
    got['MuZero: action 0 across an episode increment'] = _r(mz[:, 0], _mz(9, g, e + 1, s)[:, 0])
    got['MuZero: action 1 across an episode increment'] = _r(mz[:, 1], _mz(9, g, e + 1, s)[:, 1])
    got['MuZero: the two actions of a move'] = _r(mz[:, 0], mz[:, 1])
    for what, r in got.items():
        print('%-48s r = %+.5f (limit %.5f)' % (what, r, limit))
    for what, r in got.items():
        assert abs(r) <= limit, (what, r)


# ---------------------------------------------------------------------------------------------------------------------- the floor
def test_the_floor_of_the_muzero_draw():
    """P_floor(alpha) = P(Gamma(alpha, 1) < 1e-30): 3.5e-8 at 0.25, 1.05e-3 at 0.1, 3.2e-2 at 0.05, 0.128 at 0.03 -- from
    torch.special.gammainc, against the series' first term 1e-30 ^ alpha / Gamma(alpha + 1), and counted on the restatement's own
    draws at 0.1.  With A = 2 actions BOTH draws are floored -- uniform noise where Dirichlet(alpha) is almost one-hot -- with
    probability P_floor^2: 1.2e-15 at 0.25, 1.1e-6 at 0.1 (about one move in 10^6), 1.0e-3 at 0.05, 1.6e-2 at 0.03.  Hence
    rz_mz_play_cartpole and MuZeroSelfPlay refuse alpha < 0.1."""
    want = {0.25: 3.5e-8, 0.1: 1.05e-3, 0.05: 3.2e-2, 0.03: 0.128}
    both = {0.25: 1.2e-15, 0.1: 1.1e-6, 0.05: 1.0e-3, 0.03: 1.6e-2}
    for alpha, p in want.items():
        inc = float(ds.gamma_cdf(np.array([ds.MZ_FLOOR]), alpha)[0])
        series = ds.floor_probability(alpha)
        print('alpha %.2f: P_floor %.4e (series %.4e), both of A = 2 floored %.3e' % (alpha, inc, series, inc ** 2))
        assert abs(inc - series) <= 1e-9 * series
        assert abs(inc - p) <= 0.03 * p
        assert abs(inc ** 2 - both[alpha]) <= 0.06 * both[alpha]
    keys = _muzero_keys(N_KS)
    sample, _, _ = ds.gamma(keys, 0.1, floor=ds.MZ_FLOOR)
    hit = int((sample <= ds.MZ_FLOOR).sum())
    p = ds.floor_probability(float(np.float32(0.1)))
    print('alpha 0.1: %d of %d draws floored (expected %.0f)' % (hit, N_KS, N_KS * p))
    assert abs(hit - N_KS * p) <= 5.0 * math.sqrt(N_KS * p)
    from rlzero_amd.muzero.selfplay import MuZeroSelfPlay
    assert MuZeroSelfPlay.MIN_FUSED_ALPHA == 0.1


# ---------------------------------------------------------------------------------------------------------------------- action draw
def test_action_draw_restatement_edges():
    """muzero_action: T -> 0 takes the first maximum; at T = 1 the draw follows the uniform (u < n0 / total <=> action 0); a zero
    weight in front is skipped; the restatement's fallback is A - 1."""
    vis = np.array([[3, 3], [0, 5], [5, 0], [2, 7]])
    act, gap = ds.muzero_action(9, np.arange(4), np.zeros(4, np.int64), np.zeros(4, np.int64), vis, 0.0)
    assert act.tolist() == [0, 1, 0, 1] and np.isinf(gap).all()
    g = np.arange(4096)
    zeros = np.zeros(4096, np.int64)
    key = ds.muzero_move_key(9, g, zeros, zeros + 7, salt=ds.ACTION_SALT)
    u = (key >> np.uint64(11)).astype(np.float64) / 2.0 ** 53
    act, _ = ds.muzero_action(9, g, zeros, zeros + 7, np.tile([[2, 6]], (4096, 1)), 1.0)
    assert np.array_equal(act == 0, u * 8.0 < 2.0) and 0.2 < np.mean(act == 0) < 0.3
    act, _ = ds.muzero_action(9, g, zeros, zeros + 7, np.tile([[2, 6]], (4096, 1)), 2.0)   # T = 0.5: weights 4, 36
    assert np.array_equal(act == 0, u * 40.0 < 4.0)
    act, _ = ds.muzero_action(9, g, zeros, zeros + 7, np.tile([[0, 4, 0]], (4096, 1)), 1.0)
    assert (act == 1).all()
    other, _ = ds.muzero_action(9, g, zeros + 1, zeros + 7, np.tile([[2, 6]], (4096, 1)), 1.0)   # another episode: another uniform
    again, _ = ds.muzero_action(9, g, zeros, zeros + 7, np.tile([[2, 6]], (4096, 1)), 1.0)
    assert not np.array_equal(other, again) and np.array_equal(again == 0, u * 8.0 < 2.0)


# ---------------------------------------------------------------------------------------------------------------------- GPU cases
def test_gpu_cases_stay_inside_the_exclusion_cap():
    """The GPU tests leave a node out of the sample-by-sample comparison when some child's acceptance margin in the float64
    restatement is below 1e-4, and allow that for at most 10 % of a case's nodes.  Checked here on the CPU for the seeds those tests
    use, on the trees the first search builds under the reference's rule with a constant value while simulations <= children + 1 (the
    root, then its children in order): 1.8e-4 of the draws, i.e. about 1.5 % of the nodes at 81 children and 4 % at 225."""
    import test_noise_streams_gpu as gpu
    for name, case in gpu.AZ_CASES.items():
        cells = case['cells']
        if cells is None or case['sims'] > cells + 1:
            continue
        G, sims, seed = gpu.AZ_GAMES, case['sims'], case['seed']
        keys, ctrs, legal = [], [], []
        for g in range(G):
            for c in range(sims):
                keys.append(ds.default_noise_key(seed, g))
                ctrs.append(c)
                legal.append(np.array([a for a in range(cells) if c == 0 or a != c - 1]))
        _, margins = ds.alphazero_eta_many(np.array(keys), np.array(ctrs), legal)
        out = np.mean([float(m.min()) < gpu.MARGIN for m in margins])
        draws = np.mean(np.concatenate(margins) < gpu.MARGIN)
        print('%s: %.2f %% of %d nodes excluded (%.2e of the draws)' % (name, 100 * out, len(margins), draws))
        assert out <= gpu.EXCLUDED_CAP
    for alpha in gpu.MZ_ALPHAS:
        g, s = np.meshgrid(np.arange(gpu.MZ_ENVS), np.arange(64), indexing='ij')
        _, margin, _ = ds.muzero_eta(gpu.MZ_SEED, g.ravel(), np.zeros(g.size, np.int64), s.ravel(), 2, alpha)
        out = float(np.mean(margin.min(axis=1) < gpu.MARGIN))
        print('MuZero alpha %g: %.3f %% of the moves excluded' % (alpha, 100 * out))
        assert out <= gpu.EXCLUDED_CAP
