"""MuZero prioritized replay on the CPU: the arithmetic, the draws and the search of rlzero_amd/csrc/rz_mz_target.h that k_mzr_prio
and k_mzr_draw_prio call (priority_of, priority_weight, prio_target, prio_filler, upper_bound_u64), BIT FOR BIT against their
Python statements in rlzero_amd/muzero/replay.py (mz_priority_weights, mz_prioritized_draws), with ReplayBuffer._value_target as
the source of the n-step return.  A driver with its own main is compiled against the header with ROCm's clang++ and
-ffp-contract=off, by
tests/host_driver.py, and once more with -fsanitize=address,undefined (a
stand-alone program); every call runs both and holds their outputs equal.  The search is checked EXACTLY, not statistically: every
target 0 .. total - 1 of a small table goes through the driver, and each step is hit as often as it weighs.  Then the learner's
importance weights and the trainer's refusal of --prioritized-replay without --device-replay."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import host_driver
from rlzero_amd.muzero.replay import mz_prioritized_draws, mz_priority_weights, mz_replay_draws
from rlzero_amd.muzero.selfplay import ReplayBuffer
from test_mz_replay_host import CONFIGS, DISCOUNTS, corner, episode_lengths, episodes_of, packed_block, same_bits

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rz_mz_target.h"

namespace rt = rzmzt;

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

// weights td lens.i32 [E] reward.f64 [sum] root.f64 [sum] disc.f64 [td + 1] -> p.f64 [sum] w.i64 [sum]
static int weights(char **a) {
    const int td = atoi(a[0]);
    const std::vector<int32_t> lens = load<int32_t>(a[1]);
    const std::vector<double> reward = load<double>(a[2]), root = load<double>(a[3]), disc = load<double>(a[4]);
    if (reward.size() != root.size() || (int)disc.size() != td + 1) return 4;
    std::vector<double> p;
    std::vector<int64_t> w;
    size_t at = 0;
    for (int32_t len : lens) {
        // (heap copies of exactly `len` doubles: a read past the episode is a report of the sanitized build)
        const std::vector<double> rw(reward.begin() + at, reward.begin() + at + len), rv(root.begin() + at, root.begin() + at + len);
        for (int t = 0; t < len; ++t) {
            p.push_back(rt::priority_of(rw.data(), rv.data(), len, t, td, disc.data()));
            w.push_back((int64_t)rt::priority_weight(p.back()));
        }
        at += (size_t)len;
    }
    if (at != reward.size()) return 4;
    store(a[5], p);
    store(a[6], w);
    return 0;
}

// weigh p.f64 [n] -> w.u64 [n]
static int weigh(char **a) {
    const std::vector<double> p = load<double>(a[0]);
    std::vector<uint64_t> w;
    for (double v : p) w.push_back(rt::priority_weight(v));
    store(a[1], w);
    return 0;
}

// the tables of the device: cum[e] the inclusive prefix inside episode e, ecum the inclusive prefix of the episodes' masses
struct Tables {
    std::vector<std::vector<uint64_t>> cum;
    std::vector<uint64_t> ecum;
    uint64_t total = 0;
};
static Tables tables(const std::vector<int32_t> &lens, const std::vector<int64_t> &w) {
    Tables t;
    size_t at = 0;
    for (int32_t len : lens) {
        std::vector<uint64_t> c;
        uint64_t acc = 0;
        for (int i = 0; i < len; ++i) c.push_back(acc += (uint64_t)w.at(at + i));
        at += (size_t)len;
        t.total += acc;
        t.ecum.push_back(t.total);
        t.cum.push_back(c);
    }
    return t;
}
// k_mzr_draw_prio's two searches for target g -> (episode, position, prob)
static void resolve(const Tables &t, uint64_t g, int64_t *ep, int64_t *pos, double *prob) {
    const int64_t j = rt::upper_bound_u64(t.ecum.data(), (int64_t)t.ecum.size(), g);
    const std::vector<uint64_t> &cum = t.cum.at((size_t)j);
    const int64_t s = rt::upper_bound_u64(cum.data(), (int64_t)cum.size(), g - (j ? t.ecum[(size_t)j - 1] : 0));
    const uint64_t w = cum.at((size_t)s) - (s ? cum[(size_t)s - 1] : 0);
    *ep = j, *pos = s, *prob = (double)w / (double)t.total;
}

// search lens.i32 [E] w.i64 [sum] targets.i64 [n] -> i64 [n][2] prob.f64 [n]
static int search(char **a) {
    const Tables t = tables(load<int32_t>(a[0]), load<int64_t>(a[1]));
    const std::vector<int64_t> targets = load<int64_t>(a[2]);
    std::vector<int64_t> out(targets.size() * 2);
    std::vector<double> prob(targets.size());
    for (size_t i = 0; i < targets.size(); ++i) {
        if (targets[i] < 0 || (uint64_t)targets[i] >= t.total) return 5;
        resolve(t, (uint64_t)targets[i], &out[2 * i], &out[2 * i + 1], &prob[i]);
    }
    store(a[3], out);
    store(a[4], prob);
    return 0;
}

// draws seed step n K A lens.i32 [E] w.i64 [sum] -> i64 [n][K + 2] prob.f64 [n]
static int draws(char **a) {
    const uint64_t seed = strtoull(a[0], nullptr, 10), step = strtoull(a[1], nullptr, 10);
    const int n = atoi(a[2]), K = atoi(a[3]), A = atoi(a[4]);
    const Tables t = tables(load<int32_t>(a[5]), load<int64_t>(a[6]));
    std::vector<int64_t> out((size_t)n * (K + 2));
    std::vector<double> prob((size_t)n);
    for (int i = 0; i < n; ++i) {
        int64_t *dr = out.data() + (size_t)i * (K + 2);
        const uint64_t g = rt::prio_target(seed, step, (uint64_t)i, K, t.total);
        if (g >= t.total) return 5;
        resolve(t, g, dr, dr + 1, &prob[(size_t)i]);
        for (int k = 0; k < K; ++k) dr[2 + k] = rt::prio_filler(seed, step, (uint64_t)i, K, k, (uint64_t)A);
    }
    store(a[7], out);
    store(a[8], prob);
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "weights" && argc == 9) return weights(argv + 2);
    if (what == "weigh" && argc == 4) return weigh(argv + 2);
    if (what == "search" && argc == 7) return search(argv + 2);
    if (what == "draws" && argc == 11) return draws(argv + 2);
    return 4;
}
'''


drv = host_driver.fixture('mz_prioritized', DRIVER)


def flat(weights):
    return (np.array([len(w) for w in weights], dtype=np.int32), np.concatenate([np.asarray(w, dtype=np.int64) for w in weights]))


# ----------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize('discount', DISCOUNTS)
@pytest.mark.parametrize('K,td', CONFIGS)
def test_weights_equal_the_restatement(drv, K, td, discount):
    """|root value - ReplayBuffer._value_target| and its fixed-point weight: the header, the restatement and the host buffer's own
    expression agree bit for bit on episodes of every length that takes another path (shorter than, equal to, longer than td)."""
    D, A = 4, 2
    lengths = episode_lengths(K, td)
    episodes = episodes_of(packed_block(np.random.RandomState(7 * K + td), lengths, D, A), lengths, D, A)
    buf = ReplayBuffer(capacity=len(lengths), unroll_steps=K, td_steps=td, discount=discount)
    disc = np.array([discount ** i for i in range(td + 1)], dtype=np.float64)
    reward = np.concatenate([np.asarray(ep.rewards, dtype=np.float64) for ep in episodes])
    root = np.concatenate([np.asarray(ep.root_values, dtype=np.float64) for ep in episodes])
    p, w = drv.run('weights', [td], [np.array(lengths, dtype=np.int32), reward, root, disc], [np.float64, np.int64])
    want_p = np.array([abs(ep.root_values[t] - buf._value_target(ep, t)) for ep in episodes for t in range(len(ep))], dtype=np.float64)
    assert same_bits(p, want_p)
    want_w = np.concatenate([mz_priority_weights(ep.rewards, ep.root_values, td, discount) for ep in episodes])
    assert want_w.dtype == np.int64 and np.array_equal(w, want_w)
    assert np.array_equal(w, np.concatenate([mz_priority_weights(ep.rewards, ep.root_values, td, disc) for ep in episodes]))   # the table form
    assert np.array_equal(w, [max(1, int(v * 65536.0)) for v in want_p])   # (all below 65536: the truncation, as the issue states it)
    assert len(set(w.tolist())) > len(w) // 2 and w.min() >= 1             # full-mantissa inputs: the weights differ


@pytest.mark.parametrize('name', ['MAX', 'MIN'])
def test_weights_and_every_boundary_at_the_corners(drv, name):
    """The largest and the smallest td_steps and slot the device buffer accepts (tests/test_mz_replay_host.py: CORNERS), on the
    episodes that corner's buffer holds: the weights against the restatement and the host buffer's own expression, then the two
    searches at every boundary of their prefix sums -- each cumulative value and the target before it."""
    c = corner(name)
    buf = c.arbiter()
    episodes, td = buf.episodes, c.td
    disc = np.array([c.discount ** i for i in range(td + 1)], dtype=np.float64)
    lens = np.array([len(ep) for ep in episodes], dtype=np.int32)
    reward = np.concatenate([np.asarray(ep.rewards, dtype=np.float64) for ep in episodes])
    root = np.concatenate([np.asarray(ep.root_values, dtype=np.float64) for ep in episodes])
    p, w = drv.run('weights', [td], [lens, reward, root, disc], [np.float64, np.int64])
    want_p = np.array([abs(ep.root_values[t] - buf._value_target(ep, t)) for ep in episodes for t in range(len(ep))], dtype=np.float64)
    assert same_bits(p, want_p)
    weights = [mz_priority_weights(ep.rewards, ep.root_values, td, c.discount) for ep in episodes]
    assert np.array_equal(w, np.concatenate(weights)) and w.min() >= 1 and len(w) == int(lens.sum())
    cum = np.cumsum(w)
    total = int(cum[-1])
    targets = np.unique(np.clip(np.concatenate((cum - 1, cum, [0])), 0, total - 1)).astype(np.int64)
    out, prob = drv.run('search', [], [lens, w, targets], [np.int64, np.float64])
    out = out.reshape(-1, 2)
    ep, pos, _, want_prob = mz_prioritized_draws(0, 0, len(targets), weights, c.K, c.A, targets=targets)
    assert np.array_equal(out[:, 0], ep) and np.array_equal(out[:, 1], pos) and same_bits(prob, want_prob)
    steps = [(e, t) for e, m in enumerate(lens) for t in range(m)]
    assert sorted(set(zip(ep.tolist(), pos.tolist()))) == steps   # every step held is reached
    print('%s: %d weights, %d boundary targets' % (name, len(w), len(targets)))


def test_weight_of_hand_made_priorities(drv):
    p = np.array([0.0, 2.0 ** -17, 2.0 ** -16, 1.0 - 2.0 ** -53, 65535.99999, 65536.0, 1e300, float('nan')], dtype=np.float64)
    got, = drv.run('weigh', [], [p], [np.uint64])
    assert got.tolist() == [1, 1, 1, 65535, int(65535.99999 * 65536.0), 2 ** 32, 2 ** 32, 1]
    assert int(65535.99999 * 65536.0) == 2 ** 32 - 1   # (the truncated value: 2^32 - 0.65536 cut to an integer)
    more = np.array([-0.0, float('inf'), 0.5, 1.5 * 2.0 ** -16, 3.0, 65535.999999999], dtype=np.float64)
    got, = drv.run('weigh', [], [more], [np.uint64])
    assert got.tolist() == [1, 2 ** 32, 32768, 1, 196608, int(65535.999999999 * 65536.0)]
    # the restatement on the same values: a one-step episode with reward 0 has the return 0, so p = |root value|
    for v, w in zip(np.concatenate((p, more[1:])), [1, 1, 1, 65535, int(65535.99999 * 65536.0), 2 ** 32, 2 ** 32, 1,
                                                      2 ** 32, 32768, 1, 196608, int(65535.999999999 * 65536.0)]):
        assert mz_priority_weights([0.0], [v], 3, 0.5).tolist() == [w]


def test_the_search_is_exact(drv):
    """Every target of a small table: each step is hit exactly as often as it weighs, in order, and prob is w / total."""
    for weights in ([[3], [1, 1, 5], [2, 7]], [[1]], [[1, 1], [1], [4, 1, 1, 2]], [[2 ** 32, 1], [1, 2 ** 32]]):
        lens, w = flat(weights)
        total = int(w.sum())
        if total < 10 ** 4:
            targets = np.arange(total, dtype=np.int64)
        else:   # the cap's size: every boundary instead of every target
            cum = np.cumsum(w)
            targets = np.unique(np.clip(np.concatenate((cum - 1, cum, [0])), 0, total - 1)).astype(np.int64)
        out, prob = drv.run('search', [], [lens, w, targets], [np.int64, np.float64])
        out = out.reshape(-1, 2)
        ep, pos, _, want_prob = mz_prioritized_draws(0, 0, len(targets), weights, 2, 2, targets=targets)
        assert np.array_equal(out[:, 0], ep) and np.array_equal(out[:, 1], pos) and same_bits(prob, want_prob)
        if total < 10 ** 4:
            steps = [(e, t) for e, ws in enumerate(weights) for t in range(len(ws))]
            want = np.repeat(np.arange(len(steps)), w)   # step s owns w[s] consecutive targets
            assert [steps[s] for s in want] == [tuple(r) for r in out.tolist()]
            assert same_bits(prob, np.array([float(w[s]) / float(total) for s in want], dtype=np.float64))
    with pytest.raises(subprocess.CalledProcessError):   # (the driver refuses a target of `total`, as the kernel does)
        drv.run('search', [], [np.array([1], dtype=np.int32), np.array([3], dtype=np.int64), np.array([3], dtype=np.int64)], [np.int64, np.float64])
    with pytest.raises(ValueError):
        mz_prioritized_draws(0, 0, 1, [[3]], 2, 2, targets=[3])
    with pytest.raises(ValueError):
        mz_prioritized_draws(0, 0, 1, [[3], []], 2, 2)


@pytest.mark.parametrize('K,A', [(2, 2), (5, 3)])
def test_draws_equal_the_restatement(drv, K, A):
    rng = np.random.RandomState(K)
    weights = [rng.randint(1, 2 ** 20, size=m).astype(np.int64) for m in (1, 12, 5, 3)] + [np.array([2 ** 22, 1], dtype=np.int64)]
    lens, w = flat(weights)
    seen = []
    for seed in (13, 2 ** 64 - 1):
        for step in (0, 1):
            out, prob = drv.run('draws', [seed, step, 64, K, A], [lens, w], [np.int64, np.float64])
            out = out.reshape(64, K + 2)
            ep, pos, filler, want_prob = mz_prioritized_draws(seed, step, 64, weights, K, A)
            assert np.array_equal(out[:, 0], ep) and np.array_equal(out[:, 1], pos) and np.array_equal(out[:, 2:], filler)
            assert same_bits(prob, want_prob)
            assert (ep >= 0).all() and (ep < len(weights)).all() and (pos >= 0).all() and (pos < lens[ep]).all()
            assert (filler >= 0).all() and (filler < A).all() and len(set(filler.reshape(-1).tolist())) == A
            assert same_bits(prob, np.array([float(weights[e][t]) / float(int(w.sum())) for e, t in zip(ep, pos)], dtype=np.float64))
            # another stream than the uniform sampler's of the same (seed, step)
            s_ep, s_pos, s_fill = mz_replay_draws(seed, step, 64, lens, K, A)
            assert not np.array_equal(s_fill, filler) and not (np.array_equal(s_ep, ep) and np.array_equal(s_pos, pos))
            seen.append((ep, pos))
    assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[0][0], seen[2][0])   # step and seed key the stream


def agents(n=2):
    import torch
    from rlzero_amd.muzero import MuZeroAgent
    out = []
    for _ in range(n):
        torch.manual_seed(3)
        out.append(MuZeroAgent(device='cpu'))
    for other in out[1:]:
        for p, q in zip(out[0].net.parameters(), other.net.parameters()):
            assert torch.equal(p, q)
    return out


def host_batch(n=32):
    K, td, D, A = 5, 10, 4, 2
    lengths = episode_lengths(K, td)
    buf = ReplayBuffer(capacity=len(lengths), unroll_steps=K, td_steps=td, discount=0.997, seed=1)
    for ep in episodes_of(packed_block(np.random.RandomState(11), lengths, D, A), lengths, D, A):
        buf.add(ep)
    return buf.sample(n, A)


def test_learn_with_weights():
    """weights = 1 is weights=None bit for bit (losses and parameters, from equal initial states); weights = 2 doubles the loss."""
    import torch
    batch = host_batch()
    n = len(batch[0])
    plain, ones, twos = agents(3)
    a = plain.learn(batch)
    b = ones.learn(batch, weights=torch.ones(n))
    assert a == b
    for p, q in zip(plain.net.parameters(), ones.net.parameters()):
        assert torch.equal(p, q)
    assert plain.learn(batch) == ones.learn(batch, weights=np.ones(n, dtype=np.float32))   # a second step, the optimizer's state included
    for p, q in zip(plain.net.parameters(), ones.net.parameters()):
        assert torch.equal(p, q)
    c = twos.learn(batch, weights=torch.full((n, ), 2.0))
    assert abs(c[0] - 2.0 * a[0]) <= 1e-6 * abs(2.0 * a[0])
    assert c[1:] == a[1:]   # the component losses stay unweighted
    # weights that differ entry by entry: the weighted mean of the entries' losses
    _, weighted = agents(2)
    w = torch.linspace(0.25, 3.0, n)
    d = weighted.learn(batch, weights=w)
    assert d[1:] == a[1:] and d[0] != a[0]


def test_the_trainer_refuses_priorities_without_device_replay():
    """--prioritized-replay needs --device-replay: the script says so and exits non-zero before anything touches the GPU."""
    import importlib.util
    script = os.path.join(REPO, 'tools', 'train_muzero.py')
    for extra in ([], ['--priority-beta', '0.4']):
        run = subprocess.run([sys.executable, script, '--prioritized-replay'] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert run.returncode != 0 and b'--prioritized-replay needs --device-replay' in run.stderr
    spec = importlib.util.spec_from_file_location('train_muzero', script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(ValueError, match='needs --device-replay'):
        mod.MuZeroPipeline(n_envs=8, prioritized_replay=True)
