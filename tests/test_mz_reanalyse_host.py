"""MuZero Reanalyse on the CPU: the arithmetic and the draws of rlzero_amd/csrc/rz_mz_target.h that k_mzr_positions and
k_mzr_update call (policy_of_visits, root_value_of, reanalyse_draw), BIT FOR BIT against their numpy / Python statements --
EpisodeSeq.fields_of_packed's policy expression, MuZeroSelfPlay.search's root value, rlzero_amd/muzero/reanalyse.py:
mz_reanalyse_draws.  A driver with its own main is compiled against the header with ROCm's clang++ and -ffp-contract=off, by
tests/host_driver.py, and once more with -fsanitize=address,undefined (a stand-alone program); every
call runs both and holds their outputs equal.  ``patched`` -- the host ReplayBuffer with some steps' targets replaced by those
numpy expressions -- is what the GPU tests (tests/test_mz_reanalyse_gpu.py) compare the device store with."""
import copy
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import host_driver
from rlzero_amd.muzero.reanalyse import mz_reanalyse_draws
from rlzero_amd.muzero.replay import mz_replay_draws
from rlzero_amd.muzero.selfplay import Episode, ReplayBuffer
from test_mz_replay_host import same_bits

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

// visits A visits.i32 [R][A] -> policy.f32 [R][A]
static int visits(char **a) {
    const int A = atoi(a[0]);
    const std::vector<int32_t> in = load<int32_t>(a[1]);
    const size_t R = in.size() / A;
    std::vector<float> out(R * A);
    for (size_t r = 0; r < R; ++r) {
        const std::vector<int32_t> row(in.begin() + r * A, in.begin() + (r + 1) * A);   // (a heap row of exactly A counts)
        for (int c = 0; c < A; ++c) out[r * A + c] = rt::policy_of_visits(row.data(), A, c);
    }
    store(a[2], out);
    return 0;
}

// values n.i32 [R] sum.f64 [R] -> value.f64 [R]
static int values(char **a) {
    const std::vector<int32_t> n = load<int32_t>(a[0]);
    const std::vector<double> sum = load<double>(a[1]);
    if (n.size() != sum.size()) return 4;
    std::vector<double> out(n.size());
    for (size_t r = 0; r < n.size(); ++r) out[r] = rt::root_value_of(n[r], sum[r]);
    store(a[2], out);
    return 0;
}

// draws seed step n lengths.i32 [E] -> i64 [n][2]
static int draws(char **a) {
    const uint64_t seed = strtoull(a[0], nullptr, 10), step = strtoull(a[1], nullptr, 10);
    const int n = atoi(a[2]);
    const std::vector<int32_t> lengths = load<int32_t>(a[3]);
    std::vector<int64_t> out((size_t)n * 2);
    for (int i = 0; i < n; ++i) {
        out[2 * i] = rt::reanalyse_draw(seed, step, (uint64_t)i, 0, lengths.size());
        out[2 * i + 1] = rt::reanalyse_draw(seed, step, (uint64_t)i, 1, (uint64_t)lengths.at((size_t)out[2 * i]));
    }
    store(a[4], out);
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "visits" && argc == 5) return visits(argv + 2);
    if (what == "values" && argc == 5) return values(argv + 2);
    if (what == "draws" && argc == 7) return draws(argv + 2);
    return 4;
}
'''


drv = host_driver.fixture('mz_reanalyse', DRIVER)


# ----------------------------------------------------------------------------------------------- the numpy statements
def policy_of_visits(visits):
    """float32 [n, A]: EpisodeSeq.fields_of_packed's expression on the counts as float64; a row of zeros gives the uniform policy
    of ReplayBuffer.sample (np.full(.., 1.0 / A, dtype=float32))."""
    vis = np.asarray(visits).astype(np.float64)
    total = vis.sum(axis=1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        pol = (vis / total).astype(np.float32)
    pol[total[:, 0] == 0] = np.full(vis.shape[1], 1.0 / vis.shape[1], dtype=np.float32)
    return pol


def root_value_of(n, vsum):
    """float64 [n]: MuZeroSelfPlay.search's vsum / n.clamp_min(1)."""
    return np.asarray(vsum, dtype=np.float64) / np.maximum(np.asarray(n), 1).astype(np.float64)


def patched(host_buffer, ep_idx, pos, visits, n, vsum):
    """A copy of the host ``ReplayBuffer`` in which step ``pos[i]`` of episode ``ep_idx[i]`` (0 = the oldest held) has the policy
    ``policy_of_visits(visits[i])`` and the root value ``root_value_of(n[i], vsum[i])``; everything else -- the other steps,
    observations, actions, rewards, the generator -- as it was.  The original is not touched."""
    out = ReplayBuffer(capacity=host_buffer.capacity, unroll_steps=host_buffer.K, td_steps=host_buffer.td_steps, discount=host_buffer.discount)
    out.rng = copy.deepcopy(host_buffer.rng)
    out.episodes = [Episode.from_arrays(*(np.array(getattr(ep, name)) for name in Episode.FIELDS)) for ep in host_buffer.episodes]
    pol, val = policy_of_visits(np.asarray(visits).reshape(len(ep_idx), -1)), root_value_of(n, vsum)
    for i, (e, p) in enumerate(zip(ep_idx, pos)):
        ep = out.episodes[int(e)]
        assert 0 <= int(p) < len(ep)
        ep.policies[int(p)] = pol[i]
        ep.root_values[int(p)] = val[i]
    return out


# ----------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize('A', [2, 3, 8])
def test_policy_of_visits(drv, A):
    rng = np.random.RandomState(A)
    rows = [[0] * A, [1] + [0] * (A - 1), [0] * (A - 1) + [1], [49, 1] + [0] * (A - 2), [1, 49] + [0] * (A - 2),
            [17, 16, 17] + [0] * (A - 3) if A >= 3 else [17, 16], [50] + [0] * (A - 1), [2 ** 30] * A]
    vis = np.concatenate((np.array(rows, dtype=np.int32), rng.randint(0, 51, size=(64, A)).astype(np.int32)))
    got, = drv.run('visits', [A], [vis], [np.float32])
    want = (vis.astype(np.float64)[1:] / vis.astype(np.float64)[1:].sum(axis=1, keepdims=True)).astype(np.float32)
    assert same_bits(got.reshape(-1, A)[1:], want)                                              # the issue's expression, as it stands
    assert same_bits(got.reshape(-1, A)[0], np.full(A, 1.0 / A, dtype=np.float32))             # all zeros: uniform
    assert same_bits(got.reshape(-1, A), policy_of_visits(vis))                                 # and the helper of `patched`
    if A == 3:
        assert got.reshape(-1, A)[5].tolist() == [np.float32(17 / 50), np.float32(16 / 50), np.float32(17 / 50)]


@pytest.mark.parametrize('A', [1, 8])
def test_policy_and_root_value_at_the_action_limits(drv, A):
    """One action and eight, the limits of the device buffer: an unvisited root, a single visit, counts whose sum needs 33 bits
    at A = 8, random rows; and the root value at N = 0, 1 and 40."""
    rng = np.random.RandomState(40 + A)
    rows = [[0] * A, [1] + [0] * (A - 1), [0] * (A - 1) + [1], [40] * A, [2 ** 30] * A]
    vis = np.concatenate((np.array(rows, dtype=np.int32), rng.randint(0, 51, size=(64, A)).astype(np.int32)))
    got, = drv.run('visits', [A], [vis], [np.float32])
    got = got.reshape(-1, A)
    assert same_bits(got, policy_of_visits(vis))
    assert same_bits(got[0], np.full(A, 1.0 / A, dtype=np.float32))
    with np.errstate(invalid='ignore'):
        want = (vis.astype(np.float64) / vis.astype(np.float64).sum(axis=1, keepdims=True)).astype(np.float32)
    some = vis.sum(axis=1) > 0
    assert same_bits(got[some], want[some]) and some.sum() >= len(vis) - 2
    if A == 1:
        assert (got == 1.0).all()   # one action: the policy is 1 whatever the count, zero included
    n = np.array([0, 1, 40] * 8, dtype=np.int32)
    vsum = rng.standard_normal(len(n)) * 9.3
    value, = drv.run('values', [], [n, vsum], [np.float64])
    assert same_bits(value, root_value_of(n, vsum))
    assert same_bits(value, np.array([s / max(int(k), 1) for k, s in zip(n, vsum)], dtype=np.float64))


def test_root_value_of(drv):
    rng = np.random.RandomState(5)
    ns, sums = [], []
    for n in (0, 1, 50, 51):
        for s in (0.0, 1.0, -1.0, 1.0 / 3.0, -7.3, 49.99999, 1e-300, -123456.789, float(rng.standard_normal() * 9.3)):
            ns.append(n)
            sums.append(s)
    n, vsum = np.array(ns, dtype=np.int32), np.array(sums, dtype=np.float64)
    got, = drv.run('values', [], [n, vsum], [np.float64])
    want = np.array([s / max(int(k), 1) for k, s in zip(ns, sums)], dtype=np.float64)
    assert same_bits(got, want) and same_bits(got, root_value_of(n, vsum))
    assert got[ns.index(0)] == 0.0 and got[ns.index(0) + 1] == 1.0                              # n = 0 divides by 1
    inexact = [i for i, (k, s) in enumerate(zip(ns, sums)) if k > 1 and Fraction(float(got[i])) * k != Fraction(s)]
    assert inexact                                                                              # (quotients that had to round)


def test_draws_equal_the_restatement(drv):
    lengths = np.array([1, 12, 5, 3], dtype=np.int32)
    seen = []
    for seed, step in ((0, 0), (13, 1), (2 ** 64 - 1, 2 ** 40 + 3)):
        got, = drv.run('draws', [seed, step, 64], [lengths], [np.int64])
        got = got.reshape(64, 2)
        ep, pos = mz_reanalyse_draws(seed, step, 64, lengths)
        assert np.array_equal(got[:, 0], ep) and np.array_equal(got[:, 1], pos)
        assert (ep >= 0).all() and (ep < len(lengths)).all() and (pos >= 0).all() and (pos < lengths[ep]).all()
        assert len(set(ep.tolist())) == len(lengths)                                            # every episode is drawn
        for K, A in ((2, 2), (5, 3)):   # the sampler's stream of the same (seed, step) is another one
            s_ep, s_pos, _ = mz_replay_draws(seed, step, 64, lengths, K, A)
            assert not (np.array_equal(s_ep, ep) and np.array_equal(s_pos, pos)) and not np.array_equal(s_ep, ep)
        seen.append(ep)
    assert not np.array_equal(seen[0], seen[1])
    a, b = mz_reanalyse_draws(5, 0, 64, lengths), mz_reanalyse_draws(5, 1, 64, lengths)
    assert not np.array_equal(a[0], b[0])                                                       # the refresh's number keys the stream
    with pytest.raises(ValueError):
        mz_reanalyse_draws(0, 0, 4, [3, 0])


def test_patched_on_two_episodes():
    host = ReplayBuffer(capacity=2, unroll_steps=2, td_steps=3, discount=0.5, seed=1)
    first = Episode.from_arrays(np.arange(12, dtype=np.float32).reshape(3, 4), np.array([0, 1, 0]), np.array([1.0, 1.0, 1.0]),
                                np.array([[0.5, 0.5], [0.25, 0.75], [1.0, 0.0]], dtype=np.float32), np.array([0.1, 0.2, 0.3]))
    second = Episode.from_arrays(np.ones((2, 4), dtype=np.float32), np.array([1, 1]), np.array([1.0, 0.0]),
                                 np.array([[0.0, 1.0], [0.5, 0.5]], dtype=np.float32), np.array([-1.0, -2.0]))
    host.add(first), host.add(second)
    before = [[np.array(getattr(ep, name)) for name in Episode.FIELDS] for ep in host.episodes]
    # step 1 of the older episode (named twice, the same payload), step 0 of the younger one with an unvisited root
    out = patched(host, [0, 1, 0], [1, 0, 1], [[49, 1], [0, 0], [49, 1]], [50, 0, 50], [25.0, 3.0, 25.0])
    for ep, fields in zip(host.episodes, before):   # the original is as it was
        assert all(np.array_equal(getattr(ep, name), f) for name, f in zip(Episode.FIELDS, fields))
    a, b = out.episodes
    assert a.policies.tolist() == [[0.5, 0.5], [np.float32(0.98), np.float32(0.02)], [1.0, 0.0]] and a.policies.dtype == np.float32
    assert a.root_values.tolist() == [0.1, 0.5, 0.3]
    assert b.policies.tolist() == [[0.5, 0.5], [0.5, 0.5]] and b.root_values.tolist() == [3.0, -2.0]
    for name in ('obs', 'actions', 'rewards'):
        assert all(np.array_equal(getattr(x, name), getattr(y, name)) for x, y in zip(out.episodes, host.episodes))
    # the refreshed root value reaches the bootstrap of the step td_steps before it: none here (3 steps, td 3), so with td 1
    host.td_steps = 1
    out = patched(host, [0], [1], [[1, 1]], [4], [8.0])
    assert out._value_target(out.episodes[0], 0) == 1.0 + 2.0 * 0.5 and host._value_target(host.episodes[0], 0) == 1.0 + 0.2 * 0.5


def test_the_trainer_refuses_reanalyse_without_device_replay():
    """--reanalyse needs --device-replay: the script says so and exits non-zero before anything touches the GPU (this test has none)."""
    import importlib.util
    import sys
    script = os.path.join(REPO, 'tools', 'train_muzero.py')
    for value in ('32', 'all'):
        run = subprocess.run([sys.executable, script, '--reanalyse', value], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert run.returncode != 0 and b'--reanalyse needs --device-replay' in run.stderr
    spec = importlib.util.spec_from_file_location('train_muzero', script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.reanalyse_arg('all') == 'all' and mod.reanalyse_arg('2048') == 2048 and mod.reanalyse_arg('0') == 0
    for value in (32, 'all'):
        with pytest.raises(ValueError, match='needs --device-replay'):
            mod.MuZeroPipeline(n_envs=8, reanalyse=value)
