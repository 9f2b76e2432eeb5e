"""The rules of MuZero's moves on the device (rlzero_amd/csrc/rz_mz_env.h) on the CPU, against the scalar twins (tests/acrobot_twin.py;
oracle/muzero_ref.RefCartPole through tests/cartpole_twin.py) and the host restatement of the keys and the action draw
(tests/device_streams.py).

A driver with its own main is compiled against the header with ROCm's clang++ (by tests/host_driver.py),
-ffp-contract=off, fed binary inputs and compared with the twin:

* ``acrobot_step`` / ``acrobot_observe`` over 4000 random states and actions and over crafted states -- an angle leaving [-pi, pi]
  on each side, each velocity bound passed on each side, the height crossing 1.0, steps = max - 1 -- equal the twin BIT FOR BIT:
  the same libm, the same order of operations, no contraction.
* ``acrobot_reset`` equals ``rlzero_amd.muzero.acrobot_initial_states`` bit for bit and lies in [-0.1, 0.1).
* ``EnvCartPole`` (the benchmark's environment) over 4000 random states and actions and over crafted states -- x across +2.4 and
  -2.4, theta across each threshold, steps = 499 truncated only, one state terminated and truncated -- equals RefCartPole BIT FOR BIT;
  its reset equals ``rlzero_amd.muzero.cartpole.initial_states`` bit for bit and lies in [-0.05, 0.05).
* The header's action draw (``move_weights`` / ``move_draw`` / ``move_key``) is ``device_streams.muzero_action``, its per-action noise
  key ``device_streams.muzero_action_keys``, its record layout the one include/rlzero_hip.h documents.
* The same driver built with -fsanitize=address,undefined runs every input as a stand-alone program and writes the same bytes.
* What the GPU test's bound of 1e-9 catches: the twin with k3 dropped, dt / 6 replaced by dt / 4, the -pi / 2 dropped from phi2, or
  the velocity clamp removed is more than 1e-4 away from the true twin in at least one of the random states, each; so is RefCartPole's
  step with tau changed, the 4 / 3 dropped or the force's sign swapped.
* The trainer's parser takes ``--env acrobot`` and refuses an unknown environment."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import acrobot_twin as twin
import cartpole_twin as cart
import device_streams as ds
import host_driver
from rlzero_amd.muzero.acrobot import acrobot_initial_states

GPU_BOUND = 1e-9       # tests/test_mz_env_gpu.py
CAUGHT_ABOVE = 1e-4    # five orders above it

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rz_mz_env.h"

namespace re = rzmze;

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

// step max_steps state.f64 [n][4] steps.i64 [n] actions.i64 [n] -> state.f64 [n][4], steps.i64 [n], reward.f64 [n], flags.i32 [n],
//   obs before.f32 [n][kObs], obs after.f32 [n][kObs]      (through the trait, as the kernels go)
template <typename Env>
static int step(char **a) {
    constexpr int D = Env::kObs;
    const long long max_steps = atoll(a[0]);
    const std::vector<double> state = load<double>(a[1]);
    const std::vector<int64_t> steps = load<int64_t>(a[2]), actions = load<int64_t>(a[3]);
    const size_t n = steps.size();
    if (state.size() != 4 * n || actions.size() != n) return 4;
    std::vector<double> out(4 * n), reward(n);
    std::vector<int64_t> steps_out(n);
    std::vector<int32_t> flags(n);
    std::vector<float> before(D * n), after(D * n);
    for (size_t i = 0; i < n; ++i) {
        typename Env::State c;
        Env::load(c, &state[4 * i], steps[i], 0);
        Env::observe(c, &before[D * i]);
        flags[i] = Env::step(c, (int)actions[i], max_steps, &reward[i]);
        Env::store(c, &out[4 * i]);
        steps_out[i] = c.steps;
        Env::observe(c, &after[D * i]);
    }
    store(a[4], out);
    store(a[5], steps_out);
    store(a[6], reward);
    store(a[7], flags);
    store(a[8], before);
    store(a[9], after);
    return 0;
}

// reset seed env.i64 [n] episode.i64 [n] -> state.f64 [n][4], steps.i64 [n]
template <typename Env>
static int reset(char **a) {
    const uint64_t seed = strtoull(a[0], nullptr, 10);
    const std::vector<int64_t> env = load<int64_t>(a[1]), episode = load<int64_t>(a[2]);
    const size_t n = env.size();
    if (episode.size() != n) return 4;
    std::vector<double> out(4 * n);
    std::vector<int64_t> steps(n);
    for (size_t i = 0; i < n; ++i) {
        const double nines[4] = {9.0, 9.0, 9.0, 9.0};
        typename Env::State c;
        Env::load(c, nines, 77, episode[i]);
        Env::reset(c, seed, (int)env[i]);
        Env::store(c, &out[4 * i]);
        steps[i] = c.steps;
    }
    store(a[3], out);
    store(a[4], steps);
    return 0;
}

// draw A seed inv_T visits.i32 [n][A] env.i64 [n] episode.i64 [n] steps.i64 [n] -> action.i32 [n]
static int draw(char **a) {
    const int A = atoi(a[0]);
    const uint64_t seed = strtoull(a[1], nullptr, 10);
    const double inv_t = atof(a[2]);
    const std::vector<int32_t> visits = load<int32_t>(a[3]);
    const std::vector<int64_t> env = load<int64_t>(a[4]), episode = load<int64_t>(a[5]), steps = load<int64_t>(a[6]);
    const size_t n = env.size();
    if (A < 1 || A > RZ_MZE_MAX_ACTIONS || visits.size() != n * (size_t)A || episode.size() != n || steps.size() != n) return 4;
    std::vector<int32_t> action(n);
    for (size_t i = 0; i < n; ++i) {
        const std::vector<int> v(visits.begin() + i * A, visits.begin() + (i + 1) * A);
        std::vector<double> w((size_t)A);
        double total = 0.0;
        int act = re::move_weights(v.data(), A, inv_t, w.data(), &total);
        if (inv_t > 0.0) act = re::move_draw(w.data(), A, total, re::move_key(seed, 0xA5A5A5A5ull, (int)env[i], episode[i], steps[i]));
        action[i] = act;
    }
    store(a[7], action);
    return 0;
}

// noise_keys A seed env.i64 [n] episode.i64 [n] steps.i64 [n] -> key.u32 [n][A]: the per-action keys of a move's root noise
static int noise_keys(char **a) {
    const int A = atoi(a[0]);
    const uint64_t seed = strtoull(a[1], nullptr, 10);
    const std::vector<int64_t> env = load<int64_t>(a[2]), episode = load<int64_t>(a[3]), steps = load<int64_t>(a[4]);
    const size_t n = env.size();
    if (A < 1 || A > RZ_MZE_MAX_ACTIONS || episode.size() != n || steps.size() != n) return 4;
    std::vector<uint32_t> key(n * (size_t)A);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < A; ++k) key[i * A + k] = re::noise_key(re::move_key(seed, 0ull, (int)env[i], episode[i], steps[i]), k);
    store(a[5], key);
    return 0;
}

// layout D A -> i32 [6]: the offsets of action, reward, visits, root value and done in a record, and its length
static int layout(char **a) {
    const re::RecordLayout r = re::record_layout(atoi(a[0]), atoi(a[1]));
    store(a[2], std::vector<int32_t>{r.action, r.reward, r.visits, r.root_value, r.done, r.row});
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "step" && argc == 12) return step<re::EnvAcrobot>(argv + 2);
    if (what == "reset" && argc == 7) return reset<re::EnvAcrobot>(argv + 2);
    if (what == "cartpole_step" && argc == 12) return step<re::EnvCartPole>(argv + 2);
    if (what == "cartpole_reset" && argc == 7) return reset<re::EnvCartPole>(argv + 2);
    if (what == "noise_keys" && argc == 8) return noise_keys(argv + 2);
    if (what == "layout" && argc == 5) return layout(argv + 2);
    if (what == "draw" && argc == 10) return draw(argv + 2);
    return 4;
}
'''


drv = host_driver.fixture('mz_env', DRIVER)


def random_cases(n=4000, seed=5):
    """States over the whole range a step can leave behind (angles in [-pi, pi], velocities inside their bounds), any action, any
    step count below the limit."""
    rng = np.random.RandomState(seed)
    state = np.stack([rng.uniform(-twin.PI, twin.PI, n), rng.uniform(-twin.PI, twin.PI, n), rng.uniform(-twin.MAX_VEL_1, twin.MAX_VEL_1, n),
                      rng.uniform(-twin.MAX_VEL_2, twin.MAX_VEL_2, n)], axis=1)
    return state, rng.randint(0, 499, size=n).astype(np.int64), rng.randint(0, 3, size=n).astype(np.int64)


def twin_steps(state, steps, actions, max_steps, variant=None):
    out, steps_out, reward, flags = np.zeros_like(state), np.zeros_like(steps), np.zeros(len(state)), np.zeros(len(state), dtype=np.int32)
    for i in range(len(state)):
        new, steps_out[i], reward[i], term, trunc = twin.step(tuple(state[i]), int(steps[i]), int(actions[i]), max_steps, variant)
        out[i] = new
        flags[i] = (1 if term else 0) | (2 if trunc else 0)
    return out, steps_out, reward, flags


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def driver_step(drv, state, steps, actions, max_steps):
    out, steps_out, reward, flags, before, after = drv.run('step', [max_steps], [state, steps, actions],
                                                           [np.float64, np.int64, np.float64, np.int32, np.float32, np.float32])
    return out.reshape(-1, 4), steps_out, reward, flags, before.reshape(-1, 6), after.reshape(-1, 6)


def check_against_twin(drv, state, steps, actions, max_steps):
    out, steps_out, reward, flags, before, after = driver_step(drv, state, steps, actions, max_steps)
    want, want_steps, want_reward, want_flags = twin_steps(state, steps, actions, max_steps)
    assert same_bits(out, want), 'largest difference %g' % np.abs(out - want).max()
    assert np.array_equal(steps_out, want_steps) and same_bits(reward, want_reward) and np.array_equal(flags, want_flags)
    assert same_bits(before, np.stack([twin.observe(s) for s in state]))
    assert same_bits(after, np.stack([twin.observe(s) for s in want]))
    return want, want_flags, want_reward


def test_header_is_the_twin_on_random_states(drv):
    """4000 states x actions, both builds of the driver (the sanitized one ends clean): every bit of state, reward, flags and both
    observations.  The sample holds terminal steps, wraps on both sides and clamps (asserted: the comparison saw them)."""
    state, steps, actions = random_cases()
    want, flags, reward = check_against_twin(drv, state, steps, actions, 500)
    raw = np.array([twin.integrate(tuple(s), int(a)) for s, a in zip(state, actions)])
    assert (flags & 1).any() and not (flags & 1).all() and (reward[(flags & 1) == 1] == 0.0).all() and (reward[(flags & 1) == 0] == -1.0).all()
    assert (raw[:, :2] > twin.PI).any() and (raw[:, :2] < -twin.PI).any()
    assert (np.abs(raw[:, 2]) > twin.MAX_VEL_1).any() and (np.abs(raw[:, 3]) > twin.MAX_VEL_2).any()
    assert np.abs(want[:, :2]).max() <= twin.PI and np.abs(want[:, 2]).max() <= twin.MAX_VEL_1 and np.abs(want[:, 3]).max() <= twin.MAX_VEL_2


def test_header_is_the_twin_on_crafted_states(drv):
    """Every decision of a step met on purpose, and that the crafted states do meet them."""
    cases = twin.crafted_states()
    state = np.array([c[1] for c in cases], dtype=np.float64)
    actions = np.array([c[2] for c in cases], dtype=np.int64)
    steps = np.full(len(cases), 11, dtype=np.int64)   # steps = max - 1: every one of them is truncated at max = 12
    want, flags, reward = check_against_twin(drv, state, steps, actions, 12)
    assert (flags & 2).all()
    _, flags500, _ = check_against_twin(drv, state, steps, actions, 500)
    assert not (flags500 & 2).any() and np.array_equal(flags500 & 1, flags & 1)
    raw = {c[0]: twin.integrate(c[1], c[2]) for c in cases}
    assert raw['theta1 above pi'][0] > twin.PI and raw['theta1 below -pi'][0] < -twin.PI
    assert raw['theta2 above pi'][1] > twin.PI and raw['theta2 below -pi'][1] < -twin.PI
    assert raw['dtheta1 above its bound'][2] > twin.MAX_VEL_1 and raw['dtheta1 below minus its bound'][2] < -twin.MAX_VEL_1
    assert raw['dtheta2 above its bound'][3] > twin.MAX_VEL_2 and raw['dtheta2 below minus its bound'][3] < -twin.MAX_VEL_2
    names = [c[0] for c in cases]
    i, j = names.index('height crosses 1'), names.index('height stays below 1')
    assert twin.height(cases[i][1]) < 1.0 < twin.height(want[i]) and flags[i] & 1 and reward[i] == 0.0
    assert twin.height(want[j]) < 1.0 and not flags[j] & 1 and reward[j] == -1.0
    assert min(twin.decision_margin(c[1], c[2]) for c in cases) > 0.01   # (none of them sits on a decision: the GPU test reuses them)


def test_a_huge_angle_does_not_spin(drv):
    """The wrap is bounded (kAcroWraps turns): 1e300 - 2 pi is 1e300, and a state nobody should set still ends the step, with the
    twin's bits."""
    state = np.array([[1e300, 0.0, 0.0, 0.0], [0.0, -1e300, 0.0, 0.0]])
    steps, actions = np.zeros(2, dtype=np.int64), np.ones(2, dtype=np.int64)
    out, _, _, _, _, _ = driver_step(drv, state, steps, actions, 500)
    want, _, _, _ = twin_steps(state, steps, actions, 500)
    assert np.isfinite(want).all() and same_bits(out, want)


def test_reset_is_the_restatement(drv):
    rng = np.random.RandomState(2)
    env = np.concatenate([np.arange(40), rng.randint(0, 2 ** 20, size=200)]).astype(np.int64)
    episode = np.concatenate([np.zeros(40), rng.randint(0, 2 ** 40, size=200)]).astype(np.int64)
    for seed in (0, 7, 2 ** 64 - 1):
        got, steps = drv.run('reset', [seed], [env, episode], [np.float64, np.int64])
        want = acrobot_initial_states(seed, env, episode)
        assert same_bits(got.reshape(-1, 4), want) and not steps.any()
        assert want.min() >= -0.1 and want.max() < 0.1
        assert want.std() > 0.05 and abs(want.mean()) < 0.01   # (uniform over the range: 0.2 / sqrt(12) = 0.0577)
    assert not same_bits(acrobot_initial_states(0, env, episode), acrobot_initial_states(1, env, episode))
    assert same_bits(acrobot_initial_states(3, 5, 2), acrobot_initial_states(3, [5], [2]))


@pytest.mark.parametrize('A,inv_t', [(3, 1.0), (3, 2.0), (3, 0.0), (2, 1.0), (8, 0.5)])
def test_the_headers_action_draw_is_the_restatement(drv, A, inv_t):
    """``move_weights`` / ``move_draw`` under ``move_key``: the bits tests/device_streams.py::muzero_action restates (rows whose
    draw falls within 1e-12 of a boundary of the cumulative sums of a pow() are left out for 1 / T outside {0, 1}: none here)."""
    rng = np.random.RandomState(A)
    n = 3000
    visits = rng.randint(0, 20, size=(n, A)).astype(np.int32)
    visits[visits.sum(axis=1) == 0, 0] = 1
    env, episode, steps = (rng.randint(0, hi, size=n).astype(np.int64) for hi in (8192, 1000, 500))
    got, = drv.run('draw', [A, 11, inv_t], [visits, env, episode, steps], [np.int32])
    want, gap = ds.muzero_action(11, env, episode, steps, visits, inv_t)
    keep = gap > 1e-12
    assert keep.all() and np.array_equal(got[keep], want[keep])
    if inv_t > 0:
        assert len(np.unique(got)) == A


# ------------------------------------------------------------------------------------------------ CartPole and the rules of a move
def cartpole_random_cases(n=4000, seed=6):
    """States well past every threshold on both sides (2.4; 12 degrees = 0.2094), any action, any step count below the limit."""
    rng = np.random.RandomState(seed)
    state = np.stack([rng.uniform(-2.6, 2.6, n), rng.uniform(-3.0, 3.0, n), rng.uniform(-0.23, 0.23, n), rng.uniform(-3.0, 3.0, n)], axis=1)
    return state, rng.randint(0, 499, size=n).astype(np.int64), rng.randint(0, 2, size=n).astype(np.int64)


def cartpole_ref_steps(state, steps, actions, max_steps, variant=None):
    out, steps_out, reward, flags = np.zeros_like(state), np.zeros_like(steps), np.zeros(len(state)), np.zeros(len(state), dtype=np.int32)
    for i in range(len(state)):
        new, steps_out[i], reward[i], term, trunc = cart.step(tuple(state[i]), int(steps[i]), int(actions[i]), max_steps, variant)
        out[i] = new
        flags[i] = (1 if term else 0) | (2 if trunc else 0)
    return out, steps_out, reward, flags


def check_against_ref_cartpole(drv, state, steps, actions, max_steps):
    """``EnvCartPole`` against RefCartPole: every bit of the state, the step count, both flags, the reward of 1 and the two observations."""
    got = drv.run('cartpole_step', [max_steps], [state, steps, actions], [np.float64, np.int64, np.float64, np.int32, np.float32, np.float32])
    out, steps_out, reward, flags, before, after = got
    want, want_steps, want_reward, want_flags = cartpole_ref_steps(state, steps, actions, max_steps)
    assert same_bits(out.reshape(-1, 4), want), 'largest difference %g' % np.abs(out.reshape(-1, 4) - want).max()
    assert np.array_equal(steps_out, want_steps) and np.array_equal(flags, want_flags)
    assert same_bits(reward, want_reward) and (reward == 1.0).all()
    assert same_bits(before.reshape(-1, 4), state.astype(np.float32)) and same_bits(after.reshape(-1, 4), want.astype(np.float32))
    return want, want_flags


def test_cartpole_is_the_reference_on_random_states(drv):
    """4000 states x actions through the trait, both builds of the driver: RefCartPole bit for bit.  The sample ends episodes on each
    of the four sides and leaves others running (asserted)."""
    state, steps, actions = cartpole_random_cases()
    want, flags = check_against_ref_cartpole(drv, state, steps, actions, 500)
    running = (flags & 1) == 0
    assert running.any() and (want[:, 0] > cart.X_THRESHOLD).any() and (want[:, 0] < -cart.X_THRESHOLD).any()
    assert (want[:, 2] > cart.THETA_THRESHOLD).any() and (want[:, 2] < -cart.THETA_THRESHOLD).any()
    assert np.abs(want[running, 0]).max() <= cart.X_THRESHOLD and np.abs(want[running, 2]).max() <= cart.THETA_THRESHOLD
    assert not (flags & 2).any()
    # the limit is the caller's: one step below it is truncated
    _, flags12 = check_against_ref_cartpole(drv, state, np.full_like(steps, 11), actions, 12)
    assert (flags12 & 2).all() and np.array_equal(flags12 & 1, flags & 1)


def test_cartpole_is_the_reference_on_crafted_states(drv):
    """x across +2.4 and -2.4, theta across each threshold, and the same short of it; steps = 499 comes back truncated -- truncated ONLY
    where the step does not end the episode, terminated AND truncated where it does.  Every case is compared, every flag is seen."""
    cases = cart.crafted_states()
    state = np.array([c[1] for c in cases], dtype=np.float64)
    actions = np.array([c[2] for c in cases], dtype=np.int64)
    ends = np.array([c[3] for c in cases])
    assert ends.any() and not ends.all()
    want, flags = check_against_ref_cartpole(drv, state, np.full(len(cases), 499, dtype=np.int64), actions, 500)
    assert np.array_equal(flags, np.where(ends, 3, 2))   # (2: truncated only; 3: both)
    _, early = check_against_ref_cartpole(drv, state, np.full(len(cases), 11, dtype=np.int64), actions, 500)
    assert np.array_equal(early, np.where(ends, 1, 0))   # (1: terminated only; 0: the episode goes on)
    new = {c[0]: w for c, w in zip(cases, want)}
    assert state[0][0] < cart.X_THRESHOLD < new['x above 2.4'][0] and state[1][0] > -cart.X_THRESHOLD > new['x below -2.4'][0]
    assert state[2][2] < cart.THETA_THRESHOLD < new['theta above its threshold'][2]
    assert state[3][2] > -cart.THETA_THRESHOLD > new['theta below minus its threshold'][2]
    assert abs(new['x stays inside'][0]) < cart.X_THRESHOLD and abs(new['theta stays inside'][2]) < cart.THETA_THRESHOLD
    assert min(cart.decision_margin(c[1], c[2]) for c in cases) > 1e-3   # (none of them sits on a decision: the GPU test reuses them)


def test_cartpole_reset_is_the_restatement(drv):
    from rlzero_amd.muzero.cartpole import initial_states
    rng = np.random.RandomState(2)
    env = np.concatenate([np.arange(40), rng.randint(0, 2 ** 20, size=200)]).astype(np.int64)
    episode = np.concatenate([np.zeros(40), rng.randint(0, 2 ** 40, size=200)]).astype(np.int64)
    for seed in (0, 7, 2 ** 64 - 1):
        got, steps = drv.run('cartpole_reset', [seed], [env, episode], [np.float64, np.int64])
        want = initial_states(seed, env, episode)
        assert same_bits(got.reshape(-1, 4), want) and not steps.any()
        assert want.min() >= -0.05 and want.max() < 0.05
        assert want.std() > 0.025 and abs(want.mean()) < 0.005   # (uniform over the range: 0.1 / sqrt(12) = 0.0289)


@pytest.mark.parametrize('A', [2, 3, 8])
def test_the_headers_noise_key_is_the_restatement(drv, A):
    """``noise_key`` under ``move_key`` with salt 0: the 32-bit key of every action's gamma draw, as device_streams.muzero_action_keys."""
    rng = np.random.RandomState(A)
    env, episode, steps = (rng.randint(0, hi, size=3000).astype(np.int64) for hi in (8192, 1000, 500))
    for seed in (11, 2 ** 64 - 1):
        got, = drv.run('noise_keys', [A, seed], [env, episode, steps], [np.uint32])
        want = ds.muzero_action_keys(seed, env, episode, steps, A)
        assert np.array_equal(got.reshape(-1, A).astype(np.uint64), want)
    assert len(np.unique(got)) > 0.99 * got.size


@pytest.mark.parametrize('D,A', [(4, 2), (6, 3)])
def test_the_record_layout_is_the_documented_one(drv, D, A):
    """obs (D) | action | reward | visits (A) | root value | done: D + 4 + A doubles, 8 + A for CartPole (include/rlzero_hip.h)."""
    got, = drv.run('layout', [D, A], [], [np.int32])
    assert got.tolist() == [D, D + 1, D + 2, D + 2 + A, D + 3 + A, D + 4 + A]
    if D == 4:
        assert got[5] == 8 + A
    header = open(os.path.join(REPO, 'include', 'rlzero_hip.h')).read()
    assert 'a record is 8 + A float64 -- observation before the move (4) | action | reward | visit' in header
    assert 'obs (D) | action | reward | visits (A) | root value | done' in header and '[ring_steps][D + 4 + A]' in header


@pytest.mark.parametrize('variant', cart.VARIANTS)
def test_the_gpu_bound_catches_cartpole_rule_errors(variant):
    """As for Acrobot below: RefCartPole's step with tau changed, the 4 / 3 dropped or the force's sign swapped is more than 1e-4 away
    from the true one in at least one of the random states (figures printed); the GPU tests allow 1e-9."""
    state, steps, actions = cartpole_random_cases()
    true, _, _, _ = cartpole_ref_steps(state, steps, actions, 500)
    broken, _, _, _ = cartpole_ref_steps(state, steps, actions, 500, variant)
    worst = np.abs(broken - true).max(axis=1)
    print('%s: largest difference %.3g, %d of %d states above %g' % (variant, worst.max(), int((worst > CAUGHT_ABOVE).sum()), len(worst), CAUGHT_ABOVE))
    assert (worst > CAUGHT_ABOVE).any() and CAUGHT_ABOVE >= 1e5 * GPU_BOUND


@pytest.mark.parametrize('variant', twin.VARIANTS)
def test_the_gpu_bound_catches_rule_errors(variant):
    """The GPU test allows 1e-9.  A twin with one rule broken is more than 1e-4 away -- five orders above that -- in at least one
    of the random states (figures printed)."""
    state, steps, actions = random_cases()
    true, _, _, _ = twin_steps(state, steps, actions, 500)
    broken, _, _, _ = twin_steps(state, steps, actions, 500, variant)
    diff = np.abs(broken - true)
    diff[:, :2] = np.minimum(diff[:, :2], np.abs(diff[:, :2] - 2.0 * twin.PI))   # (angles are compared on the circle)
    worst = diff.max(axis=1)
    print('%s: largest difference %.3g, %d of %d states above %g' % (variant, worst.max(), int((worst > CAUGHT_ABOVE).sum()), len(worst), CAUGHT_ABOVE))
    assert (worst > CAUGHT_ABOVE).any() and CAUGHT_ABOVE >= 1e5 * GPU_BOUND


def load_trainer():
    spec = importlib.util.spec_from_file_location('train_muzero', os.path.join(REPO, 'tools', 'train_muzero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_trainers_parser_takes_the_environment(capsys):
    import inspect
    mod = load_trainer()
    ap = mod.build_parser()
    assert ap.parse_args([]).env == 'cartpole'
    assert ap.parse_args(['--env', 'acrobot']).env == 'acrobot'
    with pytest.raises(SystemExit):
        ap.parse_args(['--env', 'pendulum'])
    assert 'pendulum' in capsys.readouterr().err
    params = inspect.signature(mod.MuZeroPipeline.__init__).parameters
    assert params['env'].default == 'cartpole' and params['max_episode_steps'].default is None
    with pytest.raises(ValueError, match='pendulum'):
        mod.MuZeroPipeline(env='pendulum')


def test_device_moves_are_exported_and_bound():
    """The module, the symbols and the ABI number of this feature (none of them exists before it)."""
    from rlzero_amd import _hip, muzero
    assert muzero.AcrobotBatch.n_actions == 3 and muzero.AcrobotBatch.obs_dim == 6 and muzero.AcrobotBatch.kind == 'acrobot'
    assert muzero.CartPoleBatch.kind == 'cartpole'
    assert {'rz_mz_env_step', 'rz_mz_env_move', 'rz_mz_root_noise'} <= set(_hip.exported_symbols())
    assert _hip.ABI_VERSION >= 41 and _hip.MZ_ENV_KINDS == {'cartpole': 0, 'acrobot': 1}
    header = open(os.path.join(REPO, 'include', 'rlzero_hip.h')).read()
    assert '#define RZ_MZ_ENV_CARTPOLE 0' in header and '#define RZ_MZ_ENV_ACROBOT 1' in header
    # rz_mz_env_play: 4 pointers, 2 uint64, double, int64, pointer, 2 int32, int64, pointer, int64, 2 pointers, int64, pointer
    import ctypes
    assert ctypes.sizeof(_hip.RzMzEnvPlay) == 136 and _hip.RzMzEnvPlay.step.offset == 80 and _hip.RzMzEnvPlay.d_obs.offset == 128
    import inspect
    from rlzero_amd.muzero.selfplay import MuZeroSelfPlay
    assert inspect.signature(MuZeroSelfPlay.__init__).parameters['device_moves'].default is None
