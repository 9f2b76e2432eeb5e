"""The MuZero learner's unrolled targets (rlzero_amd/csrc/rz_mz_target.h) on the CPU, against the host buffer they restate.

A driver with its own main is compiled against the header with ROCm's clang++ (by tests/host_driver.py) with
-ffp-contract=off, fed binary inputs and compared in numpy with rlzero_amd/muzero/selfplay.py: ReplayBuffer.sample BIT FOR BIT --
value targets, rewards, masks, actions and policy rows of hand-made episodes -- and with EpisodeSeq.fields_of_packed (the policy of
a packed record) and rlzero_amd/muzero/replay.py: mz_replay_draws (the sampler's draws).  The draws fed to the driver are the host
buffer's own: its RandomState is seeded and its draw sequence replayed (randint for the episodes, then for the positions, then the
filler actions in (b, k) order); a second pass scripts the generator so that EVERY (episode, position) is an entry.  The same driver
is also built with -fsanitize=address,undefined and run over all inputs (a stand-alone program)."""
import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import host_driver
from rlzero_amd.muzero.replay import mz_replay_draws
from rlzero_amd.muzero.selfplay import EpisodeSeq, ReplayBuffer

MAX_STEPS = 12
CONFIGS = [(2, 3), (5, 10)]       # (K, td_steps)
DISCOUNTS = [0.5, 0.997]

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

// rows K td T disc.f64 [td + 1] lengths.i32 [E] reward.f64 [E][T] value.f64 [E][T] action.i32 [E][T] draws.i64 [n][K + 2]
//   -> tv.f32 tr.f32 mask.f32 [n][K + 1], policy_step.i32 [n][K + 1], actions.i64 [n][K]
static int rows(char **a) {
    const int K = atoi(a[0]), td = atoi(a[1]), T = atoi(a[2]);
    const std::vector<double> disc = load<double>(a[3]);
    const std::vector<int32_t> lengths = load<int32_t>(a[4]);
    const std::vector<double> reward = load<double>(a[5]), value = load<double>(a[6]);
    const std::vector<int32_t> action = load<int32_t>(a[7]);
    const std::vector<int64_t> draws = load<int64_t>(a[8]);
    const size_t E = lengths.size(), n = draws.size() / (K + 2);
    if ((int)disc.size() != td + 1 || reward.size() != E * T || value.size() != E * T || action.size() != E * T) return 4;
    std::vector<float> tv(n * (K + 1)), tr(n * (K + 1)), mask(n * (K + 1));
    std::vector<int32_t> pstep(n * (K + 1));
    std::vector<int64_t> actions(n * K);
    for (size_t b = 0; b < n; ++b) {
        const int64_t *dr = draws.data() + b * (K + 2);
        const size_t e = (size_t)dr[0];
        if (e >= E || lengths[e] < 0 || lengths[e] > T || dr[1] < 0 || dr[1] >= lengths[e]) return 5;
        const int len = lengths[e];
        // (heap arrays of exactly the episode's length: a read past the end is the sanitizer's to report)
        const std::vector<double> rw(reward.begin() + e * T, reward.begin() + e * T + len), rv(value.begin() + e * T, value.begin() + e * T + len);
        const std::vector<int32_t> ac(action.begin() + e * T, action.begin() + e * T + len);
        for (int k = 0; k <= K; ++k) {
            const rt::Row r = rt::unroll_row(rw.data(), rv.data(), ac.data(), len, (int)dr[1], k, td, disc.data(), k > 0 ? dr[2 + k - 1] : 0);
            const size_t o = b * (K + 1) + k;
            tv[o] = r.value, tr[o] = r.reward, mask[o] = r.mask, pstep[o] = r.policy_step;
            if (k > 0) actions[b * K + k - 1] = r.action;
        }
    }
    store(a[9], tv);
    store(a[10], tr);
    store(a[11], mask);
    store(a[12], pstep);
    store(a[13], actions);
    return 0;
}

// policy D A final rows.f64 [R][D + 4 + A] -> policy.f32 [R][A] then uniform_policy(A), one float
static int policy(char **a) {
    const int D = atoi(a[0]), A = atoi(a[1]), final_policy = atoi(a[2]);
    const std::vector<double> in = load<double>(a[3]);
    const size_t W = D + 4 + A, R = in.size() / W;
    std::vector<float> out(R * A + 1);
    for (size_t r = 0; r < R; ++r) {
        const std::vector<double> row(in.begin() + r * W, in.begin() + (r + 1) * W);
        for (int c = 0; c < A; ++c) out[r * A + c] = rt::policy_of_row(row.data(), D, A, c, final_policy != 0);
    }
    out[R * A] = rt::uniform_policy(A);
    store(a[4], out);
    return 0;
}

// draws seed step n K A lengths.i32 [E] -> i64 [n][K + 2]
static int draws(char **a) {
    const uint64_t seed = strtoull(a[0], nullptr, 10), step = strtoull(a[1], nullptr, 10);
    const int n = atoi(a[2]), K = atoi(a[3]), A = atoi(a[4]);
    const std::vector<int32_t> lengths = load<int32_t>(a[5]);
    std::vector<int64_t> out((size_t)n * (K + 2));
    for (int i = 0; i < n; ++i) {
        int64_t *o = out.data() + (size_t)i * (K + 2);
        o[0] = rt::draw(seed, step, rt::draw_counter((uint64_t)i, K, 0), lengths.size());
        o[1] = rt::draw(seed, step, rt::draw_counter((uint64_t)i, K, 1), (uint64_t)lengths[(size_t)o[0]]);
        for (int k = 0; k < K; ++k) o[2 + k] = rt::draw(seed, step, rt::draw_counter((uint64_t)i, K, 2 + k), (uint64_t)A);
    }
    store(a[6], out);
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "rows" && argc == 16) return rows(argv + 2);
    if (what == "policy" && argc == 7) return policy(argv + 2);
    if (what == "draws" && argc == 9) return draws(argv + 2);
    return 4;
}
'''


drv = host_driver.fixture('mz_target', DRIVER)


# ----------------------------------------------------------------------------------------------- hand-made episodes
def episode_lengths(K, td, T=MAX_STEPS):
    """1, 2, K, td_steps, td_steps + 1 and the longest a slot of T steps holds (in this order; equal ones stay: a buffer may hold
    them)."""
    return [1, 2, K, td, td + 1, T]


def packed_block(rng, lengths, D, A):
    """Packed records (obs | action | reward | visit counts | root value | done) of episodes of these lengths, one behind the
    other: non-constant rewards and root values with full float64 mantissas, integer visit counts, done on the last step."""
    n = int(np.sum(lengths))
    block = np.zeros((n, D + 4 + A), dtype=np.float64)
    block[:, :D] = rng.standard_normal((n, D)) * 1.7
    block[:, D] = rng.randint(A, size=n)
    block[:, D + 1] = rng.uniform(0.25, 1.75, size=n) * np.where(rng.uniform(size=n) < 0.2, -1.0, 1.0)
    vis = rng.randint(0, 40, size=(n, A)).astype(np.float64)
    vis[np.arange(n), rng.randint(A, size=n)] += 1.0   # (never all zero)
    block[:, D + 2:D + 2 + A] = vis
    block[:, D + 2 + A] = rng.standard_normal(n) * 9.3
    if n:
        block[np.cumsum(lengths) - 1, D + 3 + A] = 1.0
    return block


def episodes_of(block, lengths, D, A):
    """The Episode objects the host route makes of a packed block (EpisodeSeq.fields_of_packed)."""
    seq = EpisodeSeq()
    seq._add_packed(block, D, A, lengths)
    return list(seq)


def replayed_draws(buf, batch, A):
    """(ep_idx [b], pos [b], filler [b, K]) of the NEXT ``buf.sample(batch, A)``: its RandomState's draw sequence replayed on a copy
    of the generator -- randint for the episodes, then one per position, then a filler per (b, k) whose step lies past the end."""
    rng = np.random.RandomState()
    rng.set_state(buf.rng.get_state())
    ep_idx = rng.randint(len(buf.episodes), size=batch)
    pos = np.array([rng.randint(len(buf.episodes[e])) for e in ep_idx], dtype=np.int64)
    filler = np.zeros((batch, buf.K), dtype=np.int64)
    for b in range(batch):
        for k in range(1, buf.K + 1):
            if pos[b] + k - 1 >= len(buf.episodes[ep_idx[b]]):
                filler[b, k - 1] = rng.randint(A)
    return ep_idx.astype(np.int64), pos, filler


class ScriptedDraws(object):
    """Stands in for the host buffer's RandomState: ``sample`` then draws exactly (ep_idx, pos, filler)."""

    def __init__(self, buf, ep_idx, pos, filler):
        self.ep_idx = np.asarray(ep_idx)
        self.queue = [int(p) for p in pos]
        for b, (e, p) in enumerate(zip(ep_idx, pos)):
            for k in range(1, buf.K + 1):
                if p + k - 1 >= len(buf.episodes[e]):
                    self.queue.append(int(filler[b, k - 1]))

    def randint(self, high, size=None):
        if size is not None:
            assert size == len(self.ep_idx)
            return self.ep_idx
        v = self.queue.pop(0)
        assert 0 <= v < high
        return v


def every_position(lengths, K, A, rng):
    """Draws that make every (episode, position) an entry, with random filler actions."""
    ep_idx = np.repeat(np.arange(len(lengths)), lengths).astype(np.int64)
    pos = np.concatenate([np.arange(m) for m in lengths]).astype(np.int64)
    return ep_idx, pos, rng.randint(A, size=(len(ep_idx), K)).astype(np.int64)


def host_sample(buf, draws, A):
    """ReplayBuffer.sample's six arrays for scripted draws (the buffer's own generator is put back)."""
    keep = buf.rng
    buf.rng = ScriptedDraws(buf, *draws)
    try:
        out = buf.sample(len(draws[0]), A)
        assert not buf.rng.queue
    finally:
        buf.rng = keep
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def driver_sample(drv, episodes, K, td, discount, draws, A, T=MAX_STEPS):
    """The six arrays from the header's functions: rows through the driver, the policy rows and the observation looked up here."""
    ep_idx, pos, filler = draws
    E, n = len(episodes), len(ep_idx)
    lengths = np.array([len(ep) for ep in episodes], dtype=np.int32)
    reward, value = np.zeros((E, T)), np.zeros((E, T))
    action = np.zeros((E, T), dtype=np.int32)
    for e, ep in enumerate(episodes):
        reward[e, :len(ep)], value[e, :len(ep)], action[e, :len(ep)] = ep.rewards, ep.root_values, ep.actions
    disc = np.array([discount ** i for i in range(td + 1)], dtype=np.float64)
    table = np.concatenate((ep_idx[:, None], pos[:, None], filler), axis=1).astype(np.int64)
    tv, tr, mask, pstep, actions = drv.run('rows', [K, td, T], [disc, lengths, reward, value, action, table],
                                           [np.float32, np.float32, np.float32, np.int32, np.int64])
    pstep = pstep.reshape(n, K + 1)
    _, uniform = policy_rows(drv, np.zeros((0, 4 + A)), 0, A, False)
    tp = np.empty((n, K + 1, A), dtype=np.float32)
    for b in range(n):
        for k in range(K + 1):
            tp[b, k] = episodes[ep_idx[b]].policies[pstep[b, k]] if pstep[b, k] >= 0 else uniform
    obs = np.stack([episodes[e].obs[p] for e, p in zip(ep_idx, pos)]).astype(np.float32)
    return obs, actions.reshape(n, K), tv.reshape(n, K + 1), tr.reshape(n, K + 1), tp, mask.reshape(n, K + 1)


def policy_rows(drv, block, D, A, final):
    out, = drv.run('policy', [D, A, int(final)], [block], [np.float32])
    return out[:-1].reshape(-1, A), out[-1]


def assert_same_batch(got, want):
    for name, g, w in zip(('obs', 'actions', 'tv', 'tr', 'tp', 'mask'), got, want):
        assert same_bits(g, w), name


def boundary_kinds(buf, draws, got, A):
    """How many rows of the batch ``got`` (raw targets: no value transform) of ``draws`` from the host buffer ``buf`` are of each
    of the four boundary kinds, every such row held to what the rules say about it."""
    ep_idx, pos, filler = draws
    K, td, discount = buf.K, buf.td_steps, buf.discount
    obs, actions, tv, tr, tp, mask = got
    seen = {'boot == len': 0, 'boot == len - 1': 0, 'pos + k == len': 0, 'past the end': 0}
    for b in range(len(pos)):
        ep = buf.episodes[ep_idx[b]]
        m = len(ep)
        for k in range(K + 1):
            i = pos[b] + k
            if i < m and i + td == m:      # no bootstrap: the discounted rewards to the end alone
                seen['boot == len'] += 1
                assert tv[b, k] == np.float32(sum(ep.rewards[i + j] * discount ** j for j in range(td)))
            if i < m and i + td == m - 1:  # bootstrapped from the last step's root value
                seen['boot == len - 1'] += 1
                assert tv[b, k] == np.float32(buf._value_target(ep, i)) and ep.root_values[m - 1] != 0.0
            if k > 0 and i == m:           # the last step's action and reward are real, policy and mask are off
                seen['pos + k == len'] += 1
                assert actions[b, k - 1] == ep.actions[m - 1] and tr[b, k] == np.float32(ep.rewards[m - 1])
                assert mask[b, k] == 0.0 and tv[b, k] == 0.0 and (tp[b, k] == np.float32(1.0 / A)).all()
            if k > 0 and i > m:
                seen['past the end'] += 1
                assert actions[b, k - 1] == filler[b, k - 1] and tr[b, k] == 0.0 and mask[b, k] == 0.0
    return seen


def kinds_that_exist(K, td, T):
    """Which boundary kinds a buffer of slots of T steps can show at all.  A return that ends exactly at the episode's end needs
    an episode of td steps, one bootstrapped from the last step an episode of td + 1; row k = 1 of the last position always has
    pos + k == len; a row PAST the end needs K >= 2, since pos <= len - 1 puts row 1 at len at the most."""
    return {'boot == len': T >= td, 'boot == len - 1': T >= td + 1, 'pos + k == len': True, 'past the end': K >= 2}


# ----------------------------------------------------------------------------------------------- the corners
# The limits rz_mz_replay_create accepts (obs_dim 1 .. 16, n_actions 1 .. 8, unroll_steps 1 .. 16, td_steps 1 .. 64), each at its
# largest and its smallest value, and the trainer's own shape: slots of 500 steps in a ring of hundreds of episodes that wraps.
# T = 80 is the smallest slot above td + K = 64 + 16.  The CPU tests hold the header to the host buffer at these shapes, the GPU
# tests (tests/test_mz_replay_limits_gpu.py) the kernels; both take the episodes, the arbiter and the entries from ``corner``.
CORNERS = {
    'MAX': dict(D=16, A=8, K=16, td=64, T=80, capacity=5, discount=0.997),
    'MIN': dict(D=1, A=1, K=1, td=1, T=1, capacity=1, discount=0.5),
    'TALL': dict(D=16, A=1, K=16, td=1, T=80, capacity=5, discount=0.5),
    'WIDE': dict(D=1, A=8, K=1, td=64, T=80, capacity=5, discount=0.997),
    'REAL': dict(D=4, A=2, K=5, td=10, T=500, capacity=300, discount=0.997),
}
REAL_CALLS = (350, 250, 100)   # 700 episodes: the first call alone overfills the ring of 300, and the ring wraps twice


class Corner(object):
    """One corner's episodes in the three calls that store them, and the host ``ReplayBuffer`` fed the same episodes: made once
    (``corner``), shared by the tests and written by none of them.
    The small corners: the distinct values of 1, 2, K, K + 1, td, td + 1 and T, clipped to T, then two more episodes (2 and 1
    steps, so that short episodes are among those held at the end); more episodes than the ring has slots, cut into three calls.
    REAL: 700 lengths drawn from 1 .. 500 with 1, 499 and 500 forced in among the 300 held at the end, in calls of REAL_CALLS."""

    def __init__(self, name):
        self.name = name
        self.__dict__.update(CORNERS[name])
        D, A, K, td, T = self.D, self.A, self.K, self.td, self.T
        rng = np.random.RandomState(sum(ord(ch) for ch in name))
        if name == 'REAL':
            lengths = rng.randint(1, T + 1, size=sum(REAL_CALLS))
            lengths[[450, 500, 650]] = 1, T - 1, T
            sizes = REAL_CALLS
        else:
            lengths = sorted({min(v, T) for v in (1, 2, K, K + 1, td, td + 1, T)}) + [min(2, T), 1]
            sizes = (len(lengths) // 3, len(lengths) // 3, len(lengths) - 2 * (len(lengths) // 3))
        self.lengths = [int(v) for v in lengths]
        assert len(self.lengths) > self.capacity and min(sizes) >= 1
        host = self.arbiter(held=[])
        self.calls, self.held, at = [], [], 0   # (lengths, packed block, Episodes) per call; the arbiter's episodes after it
        for size in sizes:
            lens = self.lengths[at:at + size]
            block = packed_block(rng, lens, D, A)
            eps = episodes_of(block, lens, D, A)
            for ep in eps:
                host.add(ep)
            self.calls.append((lens, block, eps))
            self.held.append(list(host.episodes))
            at += size
        # the episode held in slot 0 of a ring of `capacity` slots after this many adds: the one past the ring's seam
        self.seam = self.capacity - len(self.lengths) % self.capacity

    def arbiter(self, call=-1, value_transform=False, held=None):
        """The host buffer as it stood after ``call``; its episodes are the shared ones (``sample`` only reads them)."""
        buf = ReplayBuffer(capacity=self.capacity, unroll_steps=self.K, td_steps=self.td, discount=self.discount, seed=11,
                           value_transform=value_transform)
        buf.episodes = list(self.held[call]) if held is None else held
        return buf

    def named(self):
        """REAL's subset of the episodes held: the oldest, the newest, the shortest, the longest and the two on either side of
        the ring's seam (the last slot and slot 0)."""
        lens = [len(ep) for ep in self.held[-1]]
        return sorted({0, len(lens) - 1, int(np.argmin(lens)), int(np.argmax(lens)), self.seam - 1, self.seam % len(lens)})

    def positions(self):
        """(ep_idx, pos) of every step held; on REAL of every step of the ``named`` episodes (the CPython arbiter stays in seconds)."""
        lens = [len(ep) for ep in self.held[-1]]
        which = self.named() if self.name == 'REAL' else range(len(lens))
        ep_idx = np.repeat(np.array(list(which), dtype=np.int64), [lens[j] for j in which])
        return ep_idx, np.concatenate([np.arange(lens[j]) for j in which]).astype(np.int64)

    def entries(self, rng):
        """The draws ``gather`` is held to: ``positions`` with random fillers; on REAL 512 draws of the sampler's stream as well."""
        ep_idx, pos = self.positions()
        filler = rng.randint(self.A, size=(len(ep_idx), self.K)).astype(np.int64)
        if self.name != 'REAL':
            return ep_idx, pos, filler
        more = mz_replay_draws(5, 0, 512, [len(ep) for ep in self.held[-1]], self.K, self.A)
        return tuple(np.concatenate(pair) for pair in zip((ep_idx, pos, filler), more))


_corners = {}


def corner(name):
    if name not in _corners:
        _corners[name] = Corner(name)
    return _corners[name]


# ----------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize('discount', DISCOUNTS)
@pytest.mark.parametrize('K,td', CONFIGS)
@pytest.mark.parametrize('A', [2, 3])
def test_rows_equal_the_host_buffers_sample(drv, K, td, discount, A):
    """Seeded host buffer, its draw sequence replayed, the driver fed those draws: all six arrays bit for bit; then every
    (episode, position) through a scripted generator."""
    D = 4
    rng = np.random.RandomState(1000 * K + A)
    lengths = episode_lengths(K, td)
    episodes = episodes_of(packed_block(rng, lengths, D, A), lengths, D, A)
    buf = ReplayBuffer(capacity=len(lengths), unroll_steps=K, td_steps=td, discount=discount, seed=11)
    for ep in episodes:
        buf.add(ep)
    for _ in range(2):
        draws = replayed_draws(buf, 256, A)
        want = buf.sample(256, A)
        assert_same_batch(driver_sample(drv, episodes, K, td, discount, draws, A), want)
    draws = every_position(lengths, K, A, rng)
    want = host_sample(buf, draws, A)
    got = driver_sample(drv, episodes, K, td, discount, draws, A)
    assert_same_batch(got, want)
    # the boundary cases are among them, and they look as the rules say
    seen = boundary_kinds(buf, draws, got, A)
    assert all(seen.values()), seen


@pytest.mark.parametrize('name', sorted(CORNERS))
def test_rows_equal_the_host_buffers_sample_at_the_corners(drv, name):
    """The same at the limits rz_mz_replay_create accepts and at the trainer's shape: the corner's entries (every (episode,
    position) held; a subset on REAL) bit for bit, and every boundary kind that exists at the shape is among them."""
    c = corner(name)
    buf = c.arbiter()
    draws = c.entries(np.random.RandomState(7))
    want = host_sample(buf, draws, c.A)
    got = driver_sample(drv, buf.episodes, c.K, c.td, c.discount, draws, c.A, T=c.T)
    assert_same_batch(got, want)
    seen = boundary_kinds(buf, draws, got, c.A)
    print('%s: %d entries, %d rows, boundary kinds %r' % (name, len(draws[0]), len(draws[0]) * (c.K + 1), seen))
    assert {kind: n > 0 for kind, n in seen.items()} == kinds_that_exist(c.K, c.td, c.T), seen


@pytest.mark.parametrize('A', [1, 2, 3, 8])
def test_policy_of_a_packed_record(drv, A):
    """visits / sum(visits) in fp64, cast to float32: EpisodeSeq.fields_of_packed's bits; a final policy is only cast."""
    D = 4
    rng = np.random.RandomState(A)
    block = packed_block(rng, [40], D, A)
    block[:5, D + 2:D + 2 + A] = rng.randint(1, 2 ** 30, size=(5, A))   # (large counts: the sum stays exact)
    got, uniform = policy_rows(drv, block, D, A, False)
    assert same_bits(got, EpisodeSeq.fields_of_packed(block, D, A)[3])
    assert same_bits(np.float32(uniform), np.full(1, 1.0 / A, dtype=np.float32)[0])
    final = block.copy()
    final[:, D + 2:D + 2 + A] = got
    again, _ = policy_rows(drv, final, D, A, True)
    assert same_bits(again, got)


@pytest.mark.parametrize('K,A', [(1, 1), (2, 2), (5, 3), (16, 8)])
def test_draws_equal_the_restatement(drv, K, A):
    lengths = np.array([1, 2, 5, 500, 7, 12, 1], dtype=np.int32)
    for seed, step in ((0, 0), (13, 1), (2 ** 64 - 1, 2 ** 40 + 3)):
        got, = drv.run('draws', [seed, step, 300, K, A], [lengths], [np.int64])
        got = got.reshape(300, K + 2)
        ep, pos, filler = mz_replay_draws(seed, step, 300, lengths, K, A)
        assert np.array_equal(got[:, 0], ep) and np.array_equal(got[:, 1], pos) and np.array_equal(got[:, 2:], filler)
        assert (ep >= 0).all() and (ep < len(lengths)).all() and (pos >= 0).all() and (pos < lengths[ep]).all()
        assert (filler >= 0).all() and (filler < A).all()
        assert len(set(ep.tolist())) == len(lengths) and len(set(filler.reshape(-1).tolist())) == A   # (every value occurs)
    a, b = mz_replay_draws(5, 0, 64, lengths, K, A), mz_replay_draws(5, 1, 64, lengths, K, A)
    assert not np.array_equal(a[0], b[0])   # the update's number keys the stream
