"""MuZero prioritized replay on the GPU (rlzero_amd/muzero/replay.py; csrc/rz_mz_replay.hip: k_mzr_prio, k_mzr_scan,
k_mzr_draw_prio), bit for bit against the host restatements (mz_priority_weights, mz_prioritized_draws): the integer priorities
of every step held after adds that wrap the ring, the two searches at EVERY boundary of the prefix sums (targets handed in), the
in-episode scan across wave and chunk boundaries, the episode scan across every thread's run, enabling late, ingest, the
priorities following a Reanalyse write-back, the mini-batch and its importance weights, the feature switched off, and the lazy
refresh on a stream of the caller's."""
import ctypes

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
from test_mz_replay_gpu import CAPACITY, D, filled, on_host
from test_mz_replay_host import MAX_STEPS, assert_same_batch, episodes_of, host_sample, packed_block, same_bits

pytestmark = pytest.mark.gpu


def restated(episodes, td, discount):
    from rlzero_amd.muzero import mz_priority_weights
    return [mz_priority_weights(ep.rewards, ep.root_values, td, discount) for ep in episodes]


def same_weights(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w)
    return True


def boundaries(weights):
    """0, total - 1 and c - 1, c for every cumulative value c of the steps in order (c = total itself left out)."""
    cum = np.cumsum(np.concatenate(weights))
    total = int(cum[-1])
    t = np.unique(np.concatenate((cum - 1, cum, [0, total - 1])))
    return t[(t >= 0) & (t < total)].astype(np.int64), total


def draws_equal(dev, weights, n=None, step=0, targets=None):
    from rlzero_amd.muzero import mz_prioritized_draws
    got = on_host(dev.prioritized_draws(n, step=step, targets=targets))
    want = mz_prioritized_draws(dev.seed, step, n, weights, dev.K, dev.n_actions, targets=targets)
    assert [g.dtype for g in got] == [np.int64, np.int64, np.int64, np.float64]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert same_bits(got[3], want[3])
    return got


def dev_t(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev.device)


# ----------------------------------------------------------------------------------------------- 1. the small ring
@pytest.mark.parametrize('K,td,discount', [(2, 3, 0.5), (5, 10, 0.997)])
def test_small_ring_weights_and_every_boundary(K, td, discount):
    from rlzero_amd import _hip
    A = 3
    dev, host, _ = filled(K, td, discount, A)
    dev.enable_priorities()
    weights = dev.priorities()
    assert same_weights(weights, restated(host.episodes, td, discount))
    targets, total = boundaries(weights)
    assert len(targets) >= 2 * sum(len(w) for w in weights) - 2
    ep, pos, _, prob = draws_equal(dev, weights, step=5, targets=targets)
    steps = [(e, t) for e, w in enumerate(weights) for t in range(len(w))]
    assert sorted(set(zip(ep.tolist(), pos.tolist()))) == steps                                   # every step is reached
    assert same_bits(prob, np.array([float(weights[e][t]) / float(total) for e, t in zip(ep, pos)], dtype=np.float64))
    draws_equal(dev, weights, step=5, targets=dev_t(dev, targets))                                # the same targets from the device
    # a target of `total` (and a negative one): the flag, the public call raises
    for bad in (total, -1):
        with pytest.raises(_hip.HipError):
            dev.prioritized_draws(None, step=0, targets=np.array([0, bad], dtype=np.int64))
    assert dev.poll_errors() == 0
    # ... and through the pieces: that entry's draw row is all -1, and the gather that follows refuses it and leaves its rows alone
    t4 = np.array([0, total, total - 1, -1], dtype=np.int64)
    draws, prob = dev._draw_prioritized(None, 0, t4)
    out = dev._outputs(4)
    for x in out:
        x.fill_(77)
    _hip.check(dev.lib.rz_mz_replay_gather(dev.handle, None, draws.data_ptr(), 4, *[x.data_ptr() for x in out], dev._stream()), 'rz_mz_replay_gather')
    assert dev.poll_errors() == _hip.MZ_REPLAY_BAD_INDEX
    draws, prob = draws.cpu().numpy(), prob.cpu().numpy()
    assert (draws[[1, 3]] == -1).all() and (prob[[1, 3]] == 0.0).all()
    assert draws[0, :2].tolist() == [0, 0] and draws[2, :2].tolist() == [len(weights) - 1, len(weights[-1]) - 1]
    good = on_host(dev.gather(draws[[0, 2], 0], draws[[0, 2], 1], draws[[0, 2], 2:]))
    for x, g in zip(on_host(out), good):
        assert (x[[1, 3]] == 77).all() and same_bits(x[[0, 2]], g)
    dev.close()


# ----------------------------------------------------------------------------------------------- 2. the scans
def test_long_episodes_cross_wave_and_chunk_boundaries():
    from rlzero_amd.muzero import MuZeroDeviceReplay
    K, td, discount, A, T = 5, 10, 0.997, 2, 600
    lengths = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 600]
    dev = MuZeroDeviceReplay(D, A, len(lengths), T, unroll_steps=K, td_steps=td, discount=discount, seed=9, prioritized=True)
    block = packed_block(np.random.RandomState(21), lengths, D, A)
    assert dev.add_packed(block, lengths) == len(lengths)
    weights = dev.priorities()
    assert same_weights(weights, restated(episodes_of(block, lengths, D, A), td, discount))
    # the prefixes the searches walk: both boundaries of every step resolve to that step
    targets, total = boundaries(weights)
    ep, pos, _, _ = draws_equal(dev, weights, step=0, targets=targets)
    assert len(set(zip(ep.tolist(), pos.tolist()))) == sum(lengths)
    draws_equal(dev, weights, n=512, step=1)
    dev.close()


def test_many_episodes_cross_every_threads_run():
    from rlzero_amd.muzero import MuZeroDeviceReplay
    K, td, discount, A, cap = 2, 3, 0.5, 2, 3000
    rng = np.random.RandomState(4)
    dev = MuZeroDeviceReplay(D, A, cap, 3, unroll_steps=K, td_steps=td, discount=discount, seed=6, prioritized=True)
    blocks, all_lengths = [], []
    for n in (1500, 1200, 800):   # 3500 episodes: the ring wraps, the oldest 500 are dropped
        lengths = rng.randint(1, 4, size=n)
        block = packed_block(rng, lengths, D, A)
        assert dev.add_packed(block, lengths) == n
        blocks.append(block), all_lengths.extend(int(v) for v in lengths)
    count, cursor, _ = dev._state()
    assert count == cap and cursor == 500
    assert np.array_equal(dev.lengths(), all_lengths[500:])
    weights = dev.priorities()
    kept = episodes_of(np.concatenate(blocks), all_lengths, D, A)[500:]
    assert same_weights(weights, restated(kept, td, discount))
    for step in (0, 1):
        ep, _, _, _ = draws_equal(dev, weights, n=4096, step=step)
        assert ep.min() < 100 and ep.max() >= cap - 100 and len(set(ep.tolist())) > 1000   # across the ring's seam and all runs
    dev.close()


# ----------------------------------------------------------------------------------------------- 3. the ways in
def test_enabling_late_and_ingest():
    import torch
    from rlzero_amd.muzero import MuZeroDeviceReplay
    K, td, discount, A = 5, 10, 0.997, 2
    rng = np.random.RandomState(8)
    calls = [[3, 12, 1], [11, 10], [2, 7]]   # seven episodes into a ring of four
    blocks = [packed_block(rng, lengths, D, A) for lengths in calls]
    kw = dict(unroll_steps=K, td_steps=td, discount=discount, seed=2)
    early = MuZeroDeviceReplay(D, A, CAPACITY, MAX_STEPS, prioritized=True, **kw)
    late = MuZeroDeviceReplay(D, A, CAPACITY, MAX_STEPS, **kw)
    through_ingest = MuZeroDeviceReplay(D, A, CAPACITY, MAX_STEPS, prioritized=True, **kw)
    for i, (block, lengths) in enumerate(zip(blocks, calls)):
        early.add_packed(block, lengths), late.add_packed(block, lengths)
        # the same episodes in a device arena with a gap of two rows in front of each
        first_rows = np.cumsum([2] * len(lengths)) + np.cumsum(lengths) - np.array(lengths)
        arena = np.full((int(first_rows[-1]) + lengths[-1] + 1, block.shape[1]), 5.0)
        for a, m, src in zip(first_rows, lengths, np.cumsum(lengths) - np.array(lengths)):
            arena[a:a + m] = block[src:src + m]
        through_ingest.ingest(torch.from_numpy(arena).to(through_ingest.device), lengths, first_rows)
        if i == 0:
            early.priorities()   # (a refresh between the calls: the later ones mark only what they write)
    assert not late.prioritized
    late.enable_priorities()
    episodes = [ep for block, lengths in zip(blocks, calls) for ep in episodes_of(block, lengths, D, A)][-CAPACITY:]
    want = restated(episodes, td, discount)
    for dev in (early, late, through_ingest):
        assert dev.prioritized and same_weights(dev.priorities(), want) and dev.poll_errors() == 0
        draws_equal(dev, want, n=64, step=0)
        dev.close()


# ----------------------------------------------------------------------------------------------- 4. Reanalyse moves the priorities
@pytest.mark.parametrize('K,td,discount', [(2, 3, 0.5), (5, 10, 0.997)])
def test_priorities_follow_a_write_back(K, td, discount):
    A = 2
    dev, host, rng = filled(K, td, discount, A)
    dev.enable_priorities()
    before = dev.priorities()
    lengths = [len(ep) for ep in host.episodes]
    assert lengths == [td, td + 1, MAX_STEPS, 3]
    # step s of the longest episode: its own priority and that of s - td, whose bootstrap it is, move; also the last step of the
    # second episode, the bootstrap of its first
    ep_idx, pos = np.array([2, 1], dtype=np.int64), np.array([td + 1, td], dtype=np.int64)
    where, _, ticket = dev.positions(ep_idx, pos)
    visits = rng.randint(1, 51, size=(2, A)).astype(np.int32)
    dev.update(where, dev_t(dev, visits), dev_t(dev, np.array([50, 50], dtype=np.int32)), dev_t(dev, np.array([123.25, -77.5])), ticket)
    after = dev.priorities()
    assert same_weights(after, restated(dev.read(), td, discount))
    moved = {(2, td + 1), (2, 1), (1, td), (1, 0)}
    for e in range(len(lengths)):
        for t in range(lengths[e]):
            assert (before[e][t] != after[e][t]) == ((e, t) in moved), (e, t)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[3], after[3])   # the untouched episodes
    # the next draws use the new table
    draws_equal(dev, after, n=256, step=0)
    targets, _ = boundaries(after)
    draws_equal(dev, after, step=0, targets=targets)
    dev.close()


# ----------------------------------------------------------------------------------------------- 5. the mini-batch
def test_sample_prioritized_is_draws_then_gather():
    import torch
    K, td, discount, A, n = 5, 10, 0.997, 3, 64
    dev, host, _ = filled(K, td, discount, A, seed=17)
    dev.enable_priorities()
    weights = dev.priorities()
    n_steps = sum(len(w) for w in weights)
    assert dev.step == 0
    batch, w1 = dev.sample_prioritized(n)                  # the internal counter, shared with ``sample``: update 0
    assert dev.step == 1
    ep, pos, filler, prob = draws_equal(dev, weights, n=n, step=0)
    assert dev.step == 1
    assert all(x.is_cuda for x in batch) and w1.is_cuda and w1.dtype == torch.float32 and tuple(w1.shape) == (n, )
    assert_same_batch(on_host(batch), on_host(dev.gather(ep, pos, filler)))
    assert_same_batch(on_host(batch), host_sample(host, (ep, pos, filler), A))
    for beta in (1.0, 0.4):
        again, w = dev.sample_prioritized(n, step=0, beta=beta)
        assert_same_batch(on_host(again), on_host(batch))
        want = ((n_steps * prob.astype(np.float64)) ** -beta).astype(np.float32)
        np.testing.assert_allclose(w.cpu().numpy(), want, rtol=1e-6, atol=0)
    assert same_bits(w1.cpu().numpy(), dev.sample_prioritized(n, step=0)[1].cpu().numpy())
    other, _ = dev.sample_prioritized(n)                   # update 1: other draws
    assert dev.step == 2 and not np.array_equal(on_host(other)[2], on_host(batch)[2])
    assert dev.poll_errors() == 0
    dev.close()


def test_the_learner_takes_the_weights():
    import torch
    from rlzero_amd.muzero import MuZeroAgent
    dev, _, _ = filled(5, 10, 0.997, 2)
    dev.enable_priorities()
    batch, weights = dev.sample_prioritized(32, step=0)
    made = []
    for _ in range(3):
        torch.manual_seed(3)
        made.append(MuZeroAgent(device='cuda:0'))
    a, b, c = made
    plain = a.learn(batch)
    assert b.learn(batch, weights=torch.ones(32, device=dev.device)) == plain
    for p, q in zip(a.net.parameters(), b.net.parameters()):
        assert torch.equal(p, q)
    out = c.learn(batch, weights=weights)
    assert out[1:] == plain[1:] and np.isfinite(out[0]) and out[0] != plain[0]
    dev.close()


# ----------------------------------------------------------------------------------------------- 6. off
def test_off_nothing_changes():
    from rlzero_amd import _hip
    K, td, A = 5, 10, 3
    off, _, _ = filled(K, td, 0.997, A, seed=17)
    on, _, _ = filled(K, td, 0.997, A, seed=17)
    on.enable_priorities()
    on.priorities()
    for call in (lambda: off.sample_prioritized(8), lambda: off.prioritized_draws(8), lambda: off.priorities(), lambda: off.refresh_priorities()):
        with pytest.raises(_hip.HipError):
            call()
    assert off.step == 0
    import torch
    draws, prob = torch.zeros((8, K + 2), dtype=torch.int64, device=off.device), torch.zeros(8, dtype=torch.float64, device=off.device)
    assert off.lib.rz_mz_replay_draw_prioritized(off.handle, 0, 0, 8, None, draws.data_ptr(), prob.data_ptr(), off._stream()) == -1   # RZ_ERR_ARG
    assert off.lib.rz_mz_replay_refresh_priorities(off.handle, off._stream()) == -1
    assert off.poll_errors() == 0 and int(draws.abs().sum()) == 0
    for step in (0, 1):   # ``sample`` gives the same bits with the feature on, off, and after prioritized draws
        assert_same_batch(on_host(off.sample(64, step)), on_host(on.sample(64, step)))
    off.close(), on.close()
    # an empty buffer with priorities on: refused, nothing drawn
    from rlzero_amd.muzero import MuZeroDeviceReplay
    empty = MuZeroDeviceReplay(D, A, CAPACITY, MAX_STEPS, prioritized=True)
    with pytest.raises(_hip.HipError):
        empty.prioritized_draws(4, step=0)
    assert empty.priorities() == []
    empty.close()


# ----------------------------------------------------------------------------------------------- 7. the caller's stream
def test_lazy_refresh_runs_on_the_callers_stream():
    """add, the prioritized draw (which refreshes first) and the gather on a stream of the caller's with no synchronisation between
    them; then a write-back and the next draw the same way."""
    import torch
    from rlzero_amd.muzero import MuZeroDeviceReplay
    K, td, discount, A, n = 5, 10, 0.997, 2, 256
    lengths = [513, 7, 600, 64, 1, 300]
    block = packed_block(np.random.RandomState(33), lengths, D, A)
    dev = MuZeroDeviceReplay(D, A, len(lengths), 600, unroll_steps=K, td_steps=td, discount=discount, seed=5, prioritized=True)
    stream = torch.cuda.Stream(device=dev.device)
    with torch.cuda.stream(stream):
        dev.add_packed(block, lengths)
        batch, w = dev.sample_prioritized(n, step=0)
        where, _, ticket = dev.positions(np.array([2, 0], dtype=np.int64), np.array([599, 100], dtype=np.int64))
        dev.update(where, dev_t(dev, np.array([[3, 4], [5, 6]], dtype=np.int32)), dev_t(dev, np.array([7, 11], dtype=np.int32)),
                   dev_t(dev, np.array([900.5, -650.25])), ticket)
        ep2, pos2, filler2, prob2 = dev.prioritized_draws(n, step=1)
    stream.synchronize()
    from rlzero_amd.muzero import mz_prioritized_draws
    episodes = episodes_of(block, lengths, D, A)
    first = restated(episodes, td, discount)
    ep, pos, filler, prob = mz_prioritized_draws(5, 0, n, first, K, A)
    with torch.cuda.stream(stream):
        held = dev.read()
        second = dev.priorities()
    # the first batch was gathered BEFORE the write-back: from the episodes as they were added
    from rlzero_amd.muzero import ReplayBuffer
    host = ReplayBuffer(capacity=len(lengths), unroll_steps=K, td_steps=td, discount=discount)
    for e in episodes:
        host.add(e)
    assert_same_batch(on_host(batch), host_sample(host, (ep, pos, filler), A))
    np.testing.assert_allclose(w.cpu().numpy(), ((sum(lengths) * prob) ** -1.0).astype(np.float32), rtol=1e-6, atol=0)
    assert same_weights(second, restated(held, td, discount)) and not np.array_equal(second[2], first[2]) and not np.array_equal(second[0], first[0])
    want = mz_prioritized_draws(5, 1, n, second, K, A)
    for g, x in zip(on_host((ep2, pos2, filler2)), want[:3]):
        assert np.array_equal(g, x)
    assert same_bits(prob2.cpu().numpy(), want[3]) and dev.poll_errors() == 0
    dev.close()
