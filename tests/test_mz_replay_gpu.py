"""The MuZero device replay buffer (rlzero_amd/muzero/replay.py, csrc/rz_mz_replay.hip) on the GPU against the host buffer it
restates: the episodes held after adds that wrap the ring, every (episode, position) of ``gather`` against
``ReplayBuffer.sample`` for the same draws bit for bit, the device's draws against their host restatement, the kernel's index
checks, the hand-over of finished episodes from the whole-move launches' device arena, and the learner on device batches."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO
from test_mz_replay_host import (MAX_STEPS, assert_same_batch, episode_lengths, episodes_of, every_position, host_sample, packed_block,
                                 same_bits)

pytestmark = pytest.mark.gpu
D = 4
CAPACITY = 4


def held_equal(dev, host):
    """dev.read() is the host buffer's episode list, field by field, bit for bit."""
    got = dev.read()
    assert len(got) == len(host.episodes) == len(dev)
    assert np.array_equal(dev.lengths(), [len(ep) for ep in host.episodes])
    for g, w in zip(got, host.episodes):
        assert len(g) == len(w)
        assert same_bits(g.obs, np.asarray(w.obs, dtype=np.float32)) and np.array_equal(g.actions, w.actions)
        assert same_bits(g.rewards, np.asarray(w.rewards, dtype=np.float64)) and same_bits(g.root_values, np.asarray(w.root_values, dtype=np.float64))
        assert same_bits(g.policies, np.asarray(w.policies, dtype=np.float32))
    return True


def on_host(batch):
    return tuple(x.cpu().numpy() for x in batch)


def filled(K, td, discount, A, seed=3):
    """A device buffer and a host buffer of capacity 4 after the same seven episodes in three calls (the ring wraps and evicts);
    the three calls take the three ways in: a packed block, Episode objects (float32 policies) and an EpisodeSeq."""
    from rlzero_amd.muzero import MuZeroDeviceReplay, ReplayBuffer
    from rlzero_amd.muzero.selfplay import EpisodeSeq
    rng = np.random.RandomState(100 * K + A)
    lengths = episode_lengths(K, td) + [3]
    dev = MuZeroDeviceReplay(D, A, CAPACITY, MAX_STEPS, unroll_steps=K, td_steps=td, discount=discount, seed=seed)
    host = ReplayBuffer(capacity=CAPACITY, unroll_steps=K, td_steps=td, discount=discount, seed=seed)
    calls = []
    # call 1: three episodes as a packed block
    first = lengths[:3]
    block = packed_block(rng, first, D, A)
    assert dev.add_packed(block, first) == 3
    for ep in episodes_of(block, first, D, A):
        host.add(ep)
    calls.append(held_equal(dev, host))
    # call 2: two Episode objects with an empty one between them (skipped by both buffers)
    second = [lengths[3], 0, lengths[4]]
    eps = episodes_of(packed_block(rng, second, D, A), second, D, A)
    assert dev.add(eps) == 2
    for ep in eps:
        host.add(ep)
    calls.append(held_equal(dev, host))
    # call 3: an EpisodeSeq of packed records
    third = lengths[5:]
    seq = EpisodeSeq()
    seq._add_packed(packed_block(rng, third, D, A), D, A, third)
    assert dev.add(seq) == 2
    for ep in seq:
        host.add(ep)
    calls.append(held_equal(dev, host))
    assert len(dev) == CAPACITY and calls == [True] * 3
    return dev, host, rng


@pytest.mark.parametrize('A', [2, 3])
@pytest.mark.parametrize('K,td,discount', [(2, 3, 0.5), (5, 10, 0.997)])
def test_gather_equals_the_host_buffer(K, td, discount, A):
    import torch
    dev, host, rng = filled(K, td, discount, A)
    draws = every_position([len(ep) for ep in host.episodes], K, A, rng)
    want = host_sample(host, draws, A)
    got = dev.gather(*draws)
    assert all(x.is_cuda for x in got) and [x.dtype for x in got] == [torch.float32, torch.int64] + [torch.float32] * 4
    assert_same_batch(on_host(got), want)
    # the same draws from the device
    again = dev.gather(*(torch.from_numpy(x).to(dev.device) for x in draws))
    assert_same_batch(on_host(again), want)
    dev.close()


def test_sample_equals_its_restatement():
    from rlzero_amd.muzero import mz_replay_draws
    K, td, A = 5, 10, 3
    dev, host, _ = filled(K, td, 0.997, A, seed=17)
    lengths = dev.lengths()
    seen = []
    for step in range(3):
        draws = mz_replay_draws(17, step, 64, lengths, K, A)
        want = on_host(dev.gather(*draws))
        assert dev.step == step
        assert_same_batch(on_host(dev.sample(64)), want)       # the internal counter: update `step`
        assert dev.step == step + 1
        assert_same_batch(on_host(dev.sample(64, step)), want)  # the same update again, by number
        assert dev.step == step + 1
        seen.append(draws[0])
    assert not np.array_equal(seen[0], seen[1]) and len(set(np.concatenate(seen).tolist())) == CAPACITY
    dev.close()


def test_bad_indices_are_refused():
    import torch
    from rlzero_amd import _hip
    from rlzero_amd.muzero import MuZeroDeviceReplay
    K, td, A = 2, 3, 2
    dev, host, rng = filled(K, td, 0.5, A)
    lengths = dev.lengths()
    n = 8
    ep = np.arange(n, dtype=np.int64) % CAPACITY
    pos = np.zeros(n, dtype=np.int64)
    filler = np.ones((n, K), dtype=np.int64)
    good = on_host(dev.gather(ep, pos, filler))
    bad_rows = {1: ('ep', CAPACITY), 2: ('ep', -1), 4: ('pos', None), 5: ('pos', -1), 6: ('filler', A), 7: ('filler', -1)}
    for row, (what, v) in bad_rows.items():
        e, p, f = ep.copy(), pos.copy(), filler.copy()
        if what == 'ep':
            e[row] = v
        elif what == 'pos':
            p[row] = lengths[e[row]] if v is None else v
        else:
            f[row, K - 1] = v
        # host draws: refused before any launch
        with pytest.raises(_hip.HipError):
            dev.gather(e, p, f)
        # device draws: the flag, and the public call raises
        with pytest.raises(_hip.HipError):
            dev.gather(*(torch.from_numpy(x).to(dev.device) for x in (e, p, f)))
    # all of them in one launch through the C interface, into tensors holding a sentinel: the bad entries' rows are not written
    e, p, f = ep.copy(), pos.copy(), filler.copy()
    e[1], e[2], p[4], p[5], f[6, 0], f[7, K - 1] = CAPACITY, -1, lengths[e[4]], -1, A, -1
    draws = torch.from_numpy(np.concatenate((e[:, None], p[:, None], f), axis=1)).to(dev.device).contiguous()
    out = dev._outputs(n)
    for x in out:
        x.fill_(77)
    _hip.check(dev.lib.rz_mz_replay_gather(dev.handle, None, draws.data_ptr(), n, *[x.data_ptr() for x in out], dev._stream()), 'rz_mz_replay_gather')
    flags = ctypes.c_int32()
    _hip.check(dev.lib.rz_mz_replay_poll_errors(dev.handle, ctypes.byref(flags), dev._stream()), 'rz_mz_replay_poll_errors')
    assert flags.value == _hip.MZ_REPLAY_BAD_INDEX
    _hip.check(dev.lib.rz_mz_replay_poll_errors(dev.handle, ctypes.byref(flags), dev._stream()), 'rz_mz_replay_poll_errors')
    assert flags.value == 0   # cleared by the poll
    for x, g in zip(on_host(out), good):
        for row in range(n):
            if row in bad_rows:
                assert (x[row] == 77).all()
            else:
                assert same_bits(x[row], g[row])
    # an over-long episode: refused on the host, by the class and by the C interface, and nothing changes
    before = dev.lengths().copy()
    long_block = packed_block(rng, [MAX_STEPS + 1], D, A)
    with pytest.raises(ValueError):
        dev.add_packed(long_block, [MAX_STEPS + 1])
    with pytest.raises(ValueError):
        dev.add(episodes_of(long_block, [MAX_STEPS + 1], D, A))
    h_len = np.array([MAX_STEPS + 1], dtype=np.int32)
    rc = dev.lib.rz_mz_replay_add(dev.handle, 1, ctypes.c_void_p(h_len.ctypes.data), None, ctypes.c_void_p(long_block.ctypes.data), dev._stream())
    assert rc == -1   # RZ_ERR_ARG
    assert np.array_equal(dev.lengths(), before) and held_equal(dev, host)
    dev.close()
    # the limits: refused at creation
    for kw in (dict(obs_dim=17), dict(n_actions=9), dict(unroll_steps=17), dict(td_steps=65)):
        args = dict(obs_dim=4, n_actions=2, capacity_episodes=4, max_episode_steps=12, unroll_steps=5, td_steps=10)
        args.update(kw)
        with pytest.raises(_hip.HipError):
            MuZeroDeviceReplay(**args)


@pytest.fixture(scope='module')
def net():
    import torch
    from rlzero_amd.muzero import MuZeroNet
    torch.manual_seed(7)
    return MuZeroNet().to('cuda:0').eval()


def episode_bytes(eps):
    return [(len(e), np.asarray(e.obs).tobytes(), np.asarray(e.actions).tobytes(), np.asarray(e.rewards).tobytes(),
             np.asarray(e.policies).tobytes(), np.asarray(e.root_values).tobytes()) for e in eps]


@pytest.mark.parametrize('arena_rows', [None, 40])
def test_ingest_from_the_launch_arena(net, arena_rows):
    """Whole moves hand their finished episodes over on the device: the buffer then holds what a host buffer fed the returned
    EpisodeSeq holds (the ring of 64 episodes wraps on the way), through the arena (k_mzr_ingest) and -- with an arena too small
    -- through the ring's slow path (k_mzr_add); and self-play itself is not changed by the hand-over."""
    from rlzero_amd.muzero import CartPoleBatch, MuZeroDeviceReplay, MuZeroSelfPlay, ReplayBuffer

    class Counting(MuZeroDeviceReplay):
        calls = None

        def ingest(self, *a, **k):
            self.calls['ingest'] += 1
            return MuZeroDeviceReplay.ingest(self, *a, **k)

        def add_packed(self, *a, **k):
            self.calls['add_packed'] += 1
            return MuZeroDeviceReplay.add_packed(self, *a, **k)

    def play(replay):
        env = CartPoleBatch(64, 'cuda:0', seed=5)
        sp = MuZeroSelfPlay(net, env, n_sims=8, seed=2, moves_per_launch=4, arena_rows=arena_rows)
        assert sp.fused_moves
        eps = sp.collect(60) if replay is None else sp.collect(60, replay=replay)
        sp.close()
        return eps

    dev = Counting(4, 2, 64, 500, device='cuda:0')
    dev.calls = {'ingest': 0, 'add_packed': 0}
    eps = play(dev)
    assert len(eps) > 64   # (episodes of about 20 steps: the ring of 64 wrapped)
    host = ReplayBuffer(capacity=64)
    for ep in eps:
        host.add(ep)
    assert held_equal(dev, host)
    assert dev.calls['ingest'] > 0 and (dev.calls['add_packed'] > 0) == (arena_rows is not None)
    flags = ctypes.c_int32()
    assert dev.lib.rz_mz_replay_poll_errors(dev.handle, ctypes.byref(flags), dev._stream()) == 0 and flags.value == 0
    # a batch of the episodes handed over equals the host buffer's for the same draws
    rng = np.random.RandomState(1)
    ep_idx = rng.randint(64, size=64).astype(np.int64)
    pos = np.array([rng.randint(len(host.episodes[e])) for e in ep_idx], dtype=np.int64)
    filler = rng.randint(2, size=(64, 5)).astype(np.int64)
    assert_same_batch(on_host(dev.gather(ep_idx, pos, filler)), host_sample(host, (ep_idx, pos, filler), 2))
    dev.close()
    # (which episodes find room in a tight arena depends on the order in which the launch's workgroups claim its rows: the same
    # episodes, as tests/test_muzero.py compares them; with the default arena the order is the same too)
    again, first = episode_bytes(play(None)), episode_bytes(eps)
    assert again == first if arena_rows is None else sorted(again) == sorted(first)


def test_move_by_move_routes_hand_over_through_add(net):
    from rlzero_amd.muzero import CartPoleBatch, MuZeroDeviceReplay, MuZeroSelfPlay, ReplayBuffer
    sp = MuZeroSelfPlay(net, CartPoleBatch(64, 'cuda:0', seed=5), n_sims=8, seed=2, fused_moves=False)
    dev = MuZeroDeviceReplay(4, 2, 100, 500, device='cuda:0')
    eps = sp.collect(30, replay=dev)
    sp.close()
    assert len(eps) > 20
    host = ReplayBuffer(capacity=100)
    for ep in eps:
        host.add(ep)
    assert held_equal(dev, host)
    dev.close()


def test_the_learner_takes_device_batches():
    import torch
    from rlzero_amd.muzero import MuZeroAgent
    dev, host, _ = filled(5, 10, 0.997, 2)
    batch = dev.sample(32, 0)
    torch.manual_seed(3)
    a = MuZeroAgent(device='cuda:0')
    torch.manual_seed(3)
    b = MuZeroAgent(device='cuda:0')
    for p, q in zip(a.net.parameters(), b.net.parameters()):
        assert torch.equal(p, q)
    assert a.learn(batch) == b.learn(on_host(batch))
    dev.close()


def test_the_pipeline_runs_with_device_replay(capsys):
    spec = importlib.util.spec_from_file_location('train_muzero', os.path.join(REPO, 'tools', 'train_muzero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pipe = mod.MuZeroPipeline(n_envs=64, n_sims=8, batch_size=32, moves_per_iteration=30, updates_per_iteration=2, device_replay=True)
    pipe.run(2)
    out = capsys.readouterr().out
    assert out.count('batch i:') == 2 and len(pipe.buffer) >= 8 and pipe.buffer.step == 4
    pipe.selfplay.close()
    pipe.buffer.close()
