"""MuZero Reanalyse on the GPU (rlzero_amd/muzero/reanalyse.py; csrc/rz_mz_replay.hip: k_mzr_positions, k_mzr_update), bit for bit:
the two device ends alone against the host buffer with the same steps patched in numpy (tests/test_mz_reanalyse_host.py: patched),
their index and ticket checks, and whole refreshes against an INDEPENDENT route -- ``MuZeroSelfPlay.search(obs, add_noise=False)``
with a tree and a hidden buffer of its own, fed the very 16-row batches the reanalyser forms -- also after a learner step, and from
the trainer.  The buffers are those of tests/test_mz_replay_gpu.py: capacity 4 after seven episodes in three calls, so the ring has
wrapped and the oldest episode is not in slot 0."""
import os

import numpy as np
import pytest

from conftest import REPO
from test_mz_reanalyse_host import patched
from test_mz_replay_gpu import CAPACITY, D, filled, held_equal, on_host
from test_mz_replay_host import MAX_STEPS, assert_same_batch, episodes_of, every_position, host_sample, packed_block, same_bits

pytestmark = pytest.mark.gpu
N_SIMS, BATCH = 8, 16


def dev_t(dev, a, dtype=None):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dev.device)
    return x if dtype is None else x.to(dtype)


def stored_obs(host, ep_idx, pos):
    return np.stack([np.asarray(host.episodes[int(e)].obs[int(p)], dtype=np.float32) for e, p in zip(ep_idx, pos)])


def payload(rng, n, A):
    """Synthetic visit counts, root N and root value sums of n entries."""
    return (rng.randint(0, 51, size=(n, A)).astype(np.int32), rng.randint(0, 52, size=n).astype(np.int32), rng.standard_normal(n) * 9.3)


def write_back(dev, where, visits, root_n, vsum, ticket):
    dev.update(where, dev_t(dev, visits), dev_t(dev, root_n), dev_t(dev, vsum), ticket)


# ----------------------------------------------------------------------------------------------- 1. write-back alone
@pytest.mark.parametrize('A', [2, 3])
@pytest.mark.parametrize('K,td,discount', [(2, 3, 0.5), (5, 10, 0.997)])
def test_positions_and_update_without_a_search(K, td, discount, A):
    dev, host, rng = filled(K, td, discount, A)
    count, cursor, cap = dev._state()
    oldest = (cursor - count) % cap
    assert oldest != 0 and count == cap == CAPACITY
    lengths = [len(ep) for ep in host.episodes]
    draws = every_position(lengths, K, A, rng)
    dup = len(draws[0]) // 2
    ep_idx, pos = np.append(draws[0], draws[0][dup]), np.append(draws[1], draws[1][dup])   # every step held, one of them twice
    n = len(ep_idx)
    for source in ('host', 'device'):
        args = (ep_idx, pos) if source == 'host' else (dev_t(dev, ep_idx), dev_t(dev, pos))
        where, obs, ticket = dev.positions(*args)
        assert ticket == 7 and dev.poll_errors() == 0
        assert same_bits(obs.cpu().numpy(), stored_obs(host, ep_idx, pos))
        w = where.cpu().numpy()
        assert w.dtype == np.int32 and np.array_equal(w[:, 0], (oldest + ep_idx) % cap) and np.array_equal(w[:, 1], pos)
        visits, root_n, vsum = payload(rng, n, A)
        visits[3], root_n[5] = 0, 0                        # an unvisited root: the uniform policy; N = 0 divides by 1
        visits[-1], root_n[-1], vsum[-1] = visits[dup], root_n[dup], vsum[dup]   # the duplicate carries the same payload
        write_back(dev, where, visits, root_n, vsum, ticket)
        want = patched(host, ep_idx, pos, visits, root_n, vsum)
        assert held_equal(dev, want)
        assert (want.episodes[ep_idx[3]].policies[pos[3]] == np.float32(1.0 / A)).all()
        # the refreshed root values reach the n-step bootstraps of the mini-batches
        assert_same_batch(on_host(dev.gather(*draws)), host_sample(want, draws, A))
        host = want
    # a strict subset (the even positions): every other step keeps its bits
    before = dev.read()
    sel = draws[1] % 2 == 0
    ep_even, pos_even = draws[0][sel], draws[1][sel]
    where, _, ticket = dev.positions(ep_even, pos_even)
    visits, root_n, vsum = payload(rng, len(ep_even), A)
    write_back(dev, where, visits, root_n, vsum, ticket)
    touched = 0
    for was, now in zip(before, dev.read()):
        for t in range(len(was)):
            if t % 2:
                assert same_bits(was.policies[t], now.policies[t]) and same_bits(was.root_values[t:t + 1], now.root_values[t:t + 1])
            else:   # (a random payload: the step does not keep its root value by chance)
                assert not same_bits(was.root_values[t:t + 1], now.root_values[t:t + 1])
                touched += 1
    assert touched == len(ep_even) and 0 < touched < sum(lengths)
    assert held_equal(dev, patched(host, ep_even, pos_even, visits, root_n, vsum))
    dev.close()


# ----------------------------------------------------------------------------------------------- 2. checks
def test_bad_entries_stale_tickets_and_empty_calls():
    from rlzero_amd import _hip
    K, td, A = 2, 3, 2
    dev, host, rng = filled(K, td, 0.5, A)
    lengths = dev.lengths()
    n = 8
    ep, pos = np.arange(n, dtype=np.int64) % CAPACITY, np.zeros(n, dtype=np.int64)
    e, p = ep.copy(), pos.copy()
    e[1], e[2], p[4], p[6] = CAPACITY, -1, lengths[e[4]], -1   # episode == count, negative, position == length, negative
    bad = [1, 2, 4, 6]
    good = [i for i in range(n) if i not in bad]
    # device draws: flagged, (-1, -1), a zeroed row; the valid entries of the same call are resolved and written
    where, obs, ticket = dev.positions(dev_t(dev, e), dev_t(dev, p))
    assert dev.poll_errors() == _hip.MZ_REPLAY_BAD_INDEX and dev.poll_errors() == 0
    w, o = where.cpu().numpy(), obs.cpu().numpy()
    assert (w[bad] == -1).all() and (o[bad] == 0).all() and (w[good] >= 0).all()
    assert same_bits(o[good], stored_obs(host, ep[good], pos[good]))
    visits, root_n, vsum = payload(rng, n, A)
    for i in good:   # (entries of one step carry one payload)
        first = good[[int(ep[g]) for g in good].index(int(ep[i]))]
        visits[i], root_n[i], vsum[i] = visits[first], root_n[first], vsum[first]
    write_back(dev, where, visits, root_n, vsum, ticket)
    host = patched(host, ep[good], pos[good], visits[good], root_n[good], vsum[good])
    assert held_equal(dev, host)
    # host draws: refused before any launch
    for i in bad:
        e1, p1 = ep.copy(), pos.copy()
        e1[i], p1[i] = e[i], p[i]
        with pytest.raises(_hip.HipError):
            dev.positions(e1, p1)
    assert dev.poll_errors() == 0 and held_equal(dev, host)
    # an add between positions and update: update raises, and the store holds what it held plus the added episode
    where, _, ticket = dev.positions(ep[good], pos[good])
    block = packed_block(rng, [2], D, A)
    assert dev.add_packed(block, [2]) == 1
    host.add(episodes_of(block, [2], D, A)[0])
    with pytest.raises(_hip.HipError):
        write_back(dev, where, visits[good], root_n[good], vsum[good], ticket)
    assert held_equal(dev, host)
    where, _, again = dev.positions(ep[good], pos[good])
    assert again == ticket + 1
    visits, root_n, vsum = payload(rng, 1, A)
    write_back(dev, where[:1].contiguous(), visits, root_n, vsum, again)
    host = patched(host, ep[good][:1], pos[good][:1], visits, root_n, vsum)
    assert held_equal(dev, host)
    # n = 0: nothing happens
    for args in (dict(ep_idx=np.zeros(0, dtype=np.int64), pos=np.zeros(0, dtype=np.int64)), dict(n=0)):
        where, obs, ticket = dev.positions(**args)
        assert tuple(where.shape) == (0, 2) and tuple(obs.shape) == (0, D) and ticket == again
        write_back(dev, where, np.zeros((0, A), dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), ticket)
    assert dev.poll_errors() == 0 and held_equal(dev, host)
    dev.close()


# ----------------------------------------------------------------------------------------------- 3. whole refreshes
class Route(object):
    """The independent route: MuZeroSelfPlay.search on 16 rows, with its own tree and hidden buffer."""

    def __init__(self, net, fused):
        from rlzero_amd.muzero import CartPoleBatch, MuZeroSelfPlay
        # (use_graph=False: the step loop's launches go out one by one instead of as a replayed hipGraph -- the same kernels on the
        # same inputs -- and the object takes no side stream from torch's pool: tests/test_trace.py, later in the suite, measures
        # how four lane streams overlap, and that depends on which pool streams earlier tests have bound to hardware queues)
        self.sp = MuZeroSelfPlay(net, CartPoleBatch(BATCH, 'cuda:0', seed=1), n_sims=N_SIMS, fused=fused, fused_moves=False, use_graph=False)
        assert self.sp.fused == fused and not self.sp.fused_moves

    def __call__(self, host, ep_idx, pos):
        """(visits int32 [n, A], N int32 [n], value sum float64 [n]) of the steps, searched in the reanalyser's batches: chunks of
        16 rows, a short last chunk padded with its first observation."""
        import torch
        obs = stored_obs(host, ep_idx, pos)
        out = ([], [], [])
        for a in range(0, len(obs), BATCH):
            rows = obs[a:a + BATCH]
            m = len(rows)
            rows = np.concatenate((rows, np.repeat(rows[:1], BATCH - m, axis=0)))
            visits, root_value = self.sp.search(torch.from_numpy(rows).to('cuda:0'), add_noise=False)
            root_n, root_sum, _, _ = self.sp.tree.root_stats()
            assert torch.equal(root_value, root_sum / root_n.clamp_min(1).to(torch.float64))
            for dst, x in zip(out, (visits, root_n, root_sum)):
                dst.append(x.cpu().numpy()[:m].copy())
        return tuple(np.concatenate(x) for x in out)

    def close(self):
        self.sp.close()


def make_net():
    import torch
    from rlzero_amd.muzero import MuZeroNet
    torch.manual_seed(7)
    return MuZeroNet(obs_dim=D, n_actions=2, hidden=64).to('cuda:0').eval()


@pytest.mark.parametrize('fused', [True, False])
def test_whole_refresh_equals_the_independent_route(fused):
    from rlzero_amd import _hip
    from rlzero_amd.muzero import MuZeroReanalyser, mz_reanalyse_draws
    A = 2
    net = make_net()
    dev, host, rng = filled(5, 10, 0.997, A)
    original = dev.read()
    route = Route(net, fused)
    rean = MuZeroReanalyser(net, dev, n_sims=N_SIMS, batch=BATCH, fused=fused, seed=21)
    assert rean.fused == fused
    lengths = [len(ep) for ep in host.episodes]
    every = every_position(lengths, 5, A, rng)[:2]
    order = rng.permutation(len(every[0]))
    # exactly one chunk
    ep_idx, pos = every[0][order[:BATCH]], every[1][order[:BATCH]]
    assert rean.reanalyse(ep_idx, pos) == BATCH
    host = patched(host, ep_idx, pos, *route(host, ep_idx, pos))
    assert held_equal(dev, host)
    # a full chunk and a padded one, one step named in both; the draws are device tensors
    ep_idx, pos = every[0][order[BATCH - 2:2 * BATCH]], every[1][order[BATCH - 2:2 * BATCH]]
    ep_idx, pos = np.append(ep_idx, ep_idx[2]), np.append(pos, pos[2])
    assert len(ep_idx) == 19
    assert rean.reanalyse(dev_t(dev, ep_idx), dev_t(dev, pos)) == 19
    visits, root_n, vsum = route(host, ep_idx, pos)
    assert np.array_equal(visits[2], visits[18]) and root_n[2] == root_n[18] and same_bits(vsum[2:3], vsum[18:19])
    assert visits.sum(axis=1).tolist() == [N_SIMS] * 19
    host = patched(host, ep_idx, pos, visits, root_n, vsum)
    assert held_equal(dev, host)
    # draws made on the device: exactly the positions of the restatement
    for step in (3, None):
        ep_idx, pos = mz_reanalyse_draws(21, 3 if step == 3 else 0, BATCH, dev.lengths())
        assert rean.reanalyse_sample(BATCH, step) == BATCH
        host = patched(host, ep_idx, pos, *route(host, ep_idx, pos))
        assert held_equal(dev, host)
    assert rean.step == 1
    # a device draw out of range: raised, nothing refreshed
    with pytest.raises(_hip.HipError):
        rean.reanalyse(dev_t(dev, np.array([0, CAPACITY])), dev_t(dev, np.array([0, 0])))
    with pytest.raises(_hip.HipError):
        rean.reanalyse(np.array([0]), np.array([MAX_STEPS]))
    assert held_equal(dev, host)
    # every step held: none keeps the root value it was stored with
    assert rean.reanalyse_all() == sum(lengths)
    host = patched(host, every[0], every[1], *route(host, *every))
    assert held_equal(dev, host)
    for was, now in zip(original, dev.read()):
        assert not (was.root_values == now.root_values).any() and not same_bits(was.policies, now.policies)
        assert same_bits(was.obs, now.obs) and np.array_equal(was.actions, now.actions) and same_bits(was.rewards, now.rewards)
    assert rean.positions_done == BATCH * 3 + 19 + sum(lengths)
    rean.close(), route.close(), dev.close()


# ----------------------------------------------------------------------------------------------- 4. weights follow the learner
@pytest.mark.parametrize('fused', [True, False])
def test_refreshes_follow_the_learner(fused):
    import torch
    from rlzero_amd.muzero import MuZeroAgent, MuZeroReanalyser
    A = 2
    torch.manual_seed(11)
    agent = MuZeroAgent(obs_dim=D, n_actions=A, device='cuda:0')
    agent.net.eval()
    dev, host, rng = filled(5, 10, 0.997, A)
    route = Route(agent.net, fused)
    rean = MuZeroReanalyser(agent.net, dev, n_sims=N_SIMS, batch=BATCH, fused=fused)
    every = every_position([len(ep) for ep in host.episodes], 5, A, rng)
    ep_idx, pos = every[0][:BATCH], every[1][:BATCH]
    rean.reanalyse(ep_idx, pos)
    first = route(host, ep_idx, pos)
    host = patched(host, ep_idx, pos, *first)
    assert held_equal(dev, host)
    agent.learn(dev.sample(32, 0))
    rean.reanalyse(ep_idx, pos)                               # (before the route searches: the reanalyser uploads for itself)
    second = route(host, ep_idx, pos)
    assert not same_bits(first[2], second[2])               # the step moved the values: stale weights would show
    host = patched(host, ep_idx, pos, *second)
    assert held_equal(dev, host)
    rean.close(), route.close(), dev.close()


# ----------------------------------------------------------------------------------------------- 5. the trainer
def test_the_trainer_runs_with_reanalyse():
    """tools/train_muzero.py --device-replay --reanalyse 32 | all, two iterations at a tiny geometry, as the command-line tool (two
    processes side by side): both iterations print their line, and it names the steps refreshed before the iteration's updates."""
    import re
    import subprocess
    import sys
    base = [sys.executable, os.path.join(REPO, 'tools', 'train_muzero.py'), '--device-replay', '--envs', '64', '--sims', '8', '--iterations', '2',
            '--batch-size', '32', '--updates-per-iteration', '2', '--reanalyse']
    runs = {v: subprocess.Popen(base + [v], stdout=subprocess.PIPE, stderr=subprocess.PIPE) for v in ('32', 'all')}
    for v, proc in runs.items():
        out, err = proc.communicate()
        assert proc.returncode == 0, err.decode()[-2000:]
        lines = [ln for ln in out.decode().splitlines() if ln.startswith('batch i:')]
        refreshed = [int(re.search(r'reanalysed:(\d+)$', ln).group(1)) for ln in lines]
        assert len(lines) == 2, out.decode()
        if v == '32':
            assert refreshed == [32, 32]
        else:   # every step held: at least the 8 episodes the first update waits for, and more after 20 more moves of 64 environments
            assert refreshed[0] >= 8 and refreshed[1] > refreshed[0]
