"""The MuZero device replay (rlzero_amd/muzero/replay.py, csrc/rz_mz_replay.hip) at the limits rz_mz_replay_create accepts and at
the trainer's shape, bit for bit against the host ``ReplayBuffer`` fed the same episodes and the numpy restatements.

The corners (tests/test_mz_replay_host.py: CORNERS, where the CPU tests hold the header to the same arbiter):

    MAX   D 16, A 8, K 16, td 64   every limit at once, slots of 80 steps (just above td + K), a ring of 5
    MIN   D 1, A 1, K 1, td 1      a slot of one step in a ring of one: every add evicts
    TALL  D 16, A 1, K 16, td 1    the widest rows of one kind with the narrowest of the other
    WIDE  D 1, A 8, K 1, td 64
    REAL  D 4, A 2, K 5, td 10     slots of 500 steps in a ring of 300 that 700 episodes wrap twice; the first call alone brings
                                   350 episodes, of which only the last 300 get a slot

Every kernel of the family runs at every corner: the store by its three ways in (k_mzr_add from a packed block and from Episode
objects with their final policy, k_mzr_ingest from a device arena with padding between the episodes), k_mzr_gather and
k_mzr_sample (also <true>, the value transform), k_mzr_positions and k_mzr_update, k_mzr_prio, k_mzr_scan and k_mzr_draw_prio.
On the small corners every (episode, position) held is an entry; on REAL every position of six episodes -- the oldest, the
newest, the shortest, the longest and the two on either side of the ring's seam -- so that the CPython arbiter stays in seconds.
No tolerance appears anywhere.  Each test prints how many entries it compared."""
import ctypes

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
from test_mz_prioritized_gpu import boundaries, draws_equal, restated, same_weights
from test_mz_reanalyse_gpu import dev_t, payload, stored_obs
from test_mz_reanalyse_host import patched
from test_mz_replay_gpu import held_equal, on_host
from test_mz_replay_host import CORNERS, assert_same_batch, boundary_kinds, corner, host_sample, kinds_that_exist, same_bits

pytestmark = pytest.mark.gpu
NAMES = sorted(CORNERS)
SEED = 5
SENTINEL = 77
N_DRAWN = 257   # a ragged last workgroup at every K + 1, D and A + 1


def arena_of(block, lengths):
    """The episodes of a packed block as a launch's arena holds them: two rows of padding in front of each and one behind the
    last (no first row is 0, no episode touches the next) -> (arena float64 [rows, D + 4 + A], first_rows)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    starts = np.cumsum(lengths) - lengths
    first_rows = starts + 2 * (np.arange(len(lengths)) + 1)
    arena = np.full((int(first_rows[-1] + lengths[-1]) + 1, block.shape[1]), 5.0)
    for a, m, src in zip(first_rows, lengths, starts):
        arena[a:a + m] = block[src:src + m]
    return arena, first_rows


def stored(name, check=False, **kw):
    """The corner and a device buffer after its three calls, one per way in; ``check``: held to the arbiter after every call."""
    import torch
    from rlzero_amd.muzero import MuZeroDeviceReplay
    c = corner(name)
    dev = MuZeroDeviceReplay(c.D, c.A, c.capacity, c.T, unroll_steps=c.K, td_steps=c.td, discount=c.discount, seed=SEED, **kw)
    for call, (lens, block, eps) in enumerate(c.calls):
        if call == 0:     # (on REAL: more episodes than the ring has slots)
            assert dev.add_packed(block, lens) == len(lens)
        elif call == 1:   # Episode objects: float32 policies in the visit columns, FINAL_POLICY
            assert dev.add(eps) == len(lens)
        else:
            arena, first_rows = arena_of(block, lens)
            assert first_rows.min() > 0 and dev.ingest(torch.from_numpy(arena).to(dev.device), lens, first_rows) == len(lens)
        if check:
            assert held_equal(dev, c.arbiter(call))
    assert len(dev) == c.capacity and dev.poll_errors() == 0
    return c, dev


_wanted = {}


def wanted(name, value_transform=False):
    """(the corner's entries, the arbiter's six arrays for them): formed once per corner and flag."""
    key = (name, value_transform)
    if key not in _wanted:
        c = corner(name)
        draws = c.entries(np.random.RandomState(7))
        _wanted[key] = (draws, host_sample(c.arbiter(value_transform=value_transform), draws, c.A))
    return _wanted[key]


def gather_both_ways(dev, draws, want):
    import torch
    got = dev.gather(*draws)
    assert all(x.is_cuda for x in got) and [x.dtype for x in got] == [torch.float32, torch.int64] + [torch.float32] * 4
    assert_same_batch(on_host(got), want)
    assert_same_batch(on_host(dev.gather(*(dev_t(dev, x) for x in draws))), want)   # the same draws from the device
    return on_host(got)


# ----------------------------------------------------------------------------------------------- 1. the store
@pytest.mark.parametrize('name', NAMES)
def test_the_store_holds_the_arbiters_episodes_after_every_call(name):
    c, dev = stored(name, check=True)
    assert dev._state() == (c.capacity, len(c.lengths) % c.capacity, c.capacity)
    assert len(c.lengths) >= 2 * c.capacity or name != 'REAL'           # REAL's ring wrapped twice
    assert len(c.calls[0][0]) > c.capacity or name != 'REAL'            # and one call alone overfilled it
    print('%s: %d episodes in calls of %r, %d held, %d steps held' % (name, len(c.lengths), [len(x[0]) for x in c.calls], len(dev),
                                                                       int(dev.lengths().sum())))
    dev.close()


# ----------------------------------------------------------------------------------------------- 2. mini-batches
@pytest.mark.parametrize('name', NAMES)
def test_gather_equals_the_host_buffer(name):
    c, dev = stored(name)
    draws, want = wanted(name)
    got = gather_both_ways(dev, draws, want)
    seen = boundary_kinds(c.arbiter(), draws, got, c.A)
    print('%s gather: %d entries, %d rows, boundary kinds %r' % (name, len(draws[0]), len(draws[0]) * (c.K + 1), seen))
    assert {kind: n > 0 for kind, n in seen.items()} == kinds_that_exist(c.K, c.td, c.T), seen
    dev.close()


@pytest.mark.parametrize('name', ['MAX', 'REAL'])
def test_gather_with_the_value_transform(name):
    c, dev = stored(name, prioritized=True, value_transform=True)
    draws, want = wanted(name, value_transform=True)
    gather_both_ways(dev, draws, want)
    assert not same_bits(want[2], wanted(name)[1][2])   # (the flag does change the value targets)
    _, plain = stored(name, prioritized=True)
    with_flag, without = dev.priorities(), plain.priorities()
    assert same_weights(with_flag, without)             # the priorities stay in raw units
    print('%s value transform: %d entries, %d priorities' % (name, len(draws[0]), sum(len(w) for w in with_flag)))
    dev.close(), plain.close()


@pytest.mark.parametrize('name', NAMES)
def test_sample_is_gather_of_its_draws(name):
    from rlzero_amd.muzero import mz_replay_draws
    c, dev = stored(name)
    lengths = dev.lengths()
    for step in (0, 1):
        draws = mz_replay_draws(SEED, step, N_DRAWN, lengths, c.K, c.A)
        assert_same_batch(on_host(dev.sample(N_DRAWN, step)), on_host(dev.gather(*draws)))
    assert dev.poll_errors() == 0
    print('%s sample: 2 x %d entries' % (name, N_DRAWN))
    dev.close()


# ----------------------------------------------------------------------------------------------- 3. nothing past the last row
def guarded(t, shape, dtype, device):
    return t.full(shape, SENTINEL, dtype=dtype, device=device)


@pytest.mark.parametrize('name', NAMES)
def test_no_launch_writes_past_its_last_row(name):
    """Through the C interface into outputs one entry longer than the call, filled with a sentinel: the n rows are the public
    call's, the extra row of every tensor still holds the sentinel."""
    import torch
    from rlzero_amd import _hip
    c, dev = stored(name, prioritized=True)
    draws, _ = wanted(name)
    n = len(draws[0])
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    # gather
    public = on_host(dev.gather(*draws))
    table = np.ascontiguousarray(np.concatenate((draws[0][:, None], draws[1][:, None], draws[2]), axis=1), dtype=np.int64)
    out = dev._outputs(n + 1)
    for x in out:
        x.fill_(SENTINEL)
    _hip.check(dev.lib.rz_mz_replay_gather(dev.handle, ptr(table), None, n, *[x.data_ptr() for x in out], dev._stream()), 'rz_mz_replay_gather')
    for x, g in zip(on_host(out), public):
        assert (x[n] == SENTINEL).all() and same_bits(x[:n], g)
    # positions: the caller's draws, then the device's own
    for own in (False, True):
        m = N_DRAWN if own else n
        keep = np.ascontiguousarray(np.stack(draws[:2], axis=1))
        pw, po, _ = dev.positions(n=m, step=2) if own else dev.positions(draws[0], draws[1])
        where, obs = guarded(torch, (m + 1, 2), torch.int32, dev.device), guarded(torch, (m + 1, c.D), torch.float32, dev.device)
        ticket = ctypes.c_int64(-1)
        _hip.check(dev.lib.rz_mz_replay_positions(dev.handle, None if own else ptr(keep), None, SEED, 2, m, where.data_ptr(), obs.data_ptr(),
                                                  ctypes.byref(ticket), dev._stream()), 'rz_mz_replay_positions')
        assert ticket.value == len(c.lengths)
        for x, g in zip(on_host((where, obs)), on_host((pw, po))):
            assert (x[m] == SENTINEL).all() and same_bits(x[:m], g)
    # prioritized draws: the stream's, then targets handed in
    weights = dev.priorities()
    total = sum(int(w.sum()) for w in weights)
    targets = dev_t(dev, np.arange(N_DRAWN, dtype=np.int64) * 7919 % total)
    for t in (None, targets):
        public = on_host(dev.prioritized_draws(N_DRAWN, step=4, targets=t))
        rows, prob = guarded(torch, (N_DRAWN + 1, c.K + 2), torch.int64, dev.device), guarded(torch, (N_DRAWN + 1, ), torch.float64, dev.device)
        _hip.check(dev.lib.rz_mz_replay_draw_prioritized(dev.handle, SEED, 4, N_DRAWN, None if t is None else t.data_ptr(), rows.data_ptr(),
                                                         prob.data_ptr(), dev._stream()), 'rz_mz_replay_draw_prioritized')
        rows, prob = on_host((rows, prob))
        assert (rows[N_DRAWN] == SENTINEL).all() and prob[N_DRAWN] == SENTINEL
        assert np.array_equal(rows[:N_DRAWN, 0], public[0]) and np.array_equal(rows[:N_DRAWN, 1], public[1])
        assert np.array_equal(rows[:N_DRAWN, 2:], public[2]) and same_bits(prob[:N_DRAWN], public[3])
    assert dev.poll_errors() == 0
    print('%s guard rows: gather %d, positions %d and %d, prioritized draws 2 x %d' % (name, n, n, N_DRAWN, N_DRAWN))
    dev.close()


# ----------------------------------------------------------------------------------------------- 4. Reanalyse without a search
def positions_equal(c, dev, host, got, ep_idx, pos):
    where, obs, ticket = got
    count, cursor, cap = dev._state()
    w = where.cpu().numpy()
    assert ticket == len(c.lengths) and w.dtype == np.int32
    assert np.array_equal(w[:, 0], ((cursor - count) % cap + ep_idx) % cap) and np.array_equal(w[:, 1], pos)   # the ring arithmetic
    assert same_bits(obs.cpu().numpy(), stored_obs(host, ep_idx, pos))


@pytest.mark.parametrize('name', NAMES)
def test_positions_and_update_without_a_search(name):
    from rlzero_amd import _hip
    from rlzero_amd.muzero import mz_reanalyse_draws
    c, dev = stored(name, prioritized=True)
    host = c.arbiter()
    rng = np.random.RandomState(31)
    ep_idx, pos = c.positions()
    n = len(ep_idx)
    # the device's own draws are the restatement's
    own = mz_reanalyse_draws(SEED, 3, N_DRAWN, dev.lengths())
    positions_equal(c, dev, host, dev.positions(n=N_DRAWN, step=3), *own)
    # every step (REAL: of the named episodes) from host draws and from device draws, then written back.  Among the payloads: an
    # unvisited root (the uniform policy) and a root N of 0, 1 and 40 -- in one call where there are four entries, else in turn
    updates = 0
    for turn, source in enumerate(('host', 'device') * (1 if n >= 4 else 2)):
        args = (ep_idx, pos) if source == 'host' else (dev_t(dev, ep_idx), dev_t(dev, pos))
        got = dev.positions(*args)
        assert dev.poll_errors() == 0
        positions_equal(c, dev, host, got, ep_idx, pos)
        visits, root_n, vsum = payload(rng, n, c.A)
        for which in (range(4) if n >= 4 else [turn]):
            i = which if n >= 4 else 0
            if which == 0:
                visits[i] = 0
            else:
                root_n[i] = (0, 1, 40)[which - 1]
        dev.update(got[0], dev_t(dev, visits), dev_t(dev, root_n), dev_t(dev, vsum), got[2])
        host = patched(host, ep_idx, pos, visits, root_n, vsum)
        assert held_equal(dev, host)   # the policy and the root value of the steps named, and nothing else of any step
        if n >= 4 or turn == 0:
            assert (host.episodes[ep_idx[0]].policies[pos[0]] == np.float32(1.0 / c.A)).all()
        updates += n
    # the priorities follow, and so do the n-step bootstraps of the mini-batches
    weights = dev.priorities()
    assert same_weights(weights, restated(host.episodes, c.td, c.discount))
    draws_equal(dev, weights, n=N_DRAWN, step=0)
    draws, _ = wanted(name)
    assert_same_batch(on_host(dev.gather(*draws)), host_sample(host, draws, c.A))
    # an episode stored between positions and update: the ticket is stale, update raises (twice) and writes nothing
    where, _, ticket = dev.positions(ep_idx[:1], pos[:1])
    lens, block, eps = c.calls[0]
    assert dev.add_packed(block[:lens[0]], lens[:1]) == 1
    host.add(eps[0])
    visits, root_n, vsum = payload(rng, 1, c.A)
    for _ in range(2):
        with pytest.raises(_hip.HipError):
            dev.update(where, dev_t(dev, visits), dev_t(dev, root_n), dev_t(dev, vsum), ticket)
    assert dev.positions(ep_idx[:1], pos[:1])[2] == ticket + 1 and held_equal(dev, host)
    print('%s reanalyse: %d own draws, %d steps resolved twice over, %d written back, %d priorities' % (
        name, N_DRAWN, n, updates, sum(len(w) for w in weights)))
    dev.close()


# ----------------------------------------------------------------------------------------------- 5. priorities
@pytest.mark.parametrize('name', NAMES)
def test_priorities_and_every_boundary(name):
    c, dev = stored(name, prioritized=True)
    host = c.arbiter()
    weights = dev.priorities()
    assert same_weights(weights, restated(host.episodes, c.td, c.discount))
    targets, total = boundaries(weights)
    which = range(len(weights))
    if name == 'REAL':   # the boundaries of the named episodes' steps, 0 and total - 1
        which = c.named()
        first = np.cumsum([len(w) for w in weights]) - [len(w) for w in weights]
        cum = np.cumsum(np.concatenate(weights))
        mine = np.concatenate([cum[first[j]:first[j] + len(weights[j])] for j in which])
        targets = np.unique(np.concatenate((mine - 1, mine, [0, total - 1])))
        targets = targets[(targets >= 0) & (targets < total)].astype(np.int64)
    ep, pos, _, prob = draws_equal(dev, weights, step=5, targets=targets)
    steps = {(e, t) for e in which for t in range(len(weights[e]))}
    assert steps <= set(zip(ep.tolist(), pos.tolist())) and len(targets) >= 2 * len(steps) - 2   # every step is reached
    assert same_bits(prob, np.array([float(weights[e][t]) / float(total) for e, t in zip(ep, pos)], dtype=np.float64))
    draws_equal(dev, weights, step=5, targets=dev_t(dev, targets))   # the same targets from the device
    for step in (0, 1):                                              # the stream's own draws
        draws_equal(dev, weights, n=N_DRAWN, step=step)
    assert dev.poll_errors() == 0
    print('%s priorities: %d weights, %d boundary targets twice over, 2 x %d stream draws' % (name, sum(len(w) for w in weights), len(targets),
                                                                                             N_DRAWN))
    dev.close()


# ----------------------------------------------------------------------------------------------- 6. to the fused learner
def test_the_fused_learner_takes_the_widest_batch():
    """D 16, A 8, K 16: an update on ``dev.sample(64, 0)`` and one on the arbiter's arrays for the same draws, uploaded, from equal
    parameters.  The learner's kernels are order-deterministic, so a difference is a stride or a dtype lost in the hand-over."""
    import torch
    from rlzero_amd.muzero import MuZeroAgent, mz_replay_draws
    c, dev = stored('MAX')
    made = []
    for _ in range(2):
        torch.manual_seed(3)
        made.append(MuZeroAgent(obs_dim=c.D, n_actions=c.A, device='cuda:0', fused_learner=True, unroll_steps=c.K, max_batch=64))
    a, b = made
    for p, q in zip(a.net.parameters(), b.net.parameters()):
        assert torch.equal(p, q)
    draws = mz_replay_draws(SEED, 0, 64, dev.lengths(), c.K, c.A)
    want = host_sample(c.arbiter(), draws, c.A)
    from_device = a.learn_async(dev.sample(64, 0))
    from_host = b.learn_async(tuple(dev_t(dev, x) for x in want))
    a.check(), b.check()
    assert same_bits(from_device.cpu().numpy(), from_host.cpu().numpy()) and np.isfinite(from_host.cpu().numpy()).all()
    for p, q in zip(a.net.parameters(), b.net.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(a.fused.exp_avg, b.fused.exp_avg) and not torch.equal(a.fused.exp_avg, torch.zeros_like(a.fused.exp_avg))
    a.fused.close(), b.fused.close(), dev.close()
