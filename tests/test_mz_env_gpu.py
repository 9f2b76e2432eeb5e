"""MuZero's moves kept on the device for any environment the library knows (rz_mz_env_step, rz_mz_env_move, rz_mz_root_noise;
MuZeroSelfPlay(device_moves=...)) and the second environment, Acrobot-v1, on the GPU.

G = 40 environments everywhere: not a multiple of a wave, of the search's 16 games per workgroup, or of four.  The yardsticks:
* the environment: the scalar twin tests/acrobot_twin.py (which tests/test_mz_env_host.py holds equal to the header bit for bit),
  set to the device's own float64 state before every step; state and observation within 1e-9 -- the bound
  test_cartpole_batch_vs_scalar_restatement allows over 120 unsynchronised steps; one step's rounding (another library's sin and
  cos, about 1e-16 each, through a step whose derivatives reach a few hundred) is about 1e-13.  An environment whose twin comes
  within 1e-9 of a decision (pre-wrap angle against +-pi, height against 1, velocity against its bound) is left out and counted:
  none is, asserted; CartPole, which rz_cartpole_step and rz_mz_env_step serve with one kernel, follows oracle/muzero_ref.RefCartPole
  (tests/cartpole_twin.py) under the same bound and the same rule;
* the move: tests/device_streams.py (action draw, root noise, under the tolerance rules of tests/test_noise_streams_gpu.py);
* the route: the host-driven loop (``device_moves=False``) searching from the same torch initial inference with the same kernel:
  the same episodes in the same order, bit for bit."""
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import acrobot_twin as twin
import cartpole_twin as cart
import device_streams as ds
from test_mz_replay_host import every_position, same_bits

pytestmark = pytest.mark.gpu

G = 40
BOUND = 1e-9
DEV = 'cuda:0'
D, A = 6, 3
ROW = D + 4 + A


# ------------------------------------------------------------------------------------------------ the environment against the twin
def check_step(before, steps_before, episode_before, actions, got, seed, max_steps):
    """One device step of every environment against the twin set to the device's state -> counts of what was seen."""
    from rlzero_amd.muzero import acrobot_initial_states
    state, steps, episode, obs, reward, term, trunc = got
    seen = dict(left_out=0, terminated=0, truncated=0, wrapped=0, clamped=0, reset=0)
    for i in range(len(before)):
        s, a = tuple(before[i]), int(actions[i])
        if twin.decision_margin(s, a) < BOUND:
            seen['left_out'] += 1
            continue
        raw = twin.integrate(s, a)
        new, new_steps, r, t1, t2 = twin.step(s, int(steps_before[i]), a, max_steps)
        assert (bool(term[i]), bool(trunc[i]), float(reward[i])) == (t1, t2, r), (i, s, a)
        seen['terminated'] += t1
        seen['truncated'] += t2
        seen['wrapped'] += abs(raw[0]) > twin.PI or abs(raw[1]) > twin.PI
        seen['clamped'] += abs(raw[2]) > twin.MAX_VEL_1 or abs(raw[3]) > twin.MAX_VEL_2
        if t1 or t2:   # the state is the next episode's first, exactly
            seen['reset'] += 1
            want = acrobot_initial_states(seed, i, episode_before[i] + 1)[0]
            assert same_bits(state[i], want) and steps[i] == 0 and episode[i] == episode_before[i] + 1
            new = tuple(want)
        else:
            assert np.abs(state[i] - np.array(new)).max() <= BOUND, (i, s, a, state[i], new)
            assert steps[i] == new_steps and episode[i] == episode_before[i]
        assert obs.dtype == np.float32 and np.abs(obs[i].astype(np.float64) - twin.observe(state[i]).astype(np.float64)).max() <= BOUND
        assert np.abs(obs[i].astype(np.float64) - twin.observe(new).astype(np.float64)).max() <= 1e-7   # (float32 of values 1e-9 apart)
    return seen


def device_step(env, actions):
    import torch
    obs, reward, term, trunc = env.step(torch.from_numpy(actions).to(DEV))
    return (env.state.cpu().numpy(), env.steps.cpu().numpy(), env.episode, obs.cpu().numpy(), reward.cpu().numpy(), term.cpu().numpy(),
            trunc.cpu().numpy())


def test_acrobot_batch_against_the_twin_one_step_at_a_time():
    from rlzero_amd.muzero import AcrobotBatch, acrobot_initial_states
    seed = 3
    env = AcrobotBatch(G, DEV, seed=seed)
    assert env.state.dtype.is_floating_point and tuple(env.state.shape) == (G, 4) and env.max_episode_steps == 500
    assert same_bits(env.state.cpu().numpy(), acrobot_initial_states(seed, np.arange(G), np.zeros(G)))
    assert np.abs(env.observe().cpu().numpy().astype(np.float64) - np.stack([twin.observe(s) for s in env.state.cpu().numpy()])).max() <= BOUND
    rng = np.random.RandomState(1)
    total = dict()
    for _ in range(60):
        actions = rng.randint(0, 3, size=G).astype(np.int64)
        before, steps_before, episode_before = env.state.cpu().numpy(), env.steps.cpu().numpy(), env.episode
        seen = check_step(before, steps_before, episode_before, actions, device_step(env, actions), seed, 500)
        for k, v in seen.items():
            total[k] = total.get(k, 0) + int(v)
    print('60 random steps of %d environments: %s' % (G, total))
    assert total['left_out'] == 0

    # the crafted states of the host test, time limit 12, half of them one step before it
    env = AcrobotBatch(G, DEV, seed=seed, max_episode_steps=12)
    cases = twin.crafted_states()
    states = np.array([cases[i % len(cases)][1] for i in range(G)], dtype=np.float64)
    actions = np.array([cases[i % len(cases)][2] for i in range(G)], dtype=np.int64)
    env.set_states(states)
    env.steps[G // 2:] = 11
    env.episode_dev[::3] += 5
    before, steps_before, episode_before = env.state.cpu().numpy(), env.steps.cpu().numpy(), env.episode
    assert same_bits(before, states)
    seen = check_step(before, steps_before, episode_before, actions, device_step(env, actions), seed, 12)
    print('crafted states: %s' % seen)
    assert seen['left_out'] == 0 and all(seen[k] >= 1 for k in ('terminated', 'truncated', 'wrapped', 'clamped', 'reset'))
    assert seen['truncated'] == G - G // 2 and seen['reset'] < G


def check_cartpole_step(before, steps_before, episode_before, actions, got, seed, max_steps):
    """One device step of every CartPole environment against RefCartPole set to the device's state -> counts of what was seen."""
    from rlzero_amd.muzero.cartpole import initial_states
    state, steps, episode, obs, reward, term, trunc = got
    seen = dict(left_out=0, terminated=0, truncated=0, both=0, reset=0)
    for i in range(len(before)):
        s, a = tuple(before[i]), int(actions[i])
        if cart.decision_margin(s, a) < BOUND:
            seen['left_out'] += 1
            continue
        new, new_steps, r, t1, t2 = cart.step(s, int(steps_before[i]), a, max_steps)
        assert (bool(term[i]), bool(trunc[i]), float(reward[i])) == (t1, t2, r), (i, s, a)
        seen['terminated'] += t1
        seen['truncated'] += t2
        seen['both'] += t1 and t2
        if t1 or t2:   # the state is the next episode's first, exactly
            seen['reset'] += 1
            want = initial_states(seed, [i], [episode_before[i] + 1])[0]
            assert same_bits(state[i], want) and steps[i] == 0 and episode[i] == episode_before[i] + 1
        else:
            assert np.abs(state[i] - np.array(new)).max() <= BOUND, (i, s, a, state[i], new)
            assert steps[i] == new_steps and episode[i] == episode_before[i]
        assert obs.dtype == np.float32 and same_bits(obs[i], state[i].astype(np.float32))
    return seen


def env_step_cartpole(env, actions, max_steps):
    """rz_mz_env_step(RZ_MZ_ENV_CARTPOLE) on a CartPoleBatch's tensors -> what ``device_step`` returns."""
    import ctypes
    import torch
    from rlzero_amd import _hip
    from rlzero_amd.engine import _ptr, check
    act = torch.from_numpy(actions).to(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
    check(env.lib.rz_mz_env_step(_hip.MZ_ENV_CARTPOLE, _ptr(env.state), _ptr(env.steps), _ptr(env.episode_dev), _ptr(act), G, env.seed, max_steps,
                                 _ptr(env._obs), _ptr(env._reward), _ptr(env._terminated), _ptr(env._truncated), stream), 'rz_mz_env_step')
    return (env.state.cpu().numpy(), env.steps.cpu().numpy(), env.episode, env._obs.cpu().numpy(), env._reward.cpu().numpy(),
            env._terminated.cpu().numpy().astype(bool), env._truncated.cpu().numpy().astype(bool))


def test_env_step_serves_cartpole_too():
    """rz_mz_env_step(RZ_MZ_ENV_CARTPOLE, ..., 500) and rz_cartpole_step are one kernel: over 30 steps of 40 environments each follows
    RefCartPole from the state before within 1e-9 with equal flags and step counts, a reset carries the bits of ``initial_states``, and
    the two give the same bits.  Then the crafted states of the host test through rz_mz_env_step with a limit of 12, half of the
    environments at step 11."""
    from rlzero_amd.muzero import CartPoleBatch
    from rlzero_amd.muzero.cartpole import initial_states
    seed = 2
    a, b = CartPoleBatch(G, DEV, seed=seed), CartPoleBatch(G, DEV, seed=seed)
    assert same_bits(b.state.cpu().numpy(), initial_states(seed, np.arange(G), np.zeros(G, dtype=np.int64)))
    rng = np.random.RandomState(3)
    total = dict()
    for _ in range(30):
        actions = rng.randint(0, 2, size=G).astype(np.int64)
        before, steps_before, episode_before = b.state.cpu().numpy(), b.steps.cpu().numpy(), b.episode
        got_a, got_b = device_step(a, actions), env_step_cartpole(b, actions, 500)
        for got in (got_a, got_b):
            seen = check_cartpole_step(before, steps_before, episode_before, actions, got, seed, 500)
        for x, y in zip(got_a, got_b):   # (state, steps, episode, obs, reward and the two flags)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        for k, v in seen.items():
            total[k] = total.get(k, 0) + int(v)
    print('30 random steps of %d environments: %s' % (G, total))
    assert total['left_out'] == 0 and total['terminated'] > 0 and total['reset'] == total['terminated']

    cases = cart.crafted_states()
    states = np.array([cases[i % len(cases)][1] for i in range(G)], dtype=np.float64)
    actions = np.array([cases[i % len(cases)][2] for i in range(G)], dtype=np.int64)
    b.set_states(states)
    b.steps[G // 2:] = 11
    b.episode_dev[::3] += 5
    before, steps_before, episode_before = b.state.cpu().numpy(), b.steps.cpu().numpy(), b.episode
    assert same_bits(before, states)
    seen = check_cartpole_step(before, steps_before, episode_before, actions, env_step_cartpole(b, actions, 12), seed, 12)
    print('crafted states: %s' % seen)
    ends = sum(bool(cases[i % len(cases)][3]) for i in range(G))
    assert seen['left_out'] == 0 and seen['terminated'] == ends and seen['truncated'] == G - G // 2
    assert 1 <= seen['both'] < seen['truncated'] and seen['reset'] < G   # (truncated only, terminated only, both and neither are all met)


# ------------------------------------------------------------------------------------------------ env_move alone
def make_net(obs_dim=D, n_actions=A, seed=6):
    import torch
    from rlzero_amd.muzero import MuZeroNet
    torch.manual_seed(seed)
    return MuZeroNet(obs_dim, n_actions).to(DEV).eval()


class Searched(object):
    """40 Acrobot environments a few steps into episodes of different numbers, and one 8-simulation search of them, noise off."""

    def __init__(self, max_steps, warm_steps):
        import torch
        from rlzero_amd.muzero import AcrobotBatch, MuZeroTree
        self.seed, self.noise_seed, self.t = 5, 17, 7
        self.env = env = AcrobotBatch(G, DEV, seed=self.seed, max_episode_steps=max_steps)
        rng = np.random.RandomState(8)
        for _ in range(warm_steps):
            env.step(torch.from_numpy(rng.randint(0, 3, size=G).astype(np.int64)).to(DEV))
        env.episode_dev += torch.arange(G, device=DEV) % 3
        net = make_net()
        self.tree = tree = MuZeroTree(G, A, 8, device=DEV)
        tree.load_model(net)
        hidden = torch.zeros((G, tree.slots_per_game, net.hidden), dtype=torch.float32, device=DEV)
        with torch.no_grad():
            s0, logits, _ = net.initial_inference(env.observe())
            hidden[:, 0] = s0
            tree.init_roots(torch.softmax(logits, dim=1).contiguous(), None, 0.0)
            tree.search_fused(hidden, 8)
        self.visits = tree.root_visits().cpu().numpy().copy()
        n, vsum, _, _ = tree.root_stats()
        self.root_n, self.root_sum = n.cpu().numpy().copy(), vsum.cpu().numpy().copy()
        assert (self.visits.sum(axis=1) == 8).all() and (self.root_n == 8).all()
        self.saved = (env.state.clone(), env.steps.clone(), env.episode_dev.clone())

    def move(self, temperature, hist=16, arena_rows=64):
        """Put the environments back, one env_move at step ``t`` with fresh history -> everything it wrote, as numpy."""
        import torch
        env = self.env
        for dst, src in zip((env.state, env.steps, env.episode_dev), self.saved):
            dst.copy_(src)
        kw = dict(device=DEV)
        ring = torch.full((G, hist, ROW), -7.0, dtype=torch.float64, **kw)
        ep_start = torch.from_numpy(self.t - self.saved[1].cpu().numpy()).to(DEV)
        arena = torch.full((arena_rows, ROW), -7.0, dtype=torch.float64, **kw)
        counters, entries = torch.zeros(4, dtype=torch.int64, **kw), torch.full((G, 4), -7, dtype=torch.int64, **kw)
        obs = torch.full((G, D), -7.0, dtype=torch.float32, **kw)
        self.tree.env_move(env, self.noise_seed, temperature, (ring, ep_start), self.t, arena, counters, entries, obs)
        torch.cuda.synchronize()
        return dict(ring=ring.cpu().numpy(), ep_start=ep_start.cpu().numpy(), arena=arena.cpu().numpy(), counters=counters.cpu().numpy(),
                    entries=entries.cpu().numpy(), obs=obs.cpu().numpy(), state=env.state.cpu().numpy(), steps=env.steps.cpu().numpy(),
                    episode=env.episode)


@pytest.fixture(scope='module')
def searched():
    s = Searched(max_steps=12, warm_steps=3)
    yield s
    s.tree.close()


@pytest.mark.parametrize('temperature', [1.0, 0.0, 0.5])
def test_env_move_writes_every_word_of_the_record(searched, temperature):
    from rlzero_amd.muzero import acrobot_initial_states
    s = searched
    before, steps_before, episode_before = (x.cpu().numpy() for x in s.saved)
    assert (steps_before == 3).all() and len(set(episode_before)) == 3
    out = s.move(temperature)
    hist = out['ring'].shape[1]
    rec = out['ring'][:, s.t % hist]
    assert (np.delete(out['ring'], s.t % hist, axis=1) == -7.0).all()   # one record per environment, nothing else
    inv_t = 1.0 / temperature if temperature > 0 else 0.0
    want_action, gap = ds.muzero_action(s.noise_seed, np.arange(G), episode_before, steps_before, s.visits, inv_t)
    keep = ~((gap < 1e-9) & (inv_t != 1.0))   # (the rule of test_whole_move_action_draws_are_the_restatement)
    assert keep.sum() > G // 2 and np.array_equal(rec[keep, D].astype(np.int64), want_action[keep])
    if temperature > 0:
        assert len(set(rec[:, D])) > 1 and (rec[:, D] != np.argmax(s.visits, axis=1)).any()   # (a draw, not the arg-max)
    assert same_bits(rec[:, D + 2:D + 2 + A], s.visits.astype(np.float64))
    assert same_bits(rec[:, D + 2 + A], s.root_sum / np.maximum(s.root_n, 1).astype(np.float64))
    n_done = 0
    for g in range(G):
        st, a = tuple(before[g]), int(rec[g, D])
        assert twin.decision_margin(st, a) >= BOUND
        assert np.abs(rec[g, :D] - twin.observe(st).astype(np.float64)).max() <= BOUND and same_bits(rec[g, :D], rec[g, :D].astype(np.float32).astype(np.float64))
        new, new_steps, r, t1, t2 = twin.step(st, int(steps_before[g]), a, 12)
        assert rec[g, D + 1] == r and rec[g, D + 3 + A] == float(t1 or t2)
        if t1 or t2:
            n_done += 1
            new, new_steps = tuple(acrobot_initial_states(s.seed, g, episode_before[g] + 1)[0]), 0
            assert same_bits(out['state'][g], np.array(new)) and out['episode'][g] == episode_before[g] + 1 and out['ep_start'][g] == s.t + 1
        else:
            assert np.abs(out['state'][g] - np.array(new)).max() <= BOUND and out['episode'][g] == episode_before[g] and out['ep_start'][g] == s.t - 3
        assert out['steps'][g] == new_steps
        assert np.abs(out['obs'][g].astype(np.float64) - twin.observe(out['state'][g]).astype(np.float64)).max() <= BOUND
    assert tuple(out['counters'][:3]) == (4 * n_done, n_done, 0)   # (an episode that ended here is 4 steps long)


def test_env_move_hands_over_finished_episodes():
    """max_episode_steps = 1: every environment ends with this move -- runs, entries, counters, ep_start, the next episode; then an
    arena of 25 rows for the 40 one-step episodes: 15 entries carry row -1 and are counted."""
    from rlzero_amd.muzero import acrobot_initial_states
    s = Searched(max_steps=1, warm_steps=0)
    episode_before = s.saved[2].cpu().numpy()
    for arena_rows, fit in ((64, G), (25, 25)):
        out = s.move(0.0, hist=4, arena_rows=arena_rows)
        rec = out['ring'][:, s.t % 4]
        assert (rec[:, D + 3 + A] == 1.0).all() and (rec[:, D + 1] == -1.0).all()
        assert tuple(out['counters'][:3]) == (G, G, G - fit)
        ent = out['entries'][np.argsort(out['entries'][:, 0])]
        assert np.array_equal(ent[:, 0], np.arange(G)) and (ent[:, 1] == s.t + 1).all() and (ent[:, 2] == 1).all()
        rows = ent[:, 3]
        assert sorted(rows[rows >= 0]) == list(range(fit)) and (rows[rows < 0] == -1).all()
        for g in np.nonzero(rows >= 0)[0]:
            assert same_bits(out['arena'][rows[g]], rec[g])
        assert (out['arena'][fit:] == -7.0).all()
        assert (out['ep_start'] == s.t + 1).all() and np.array_equal(out['episode'], episode_before + 1) and not out['steps'].any()
        assert same_bits(out['state'], acrobot_initial_states(s.seed, np.arange(G), episode_before + 1))
    s.tree.close()


def test_env_move_refuses_what_it_cannot_serve(searched):
    import torch
    from rlzero_amd._hip import HipError
    from rlzero_amd.muzero import CartPoleBatch
    s = searched
    with pytest.raises(HipError, match='ring_steps'):
        s.move(0.0, hist=8)   # shorter than an episode of 12
    kw = dict(device=DEV)
    ring, ep_start = torch.zeros((G, 512, 4 + 4 + A), dtype=torch.float64, **kw), torch.zeros(G, dtype=torch.int64, **kw)
    with pytest.raises(ValueError, match='shape'):   # a two-action environment behind a three-action tree
        s.tree.env_move(CartPoleBatch(G, DEV), 0, 0.0, (ring, ep_start), 0, torch.zeros((8, 11), dtype=torch.float64, **kw),
                        torch.zeros(4, dtype=torch.int64, **kw), torch.zeros((G, 4), dtype=torch.int64, **kw), torch.zeros((G, 4), dtype=torch.float32, **kw))
    s.tree.check()


# ------------------------------------------------------------------------------------------------ the route against the host loop
def episode_bytes(eps):
    return [(len(e), np.asarray(e.obs).tobytes(), np.asarray(e.actions).tobytes(), np.asarray(e.rewards).tobytes(),
             np.asarray(e.policies).tobytes(), np.asarray(e.root_values).tobytes()) for e in eps]


def make_env(kind):
    from rlzero_amd.muzero import AcrobotBatch, CartPoleBatch
    return AcrobotBatch(G, DEV, seed=9, max_episode_steps=12) if kind == 'acrobot' else CartPoleBatch(G, DEV, seed=9)


def play(kind, device_moves, replay=None, arena_rows=None, n_moves=30, **kw):
    """30 moves of 40 environments, 10 simulations, arg-max moves, no noise, chunks of five -> what the run handed out and left."""
    from rlzero_amd.muzero import MuZeroSelfPlay
    env = make_env(kind)
    net = make_net(env.obs_dim, env.n_actions)
    args = dict(n_sims=10, temperature=0.0, root_exploration_fraction=0.0, seed=4, moves_per_launch=5, fused_moves=False,
                device_moves=device_moves, arena_rows=arena_rows)
    args.update(kw)
    sp = MuZeroSelfPlay(net, env, **args)
    assert sp.device_moves == bool(device_moves) and not sp.fused_moves and sp.fused
    missed = []
    if device_moves:
        inner = sp._episodes_of_launch

        def spy(buf, replay=None):
            out = inner(buf, replay)
            missed.append(int(buf[1][0].numpy()[2]))
            return out
        sp._episodes_of_launch = spy
    eps = sp.collect(n_moves, replay=replay)
    sp.tree.check()
    out = dict(episodes=episode_bytes(eps), returns=eps.returns(), lengths=eps.lengths(), sims_done=sp.sims_done, moves_done=sp.moves_done,
               t=sp._t, episode=env.episode.copy(), steps=env.steps.cpu().numpy(), state=env.state.cpu().numpy(), missed=missed,
               obs=sp.obs.cpu().numpy(), history=sp.device_history() if device_moves else None, eps=eps)
    sp.close()
    return out


_HOST_LOOP = {}


def host_loop(kind):
    if kind not in _HOST_LOOP:
        _HOST_LOOP[kind] = play(kind, False)
    return _HOST_LOOP[kind]


def assert_same_run(got, want):
    assert len(got['episodes']) == len(want['episodes']) > 0 and got['episodes'] == want['episodes']
    for k in ('sims_done', 'moves_done', 't'):
        assert got[k] == want[k], k
    for k in ('episode', 'steps', 'state', 'obs'):
        assert same_bits(got[k], want[k]), k


def episodes_in_the_ring(history, n_moves, obs_dim, n_actions):
    """The finished episodes cut out of the device ring by its done flags, in the order of (last move, environment)."""
    from rlzero_amd.muzero.selfplay import Episode, EpisodeSeq
    ring, ep_start = history
    hist, out = ring.shape[1], []
    start = np.zeros(ring.shape[0], dtype=np.int64)
    for t in range(n_moves):
        for g in np.nonzero(ring[:, t % hist, obs_dim + 3 + n_actions] != 0.0)[0]:
            rows = ring[g, np.arange(start[g], t + 1) % hist]
            out.append(Episode.from_arrays(*EpisodeSeq.fields_of_packed(rows, obs_dim, n_actions)))
            start[g] = t + 1
    assert np.array_equal(start, ep_start)
    return out


@pytest.mark.parametrize('kind', ['acrobot', 'cartpole'])
def test_device_moves_hand_out_the_host_loops_episodes(kind):
    want = host_loop(kind)
    got = play(kind, True)
    assert_same_run(got, want)
    assert got['missed'] and not any(got['missed'])
    shape = (6, 3) if kind == 'acrobot' else (4, 2)
    assert 30 <= got['history'][0].shape[1]   # (the ring has not wrapped: all 30 moves are in it)
    assert episode_bytes(episodes_in_the_ring(got['history'], 30, *shape)) == want['episodes']
    if kind == 'acrobot':   # every episode runs into the limit of 12 here: returns of -12, two rounds of 40
        assert len(want['episodes']) == 2 * G and (want['lengths'] == 12).all() and (want['returns'] == -12.0).all()
    else:
        assert same_bits(want['returns'], want['lengths'].astype(np.float64)) and len(set(want['lengths'])) > 1


def test_device_moves_with_an_arena_too_small():
    """An arena of 8 rows holds no episode of 12 steps: every one of them is read from the ring, in the same order."""
    want = host_loop('acrobot')
    got = play('acrobot', True, arena_rows=8)
    assert_same_run(got, want)
    assert sum(got['missed']) == len(want['episodes']) > 0


def test_device_moves_on_a_side_stream():
    import torch
    want = host_loop('acrobot')
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = play('acrobot', True)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert_same_run(got, want)


def test_device_moves_do_not_depend_on_the_chunk():
    """One move per set of buffers, through ``play_move``: the same run as chunks of five."""
    from rlzero_amd.muzero import MuZeroSelfPlay
    want = host_loop('acrobot')
    env = make_env('acrobot')
    sp = MuZeroSelfPlay(make_net(), env, n_sims=10, temperature=0.0, root_exploration_fraction=0.0, seed=4, moves_per_launch=3)
    assert sp.device_moves and not sp.fused_moves   # (the default for an environment that is not CartPole)
    eps = []
    for _ in range(30):
        eps += list(sp.play_move())
    assert episode_bytes(eps) == want['episodes'] and sp._t == 30 and sp.moves_done == want['moves_done']
    assert same_bits(sp.obs.cpu().numpy(), want['obs'])
    sp.close()


def test_the_default_route_and_its_refusals():
    from rlzero_amd.muzero import CartPoleBatch, MuZeroNet, MuZeroSelfPlay
    cart = CartPoleBatch(G, DEV)
    sp = MuZeroSelfPlay(make_net(4, 2), cart)
    assert sp.fused_moves and not sp.device_moves   # CartPole keeps whole moves
    sp.close()
    sp = MuZeroSelfPlay(make_net(4, 2), cart, fused_moves=False)
    assert not sp.fused_moves and not sp.device_moves   # ... and the host loop behind fused_moves=False
    sp.close()
    with pytest.raises(ValueError, match='whole moves'):
        MuZeroSelfPlay(make_net(4, 2), cart, device_moves=True)
    with pytest.raises(ValueError, match='fused search'):
        MuZeroSelfPlay(MuZeroNet(6, 3, 32).to(DEV), make_env('acrobot'), device_moves=True)
    with pytest.raises(ValueError, match='below 0.1'):
        MuZeroSelfPlay(make_net(), make_env('acrobot'), device_moves=True, root_dirichlet_alpha=0.05)

    class Unknown(object):
        n_envs, n_actions, obs_dim, max_episode_steps, device = G, 3, 6, 12, cart.device

        def observe(self):
            return None
    with pytest.raises(ValueError, match='no kind'):
        MuZeroSelfPlay(make_net(), Unknown(), device_moves=True)
    sp = MuZeroSelfPlay(make_net(), Unknown())
    assert not sp.device_moves
    sp.close()
    sp = MuZeroSelfPlay(make_net(), make_env('acrobot'), root_dirichlet_alpha=0.05)   # the default falls back to the host loop
    assert not sp.device_moves
    sp.close()


# ------------------------------------------------------------------------------------------------ root noise
def test_device_moves_root_noise_is_the_restatement():
    """root_exploration_fraction = 1: root_children('prior') behind a chunk is muzero_eta for three actions of (episode, steps) before
    the chunk's last move -- the tolerance rule and the margin filter of test_whole_move_root_noise_is_the_restatement."""
    import torch
    from rlzero_amd._hip import HipError
    from rlzero_amd.muzero import MuZeroSelfPlay
    seed, alpha, chunk, chunks = 9, 0.25, 5, 6
    env = make_env('acrobot')
    sp = MuZeroSelfPlay(make_net(), env, n_sims=2, seed=seed, root_dirichlet_alpha=alpha, root_exploration_fraction=1.0, temperature=1.0,
                        moves_per_launch=chunk)
    assert sp.device_moves
    priors = []
    for _ in range(chunks):
        sp.collect(chunk)
        priors.append(sp.tree.root_children('prior').cpu().numpy().copy())
    ring, _ = sp.device_history()
    n_moves = chunk * chunks
    steps, episode = np.zeros((n_moves + 1, G), np.int64), np.zeros((n_moves + 1, G), np.int64)
    for t in range(n_moves):
        done = ring[:, t, D + 3 + A] != 0.0
        steps[t + 1] = np.where(done, 0, steps[t] + 1)
        episode[t + 1] = episode[t] + done
    assert np.array_equal(steps[-1], env.steps.cpu().numpy()) and np.array_equal(episode[-1], env.episode)
    g = np.arange(G)
    left_out, total, later, worst = 0, 0, 0, 0.0
    for i, pri in enumerate(priors):
        t = chunk * i + chunk - 1
        ref, margin, _ = ds.muzero_eta(seed, g, episode[t], steps[t], A, alpha)
        ref32, _, _ = ds.muzero_eta(seed, g, episode[t], steps[t], A, alpha, dtype=np.float32)
        assert pri.dtype == np.float64 and pri.shape == ref.shape
        assert np.max(np.abs(pri.sum(axis=1) - 1.0)) <= 1e-12 and (pri >= 0).all()
        keep = margin.min(axis=1) >= 1e-4
        t_rel = 4.0 * ds.relative_spread(ref[keep], ref32[keep])
        rel = np.abs(pri[keep] - ref[keep]) / ref[keep]
        assert t_rel < 1e-2 and (rel <= t_rel).all(), (i, float(rel.max()), t_rel)
        left_out, total, later, worst = left_out + int((~keep).sum()), total + G, later + int((episode[t][keep] > 0).sum()), max(worst, float(rel.max()))
    print('root noise, 3 actions: %d moves, %d left out, %d in a later episode, worst relative difference %.3e' % (total, left_out, later, worst))
    assert left_out <= 0.10 * total and later >= G
    # the draws of the actions at T = 1 are the restatement's too, record by record
    visits = ring[:, :n_moves, D + 2:D + 2 + A].astype(np.int64)
    want, _ = ds.muzero_action(seed, np.broadcast_to(g[:, None], (G, n_moves)), episode[:-1].T, steps[:-1].T, visits, 1.0)
    assert np.array_equal(ring[:, :n_moves, D].astype(np.int64), want)
    with pytest.raises(HipError, match='0.1'):
        sp.tree.root_noise(env.episode_dev, env.steps, seed, 0.05)
    sp.tree.check()
    sp.close()
    del torch


# ------------------------------------------------------------------------------------------------ hand-over to the device replay
def test_device_moves_hand_over_to_the_device_replay():
    """collect(replay=...) ingests from the launch arenas on the device; a second buffer is given the returned episodes through add.
    Every (episode, position) gathered from both: six tensors bit for bit, with rewards of -1 and value targets below zero."""
    from rlzero_amd.muzero import MuZeroDeviceReplay
    a = MuZeroDeviceReplay(D, A, 128, 12, device=DEV)
    b = MuZeroDeviceReplay(D, A, 128, 12, device=DEV)
    got = play('acrobot', True, replay=a)
    assert got['episodes'] == host_loop('acrobot')['episodes']
    b.add(got['eps'])
    assert len(a) == len(b) == len(got['episodes']) and np.array_equal(a.lengths(), b.lengths())
    draws = every_position(a.lengths(), a.K, A, np.random.RandomState(4))
    x, y = (tuple(v.cpu().numpy() for v in buf.gather(*draws)) for buf in (a, b))
    for name, u, v in zip(('obs', 'actions', 'tv', 'tr', 'tp', 'mask'), x, y):
        assert same_bits(u, v), name
    assert x[2].min() < -5.0 and set(np.unique(x[3])) == {-1.0, 0.0}   # (tr is 0 at k = 0 and past the end; the rewards are all -1)
    for buf in (a, b):
        assert buf.poll_errors() == 0
        buf.close()


# ------------------------------------------------------------------------------------------------ the trainer
def load_trainer():
    spec = importlib.util.spec_from_file_location('train_muzero', os.path.join(REPO, 'tools', 'train_muzero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


OLD_LINE = re.compile(r'^batch i:(\d+), episodes:(\d+), episode_len:([\d.]+), loss:(\S+), value:(\S+), reward:(\S+), policy:(\S+?)(, reanalysed:(\d+))?$')
NEW_LINE = re.compile(r'^batch i:(\d+), episodes:(\d+), episode_len:([\d.]+), episode_return:(-?[\d.]+), loss:(\S+), value:(\S+), reward:(\S+), '
                      r'policy:(\S+?)(, reanalysed:(\d+))?$')


@pytest.mark.parametrize('on_device', [True, False], ids=['device_replay_fused_learner', 'host_buffer_torch_learner'])
def test_the_trainer_runs_acrobot_end_to_end(capsys, on_device):
    mod = load_trainer()
    kw = dict(device_replay=True, fused_learner=True, prioritized_replay=True, reanalyse=64) if on_device else {}
    pipe = mod.MuZeroPipeline(env='acrobot', n_envs=32, n_sims=8, max_episode_steps=12, batch_size=32, updates_per_iteration=2, **kw)
    assert pipe.selfplay.device_moves and pipe.agent.net.obs_dim == 6 and pipe.env.n_actions == 3 and pipe.env.max_episode_steps == 12
    seen = []
    inner = pipe.selfplay.collect

    def collect(n_moves, replay=None):
        eps = inner(n_moves, replay=replay)
        seen.append(eps)
        return eps
    pipe.selfplay.collect = collect
    pipe.run(3)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('batch i:')]
    assert len(lines) == 3 and len(seen) == 3 and all(len(eps) > 0 for eps in seen)
    for line, eps in zip(lines, seen):
        m = NEW_LINE.match(line)
        assert m and int(m.group(2)) == len(eps), line
        assert all(np.isfinite(float(m.group(i))) for i in (5, 6, 7, 8)), line
        assert (m.group(10) is not None and int(m.group(10)) == 64) == on_device
        # the return is minus the number of steps that did not reach the goal
        non_terminal = [int((np.asarray(ep.rewards) != 0.0).sum()) for ep in eps]
        assert all(set(np.unique(ep.rewards)) <= {-1.0, 0.0} for ep in eps)
        assert abs(float(m.group(4)) + np.mean(non_terminal)) <= 0.05 + 1e-9 and abs(float(m.group(3)) - np.mean([len(ep) for ep in eps])) <= 0.05 + 1e-9
    assert pipe.episode_return == -float(np.mean([int((np.asarray(ep.rewards) != 0.0).sum()) for ep in seen[-1]]))
    if on_device:
        pipe.agent.check()
        assert pipe.buffer.poll_errors() == 0
    pipe.selfplay.tree.check()
    pipe.selfplay.close()
    if on_device:
        pipe.buffer.close()


def test_the_trainers_cartpole_line_is_the_one_it_printed(capsys):
    """Default environment: the line tests/test_mz_learner_gpu.py parses, and the return beside the length as an attribute (on
    CartPole the two are equal)."""
    mod = load_trainer()
    pipe = mod.MuZeroPipeline(n_envs=64, n_sims=8, batch_size=32, moves_per_iteration=30, updates_per_iteration=2, device_replay=True)
    assert pipe.selfplay.fused_moves and not pipe.selfplay.device_moves and pipe.env_name == 'cartpole'
    pipe.run(2)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('batch i:')]
    assert len(lines) == 2 and all(OLD_LINE.match(ln) for ln in lines), lines
    assert pipe.episode_return == pipe.episode_len > 0
    pipe.selfplay.close()
    pipe.buffer.close()
