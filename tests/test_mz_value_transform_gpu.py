"""MuZero's invertible value transform on the GPU: k_mz_search's VT instantiations (rz_mz_set_value_transform), the targets of
k_mzr_gather<true> / k_mzr_sample<true> (rz_mz_replay_set_value_transform), the flag's plumbing and the greedy evaluation.

G = 40 environments (two workgroups of 16 and half of a third), 20 simulations unless a tree placement needs another count.

1. Network.  ``rz_mz_search`` with VT at A = 2, 3 and 8, trees in LDS and in HBM, rew2 / val mapped so that the raw head outputs lie
   within about 1 and reach about 20, both signs (tests/test_mz_value_transform_host.py: scaled_heads).  Per simulation and game the
   float64 twin (tests/mz_net_twin.py) is applied to the kernel's OWN float32 parent state and traced action, its reward and value
   go through the twin's h^-1 (tests/mz_value_twin.py) and are compared with the traced reward and value -- every entry.  The
   tolerance is tests/test_mz_search_net_gpu.py's, applied after the inverse: YARDSTICK = 4 errors of the torch float32 route
   (``recurrent_inference`` then ``inverse_value_transform``, on the GPU, on the same inputs), floored at 2^-23 max |h^-1|.  The host
   test shows that a wrong inverse lands 12 tolerances or more away.  One run's ratios (MEASURED, MI355X: between 0.55 and 1.23 of
   the yardstick over the 24 figures): profiles/mz_value_transform/errors.txt.
2. Tree.  Every node, the MinMax bounds, the visit counts and the root values against oracle/muzero_ref.py fed the traced (MOVES =
   false) or unfolded (whole moves: tests/mz_unfold.py) expansions, bit for bit.
3. Routes, 4. targets, 5. refusals, 6. trainer and evaluation: the docstrings below."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import mz_net_twin
import mz_value_twin as vt
from mz_unfold import slot_of_path, unfold
from oracle import muzero_ref as ref
from test_muzero_moves_tree import _BareEnv, _replay as replay_cartpole
from test_mz_learner_host import YARDSTICK, copy_net
from test_mz_replay_host import assert_same_batch, every_position, host_sample, same_bits
from test_mz_value_transform_host import DISCOUNT, K, REACH, T, TD, episodes as host_episodes, scaled_heads
from test_mz_whole_env_gpu import _replay as replay_acrobot, episode_bytes, stream_pool_left_as_found  # noqa: F401  (the fixture: autouse)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = 40
N_SIMS = 20
U = 2.0 ** -23
OBS_DIM = 6   # the test nets of tests/test_mz_search_net_host.py


def _hexf(x):
    return float(x).hex()


# ----------------------------------------------------------------------------------------------- 1. the network
class Search(object):
    """A tree of G games with ``net64``'s float32 copy loaded, the value transform ``on`` or off."""

    def __init__(self, net64, n_sims, on=True):
        from rlzero_amd.muzero.tree import MuZeroTree
        self.A, self.n_sims = net64.n_actions, n_sims
        self.tree = MuZeroTree(G, self.A, n_sims, device=DEV)
        assert self.tree.value_transform is False
        if on:
            assert self.tree.set_value_transform(True) is self.tree and self.tree.value_transform is True
        self.hidden = torch.zeros((G, self.tree.slots_per_game, 64), dtype=torch.float32, device=DEV)
        self.obs = torch.randn(G, OBS_DIM, generator=torch.Generator().manual_seed(2000 + 10 * self.A + n_sims)).to(DEV)
        self.priors = torch.full((G, self.A), 1.0 / self.A, dtype=torch.float32, device=DEV)
        self.net32 = copy_net(net64, torch.float32, DEV).eval()
        self.tree.load_model(self.net32)

    def run(self):
        from rlzero_amd.muzero import inverse_value_transform
        self.hidden.zero_()
        with torch.no_grad():
            self.hidden[:, 0] = self.net32.initial_inference(self.obs)[0]
        self.tree.init_roots(self.priors)
        trace = self.tree.search_fused(self.hidden, self.n_sims, trace=True)
        rows = torch.arange(G, device=DEV)
        raw32, inv32 = [], []
        with torch.no_grad():
            for s in range(self.n_sims):
                _, r, _, v = self.net32.recurrent_inference(self.hidden[rows, trace['parent'][s].long()], trace['action'][s].long())
                raw32.append((r, v))
                inv32.append((inverse_value_transform(r), inverse_value_transform(v)))
        out = {k: v.cpu().numpy() for k, v in trace.items()}
        out['hidden'] = self.hidden.cpu().numpy()
        out['raw32'] = tuple(torch.cat([x[i] for x in raw32]).cpu().numpy() for i in range(2))
        out['inv32'] = tuple(torch.cat([x[i] for x in inv32]).double().cpu().numpy() for i in range(2))
        out['plan'] = self.tree.search_plan(False)
        n, vsum, vmin, vmax = (x.cpu().numpy().copy() for x in self.tree.root_stats())
        out['root'] = (n, vsum, vmin, vmax, self.tree.root_visits().cpu().numpy().copy())
        assert (n == self.n_sims).all()
        self.tree.check()
        return out

    def close(self):
        self.tree.close()


# (A, n_sims, trees in LDS): the plan's own formula, asserted
NET_SHAPES = ((2, 20, True), (2, 64, False), (3, 20, True), (3, 40, False), (8, 12, True), (8, 40, False))


@pytest.mark.parametrize('reach', REACH)
@pytest.mark.parametrize('A,n_sims,in_lds', NET_SHAPES)
def test_the_kernels_inverted_reward_and_value_against_the_twin(A, n_sims, in_lds, reach):
    net64 = scaled_heads(A, reach)
    search = Search(net64, n_sims)
    out = search.run()
    search.close()
    assert out['plan']['tree_in_lds'] == in_lds and out['plan']['games_per_workgroup'] == 16, out['plan']
    S = out['parent'].shape[0]
    games = np.broadcast_to(np.arange(G), (S, G))
    states = out['hidden'][games, out['parent']].reshape(S * G, 64)
    want = mz_net_twin.recurrent(mz_net_twin.state_dict64(net64), states.astype(np.float64), out['action'].reshape(-1))
    what = 'A=%d n_sims=%d (%s) reach %g' % (A, n_sims, 'LDS' if in_lds else 'HBM', reach)
    for name, y, got, inv32 in (('reward', want.reward, out['reward'], out['inv32'][0]), ('value', want.value, out['value'], out['inv32'][1])):
        got = got.reshape(-1).astype(np.float64)
        assert got.shape == y.shape == (S * G, ) and np.isfinite(got).all()   # every entry of the trace
        raw = vt.h_inv_array(y)
        assert (y > 0).any() and (y < 0).any() and 0.3 * reach <= np.abs(y).max() <= 3.0 * reach, (what, name, y.min(), y.max())
        err = float(np.abs(got - raw).max())
        yard = max(float(np.abs(inv32 - raw).max()), U * float(np.abs(raw).max()))
        print('%s %s: |y| <= %.2f, raw within %.1f: HIP error %.3e, torch-f32 yardstick %.3e, ratio %.2f'
              % (what, name, np.abs(y).max(), np.abs(raw).max(), err, yard, err / yard))
        assert err <= YARDSTICK * yard, (what, name, err, yard)
    # the other two quantities are the kernel's as before (the tolerance of tests/test_mz_search_net_gpu.py)
    leaf = out['hidden'][games, out['leaf']].reshape(S * G, 64)
    assert np.abs(leaf - want.next_state).max() <= 1e-4 and np.abs(out['probs'].reshape(S * G, -1) - want.probs).max() <= 1e-4


def test_the_first_simulation_of_a_whole_move_inverts_what_the_plain_kernel_backs_up():
    """Whole moves have no trace, but the first simulation of a move descends by the priors alone: with the flag on and off it
    expands the same edge from the same state, so the unfolded reward and value of the two runs are y and float32(h^-1(float64(y)))
    of the same float32 y -- bit for bit, for CartPole and Acrobot (the twin's fp64 sqrt against the device's)."""
    from rlzero_amd.muzero import AcrobotBatch, CartPoleBatch
    for env_class in (CartPoleBatch, AcrobotBatch):
        first = {}
        for on in (False, True):
            run = whole_move_run(env_class, 1.0, on, moves=1)
            first[on] = [unfold(run['nodes'][g], run['top'][g], env_class.n_actions, run['discount'])[0][0] for g in range(G)]
        moved = 0
        for off, on in zip(first[False], first[True]):
            assert (off.path, off.action) == (on.path, on.action) and off.probs.tobytes() == on.probs.tobytes()
            for y, x in ((off.reward, on.reward), (off.value, on.value)):
                assert same_bits(np.float32(x).reshape(1), vt.h_inv_f32(np.float32(y).reshape(1)))
                moved += float(x) != float(y)
        assert moved >= G   # (the inverse is not the identity on these heads)


# ----------------------------------------------------------------------------------------------- 2. the tree
def vt_net(obs_dim, n_actions, seed=7, head_gain=6.0):
    """A MuZeroNet that owns the flag, its reward and value heads scaled so that h^-1 is far from the identity."""
    from rlzero_amd.muzero import MuZeroNet
    torch.manual_seed(seed)
    net = MuZeroNet(obs_dim, n_actions, value_transform=True).to(DEV).eval()
    with torch.no_grad():
        for layer in (net.rew2, net.val):
            layer.weight.mul_(head_gain)
    return net


@pytest.mark.parametrize('A,n_sims,in_lds', [(2, 20, True), (3, 40, False)])
def test_traced_search_trees_are_the_pseudocodes_bit_for_bit(A, n_sims, in_lds):
    """MOVES = false with VT: the restatement fed the TRACED expansions (which hold what entered the backup) builds the device's
    tree -- every node, the MinMax bounds, the visit counts, the root value.  The trace is h^-1 of the net's own float32 outputs."""
    from rlzero_amd.muzero import MuZeroSelfPlay, inverse_value_transform
    net = vt_net(4, A)
    obs = torch.randn(G, 4, generator=torch.Generator().manual_seed(5)).to(DEV)
    sp = MuZeroSelfPlay(net, _BareEnv(G, A, obs), n_sims=n_sims, seed=3, fused=True)
    assert sp.fused and not sp.fused_moves and sp.value_transform and sp.tree.value_transform
    assert sp.tree.search_plan(False)['tree_in_lds'] == in_lds
    record = []
    visits, root_value = sp.search(obs, add_noise=True, record=record)
    visits, root_value = visits.cpu().numpy(), root_value.cpu().numpy()
    n, vsum, vmin, vmax = (x.cpu().numpy().copy() for x in sp.tree.root_stats())
    nodes, top = sp.tree.nodes()
    _, probs0, noise = record[0]
    probs0, noise = probs0.cpu().numpy(), noise.cpu().numpy()
    sims = [tuple(x.cpu().numpy() for x in r) for r in record[1:]]
    cfg = ref.MuZeroConfig(num_simulations=n_sims)
    for g in range(G):
        root = ref.Node(0)
        ref.expand_node(root, None, 0.0, [float(p) for p in probs0[g]])
        ref.add_exploration_noise(cfg, root, [float(x) for x in noise[g]])
        step = [0]

        def model(hidden, action, path, g=g, step=step):
            parent, act, leaf, reward, probs, value = sims[step[0]]
            assert act[g] == action
            step[0] += 1
            return None, float(reward[g]), [float(p) for p in probs[g]], float(value[g])

        stats = ref.run_mcts(cfg, root, model)
        assert root.visit_count == n[g] == n_sims and _hexf(root.value_sum) == _hexf(vsum[g])
        assert _hexf(stats.minimum) == _hexf(vmin[g]) and _hexf(stats.maximum) == _hexf(vmax[g])
        assert [c.visit_count for c in root.children] == visits[g].tolist() and _hexf(root.value()) == _hexf(root_value[g])
        dump = ref.tree_dump(root)
        assert len(dump) == top[g]
        for path, (cnt, value_sum, reward, prior) in dump.items():
            nd = nodes[g][slot_of_path(nodes[g], path)]
            assert cnt == nd['N'] and (_hexf(value_sum), _hexf(reward), _hexf(prior)) == (_hexf(nd['value_sum']), _hexf(nd['reward']), _hexf(nd['prior']))
    # what was traced: within the float32 yardstick of h^-1 of the torch net's outputs on the same states (the network test above
    # holds it to the twin; here only that the trace is in RAW units, far from the heads' own outputs)
    rows = torch.arange(G, device=DEV)
    with torch.no_grad():
        _, r, _, v = net.recurrent_inference(sp.hidden[rows, torch.from_numpy(sims[0][0]).to(DEV).long()], torch.from_numpy(sims[0][1]).to(DEV).long())
    for got, y in ((sims[0][3], r), (sims[0][5], v)):
        raw = inverse_value_transform(y).cpu().numpy()
        assert np.abs(got - raw).max() <= 1e-4 * max(1.0, np.abs(raw).max()) and np.abs(raw - y.cpu().numpy()).max() > 0.05
    sp.tree.check()
    sp.close()


_WHOLE = {}


def whole_move_run(env_class, temperature, on=True, moves=3):
    """``moves`` whole moves of G environments in ONE launch; the trees of the last move and its record, as host arrays."""
    key = (env_class.__name__, temperature, on, moves)
    if key not in _WHOLE:
        from rlzero_amd.muzero import MuZeroSelfPlay
        net = vt_net(env_class.obs_dim, env_class.n_actions)
        net.value_transform = on
        sp = MuZeroSelfPlay(net, env_class(G, DEV, seed=3), n_sims=N_SIMS, seed=9, temperature=temperature, fused=True, fused_moves=True,
                            moves_per_launch=moves)
        assert sp.fused_moves and sp.value_transform == on and sp.tree.value_transform == on
        sp.collect(moves)
        nodes, top = sp.tree.nodes()
        ring, _ = sp.device_history()
        n, vsum, vmin, vmax = (x.cpu().numpy().copy() for x in sp.tree.root_stats())
        _WHOLE[key] = dict(n_sims=N_SIMS, discount=sp.discount, nodes=nodes, top=top, record=ring[:, moves - 1].copy(), ring=ring[:, :moves].copy(),
                           root_n=n, root_sum=vsum, vmin=vmin, vmax=vmax)
        sp.tree.check()
        sp.close()
    return _WHOLE[key]


@pytest.mark.parametrize('temperature', [1.0, 0.0])
@pytest.mark.parametrize('kind', ['cartpole', 'acrobot'])
def test_whole_move_trees_with_the_transform_are_the_pseudocodes(kind, temperature):
    """3 moves of one launch with VT, root noise on: the last move's trees, every game, through the helpers of
    tests/test_muzero_moves_tree.py (CartPole) and tests/test_mz_whole_env_gpu.py (Acrobot) as they are."""
    from rlzero_amd.muzero import AcrobotBatch, CartPoleBatch
    run = whole_move_run(CartPoleBatch if kind == 'cartpole' else AcrobotBatch, temperature)
    replay = replay_cartpole if kind == 'cartpole' else replay_acrobot
    for g in range(G):
        replay(run, g)
    A, D = (2, 4) if kind == 'cartpole' else (3, 6)
    if temperature == 0.0:   # the arg-max of the visit counts, in every record of the launch
        vis = run['ring'][:, :, D + 2:D + 2 + A]
        act = run['ring'][:, :, D].astype(np.int64)
        assert (np.take_along_axis(vis, act[:, :, None], axis=2)[:, :, 0] == vis.max(axis=2)).all()


# ----------------------------------------------------------------------------------------------- 3. routes
def test_the_host_step_loop_inverts_the_heads_also_inside_its_graph():
    """``fused=False``: a record's reward and value are ``inverse_value_transform`` of the net's outputs on the recorded parent state
    and action, bit for bit; the replayed hipGraph (no record) builds the same trees as the eager loop."""
    from rlzero_amd.muzero import CartPoleBatch, MuZeroSelfPlay, inverse_value_transform
    net = vt_net(4, 2)
    env = CartPoleBatch(G, DEV, seed=2)
    sp = MuZeroSelfPlay(net, env, n_sims=N_SIMS, seed=5, fused=False)
    assert not sp.fused and sp.value_transform and sp._graph is not None
    obs = env.observe()
    record = []
    v_eager, rv_eager = sp.search(obs, add_noise=False, record=record)
    v_eager, rv_eager = v_eager.clone(), rv_eager.clone()
    rows = torch.arange(G, device=DEV)
    moved = 0
    with torch.no_grad():
        for parent, action, leaf, reward, probs, value in record[1:]:
            _, r, _, v = net.recurrent_inference(sp.hidden[rows, parent.long()], action.long())
            assert torch.equal(reward, inverse_value_transform(r)) and torch.equal(value, inverse_value_transform(v))
            moved += int((value != v).sum())
    assert moved >= G * N_SIMS // 2
    v_graph, rv_graph = sp.search(obs, add_noise=False)
    assert torch.equal(v_graph, v_eager) and torch.equal(rv_graph, rv_eager)
    # the same search with the flag off is another search
    net.value_transform = False
    plain = MuZeroSelfPlay(net, env, n_sims=N_SIMS, seed=5, fused=False, use_graph=False)
    _, rv_plain = plain.search(obs, add_noise=False)
    assert not torch.equal(rv_plain, rv_eager)
    for x in (sp, plain):
        x.tree.check()
        x.close()


def _six_moves(env_class, route, collects, moves_per_launch, side=False):
    """Six moves of G environments with the flag on, split into ``collects`` -> (ring, states, finished episodes) as bytes."""
    from rlzero_amd.muzero import MuZeroSelfPlay
    net = vt_net(env_class.obs_dim, env_class.n_actions)
    kw = dict(max_episode_steps=4) if env_class.kind == 'acrobot' else {}
    env = env_class(G, DEV, seed=11, **kw)

    def play():
        # (an arena of 512 rows: the episodes that end in one launch fit it at every split -- tests/test_mz_whole_env_gpu.py says why)
        sp = MuZeroSelfPlay(net, env, n_sims=N_SIMS, seed=4, temperature=1.0, fused=True, moves_per_launch=moves_per_launch, arena_rows=512,
                            **route)
        assert sp.value_transform and sp.tree.value_transform
        eps = []
        for n in collects:
            eps.extend(sp.collect(n))
        ring, ep_start = sp.device_history()
        sp.tree.check()
        out = (ring[:, :6].tobytes(), ep_start.tobytes(), env.state.cpu().numpy().tobytes(), env.steps.cpu().numpy().tobytes(), episode_bytes(eps))
        sp.close()
        return out, ring[:, :6].copy()

    if not side:
        return play()
    stream = torch.cuda.Stream(device=DEV, priority=-1)   # (the high-priority pool: tests/test_mz_learner_gpu.py says why)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        out = play()
    torch.cuda.current_stream(DEV).wait_stream(stream)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('kind', ['cartpole', 'acrobot'])
def test_whole_moves_with_the_transform_do_not_depend_on_launch_splits_or_the_stream(kind):
    """6 = 6, 3 + 3 and 6 x 1 moves per launch, and 6 on a side stream: the same records, states and episodes, bit for bit."""
    from rlzero_amd.muzero import AcrobotBatch, CartPoleBatch
    env_class = CartPoleBatch if kind == 'cartpole' else AcrobotBatch
    route = dict(fused_moves=True)
    base, ring = _six_moves(env_class, route, (6, ), 6)
    D, A = env_class.obs_dim, env_class.n_actions
    assert (ring[:, :, D + 2:D + 2 + A].sum(axis=2) == N_SIMS).all() and np.isfinite(ring).all()
    if kind == 'acrobot':
        assert len(base[4]) >= G   # (a time limit of 4: every environment ended an episode, through the arena)
    for collects, per_launch, side in (((3, 3), 3, False), ((6, ), 1, False), ((6, ), 6, True)):
        got, _ = _six_moves(env_class, route, collects, per_launch, side)
        for i, (a, b) in enumerate(zip(base, got)):
            assert a == b, (i, collects, per_launch, side)


def test_device_moves_with_the_transform():
    """Device moves (Acrobot's default route) with the flag on: 6 = 6 and 3 + 3 give the same records bit for bit, and the first
    move's visit counts and root value are those of ``MuZeroSelfPlay.search`` on a VT tree from the same observations (no noise)."""
    from rlzero_amd.muzero import AcrobotBatch, MuZeroSelfPlay
    route = dict(fused_moves=False, device_moves=True)
    base, ring = _six_moves(AcrobotBatch, route, (6, ), 6)
    got, _ = _six_moves(AcrobotBatch, route, (3, 3), 3)
    for a, b in zip(base, got):
        assert a == b
    net = vt_net(6, 3)
    env = AcrobotBatch(G, DEV, seed=11, max_episode_steps=4)
    moves = MuZeroSelfPlay(net, env, n_sims=N_SIMS, seed=4, fused=True, device_moves=True, root_exploration_fraction=0.0, moves_per_launch=1)
    assert moves.device_moves and moves.value_transform
    obs = env.observe().clone()
    moves.collect(1)
    ring, _ = moves.device_history()
    search = MuZeroSelfPlay(net, _BareEnv(G, 3, obs), n_sims=N_SIMS, seed=4, fused=True)
    visits, root_value = search.search(obs, add_noise=False)
    assert np.array_equal(ring[:, 0, 8:11].astype(np.int32), visits.cpu().numpy()) and same_bits(ring[:, 0, 11].copy(), root_value.cpu().numpy())
    search.tree.set_value_transform(False)
    _, plain_value = search.search(obs, add_noise=False)
    assert not torch.equal(plain_value.cpu(), torch.from_numpy(ring[:, 0, 11].copy()))
    for x in (moves, search):
        x.tree.check()
        x.close()


# ----------------------------------------------------------------------------------------------- 4. targets
D6, A3 = 6, 3


def filled(value_transform, prioritized=False, seed=17):
    """A device buffer and a host buffer holding the host test's episodes: D = 6, A = 3, negative rewards, lengths 1 .. K + td + 3."""
    from rlzero_amd.muzero import MuZeroDeviceReplay, ReplayBuffer
    eps = host_episodes(11)
    assert [len(ep) for ep in eps] == list(range(1, K + TD + 4)) and all((ep.rewards < 0).all() for ep in eps)
    dev = MuZeroDeviceReplay(D6, A3, 64, T, unroll_steps=K, td_steps=TD, discount=DISCOUNT, device=DEV, seed=seed, prioritized=prioritized,
                             value_transform=value_transform)
    host = ReplayBuffer(capacity=64, unroll_steps=K, td_steps=TD, discount=DISCOUNT, seed=seed, value_transform=value_transform)
    assert dev.add(eps) == len(eps)
    for ep in eps:
        host.add(ep)
    assert dev.value_transform == host.value_transform == value_transform
    return dev, host


def on_host(batch):
    return tuple(x.cpu().numpy() for x in batch)


def test_the_device_targets_equal_the_host_buffers():
    from rlzero_amd.muzero import mz_replay_draws
    dev, host = filled(True)
    plain, plain_host = filled(False)
    draws = every_position([len(ep) for ep in host.episodes], K, A3, np.random.RandomState(2))
    want = host_sample(host, draws, A3)
    got = on_host(dev.gather(*draws))
    assert_same_batch(got, want)
    assert_same_batch(on_host(dev.gather(*(torch.from_numpy(x).to(DEV) for x in draws))), want)   # the same draws from the device
    # (tests/test_mz_value_transform_host.py holds the host buffer to the twin's h of the fp64 targets.)  Against the buffer without
    # the flag only tv and tr differ
    off = on_host(plain.gather(*draws))
    assert_same_batch(off, host_sample(plain_host, draws, A3))
    for i in (0, 1, 4, 5):
        assert same_bits(got[i], off[i])
    inside = off[5] != 0.0
    assert (got[2][inside] != off[2][inside]).all() and (got[2][~inside] == 0.0).all() and got[2].min() < -3.0 and off[2].min() < -60.0
    # sample: gather of the restated draws
    for step in range(2):
        restated = mz_replay_draws(17, step, 64, dev.lengths(), K, A3)
        assert_same_batch(on_host(dev.sample(64)), on_host(dev.gather(*restated)))
    for buf in (dev, plain):
        assert buf.poll_errors() == 0
        buf.close()


def test_prioritized_samples_are_transformed_and_priorities_stay_raw():
    dev, host = filled(True, prioritized=True)
    plain, _ = filled(False, prioritized=True)
    w_on, w_off = dev.priorities(), plain.priorities()
    assert len(w_on) == len(w_off) == len(host.episodes)
    for a, b in zip(w_on, w_off):
        assert np.array_equal(a, b)
    assert max(int(w.max()) for w in w_on) > 65536   # (|root value - return| above 1 in raw units: nothing was squashed)
    (batch_on, weights_on), (batch_off, weights_off) = dev.sample_prioritized(48, step=3), plain.sample_prioritized(48, step=3)
    ep_idx, pos, filler, _ = dev.prioritized_draws(48, step=3)
    assert_same_batch(on_host(batch_on), host_sample(host, (ep_idx.cpu().numpy(), pos.cpu().numpy(), filler.cpu().numpy()), A3))
    on, off = on_host(batch_on), on_host(batch_off)
    assert torch.equal(weights_on, weights_off)
    for i in (0, 1, 4, 5):   # the same draws (the priorities are the same), the same rows but for tv and tr
        assert same_bits(on[i], off[i])
    inside, prev = off[5] != 0.0, off[3] != 0.0
    assert inside.any() and (on[2][inside] != off[2][inside]).all() and (on[2][~inside] == 0.0).all()
    assert prev.any() and (np.abs(on[3][prev]) < np.abs(off[3][prev])).all()   # |h(r)| < |r|
    for buf in (dev, plain):
        assert buf.poll_errors() == 0
        buf.close()


def test_reanalyse_writes_back_the_raw_root_value_of_a_vt_search():
    from rlzero_amd.muzero import MuZeroReanalyser, MuZeroSelfPlay
    dev, host = filled(True)
    net = vt_net(D6, A3)
    rean = MuZeroReanalyser(net, dev, n_sims=N_SIMS, batch=16, fused=True, seed=21)
    assert rean.value_transform and rean.tree.value_transform
    lengths = [len(ep) for ep in host.episodes]
    ep_idx, pos, _ = every_position(lengths, K, A3, np.random.RandomState(1))
    pick = np.random.RandomState(6).permutation(len(ep_idx))[:16]
    ep_idx, pos = ep_idx[pick], pos[pick]
    before = dev.read()
    assert rean.reanalyse(ep_idx, pos) == 16
    after = dev.read()
    obs = torch.from_numpy(np.stack([host.episodes[e].obs[p] for e, p in zip(ep_idx, pos)]).astype(np.float32)).to(DEV)
    sp = MuZeroSelfPlay(net, _BareEnv(16, A3, obs), n_sims=N_SIMS, fused=True, use_graph=False)
    assert sp.tree.value_transform
    visits, root_value = sp.search(obs, add_noise=False)
    visits, root_value = visits.cpu().numpy(), root_value.cpu().numpy()
    sp.tree.set_value_transform(False)
    _, plain_value = sp.search(obs, add_noise=False)
    plain_value = plain_value.cpu().numpy()
    for i, (e, p) in enumerate(zip(ep_idx, pos)):
        assert same_bits(after[e].root_values[p:p + 1], root_value[i:i + 1]), (e, p)
        assert same_bits(after[e].policies[p], (visits[i] / visits[i].sum()).astype(np.float32))
        assert after[e].root_values[p] != before[e].root_values[p] and after[e].root_values[p] != plain_value[i]
    assert same_bits(np.concatenate([ep.rewards for ep in after]), np.concatenate([ep.rewards for ep in before]))
    rean.close(), sp.close(), dev.close()


# ----------------------------------------------------------------------------------------------- 5. refusals
def load_trainer():
    spec = importlib.util.spec_from_file_location('train_muzero', os.path.join(REPO, 'tools', 'train_muzero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_turning_the_transform_off_gives_the_tree_that_never_had_it():
    net64 = scaled_heads(3, 20.0)
    a = Search(net64, N_SIMS, on=True)
    with_vt = a.run()
    a.tree.set_value_transform(False)
    assert a.tree.value_transform is False
    after = a.run()
    a.close()
    b = Search(net64, N_SIMS, on=False)
    never = b.run()
    b.close()
    for k in ('parent', 'action', 'leaf', 'reward', 'probs', 'value', 'hidden'):
        assert same_bits(after[k], never[k]), k
    for x, y in zip(after['root'], never['root']):
        assert same_bits(x, y)
    assert not same_bits(with_vt['value'], never['value']) and not same_bits(with_vt['root'][1], never['root'][1])


def test_a_net_and_a_buffer_that_disagree_are_refused_before_any_launch(tmp_path):
    from rlzero_amd._hip import HipError
    from rlzero_amd.muzero import MuZeroAgent, MuZeroDeviceReplay, MuZeroReanalyser, ReplayBuffer
    mod = load_trainer()
    kw = dict(n_envs=G, n_sims=8, batch_size=32, updates_per_iteration=2, device_replay=True, fused_learner=True)
    pipe = mod.MuZeroPipeline(value_transform=True, **kw)
    assert pipe.agent.net.value_transform and pipe.buffer.value_transform and pipe.selfplay.value_transform
    own = pipe.buffer
    for wrong in (MuZeroDeviceReplay(4, 2, 64, 500, device=DEV), ReplayBuffer()):
        pipe.buffer = wrong
        version = [p._version for p in pipe.agent.net.parameters()]
        with pytest.raises(ValueError) as info:
            pipe.policy_update()
        assert 'net has value_transform=True' in str(info.value) and '%s) has value_transform=False' % type(wrong).__name__ in str(info.value)
        assert version == [p._version for p in pipe.agent.net.parameters()]   # (no update ran)
        with pytest.raises(ValueError, match='value_transform'):
            pipe.agent.learn_async(None, buffer=wrong)
        with pytest.raises(ValueError, match='value_transform'):
            pipe.agent.learn(None, buffer=wrong)
        if isinstance(wrong, MuZeroDeviceReplay):
            with pytest.raises(ValueError, match='net has value_transform=True'):
                MuZeroReanalyser(pipe.agent.net, wrong, n_sims=8, batch=16)
            wrong.close()
    pipe.buffer = own
    # checkpoints: the key only when the flag is on; the other setting is refused and nothing is loaded
    plain = MuZeroAgent(device=DEV, fused_learner=True, max_batch=32)
    p_on, p_off = str(tmp_path / 'on.model'), str(tmp_path / 'off.model')
    pipe.agent.save_model(p_on)
    plain.save_model(p_off)
    assert torch.load(p_on)['value_transform'] is True and sorted(torch.load(p_off)) == ['model', 'optimizer']
    pipe.agent.load_model(p_on)
    plain.load_model(p_off)
    for agent, path in ((pipe.agent, p_off), (plain, p_on)):
        before = [p.clone() for p in agent.net.parameters()]
        with pytest.raises(ValueError, match='saved with value_transform'):
            agent.load_model(path)
        assert all(torch.equal(x, y) for x, y in zip(before, agent.net.parameters()))
    # the library's two entries take 0 or 1
    from rlzero_amd._hip import check
    with pytest.raises(HipError, match='0 .off. or 1'):
        check(pipe.selfplay.tree.lib.rz_mz_set_value_transform(pipe.selfplay.tree.handle, 2), 'rz_mz_set_value_transform')
    with pytest.raises(HipError, match='0 .off. or 1'):
        check(own.lib.rz_mz_replay_set_value_transform(own.handle, -1), 'rz_mz_replay_set_value_transform')
    pipe.selfplay.close()
    own.close()


# ----------------------------------------------------------------------------------------------- 6. the trainer and the evaluation
def _pipeline(mod, env, whole_moves, **more):
    kw = dict(env=env, n_envs=G, n_sims=N_SIMS, batch_size=32, updates_per_iteration=2, device_replay=True, fused_learner=True,
              value_transform=True, whole_moves=whole_moves, moves_per_iteration=32 if env == 'cartpole' else 16)
    if env == 'acrobot':
        kw['max_episode_steps'] = 12
    kw.update(more)
    torch.manual_seed(3)   # (the net's initial weights come from torch's global generator: two pipelines are twins only behind the same seed)
    return mod.MuZeroPipeline(**kw)


def _close(pipe):
    pipe.agent.check()
    assert pipe.buffer.poll_errors() == 0
    pipe.selfplay.tree.check()
    pipe.selfplay.close()
    if pipe._evaluator is not None:
        pipe._evaluator[0].tree.check()
        pipe._evaluator[0].close()
    pipe.buffer.close()


@pytest.mark.parametrize('env,whole_moves', [('cartpole', None), ('acrobot', None), ('acrobot', True)])
def test_the_pipeline_trains_and_evaluates_with_the_transform(capsys, env, whole_moves):
    """Two iterations with the flag on, the device replay and the fused learner; ``evaluate`` returns exactly n_envs episodes, twice the
    same numbers with no update in between, greedy first moves, and leaves the training run's episodes as they would have been."""
    mod = load_trainer()
    pipe = _pipeline(mod, env, whole_moves)
    sp = pipe.selfplay
    assert sp.value_transform and sp.tree.value_transform and pipe.buffer.value_transform and pipe.agent.net.value_transform
    assert sp.fused_moves == (env == 'cartpole' or bool(whole_moves)) and sp.device_moves == (env == 'acrobot' and not whole_moves)
    pipe.run(2, eval_every=1)
    out = capsys.readouterr().out
    batch_lines = [ln for ln in out.splitlines() if ln.startswith('batch i:')]
    eval_lines = [ln for ln in out.splitlines() if ln.startswith('eval i:')]
    from test_mz_env_gpu import NEW_LINE, OLD_LINE
    assert len(batch_lines) == 2 and all((OLD_LINE if env == 'cartpole' else NEW_LINE).match(ln) for ln in batch_lines), out
    assert len(eval_lines) == 2 and all('episodes:%d,' % G in ln for ln in eval_lines), out
    ev = pipe._evaluator[0]
    assert ev is not sp and ev.env is not pipe.env and ev.temperature == 0.0 and ev.noise_frac == 0.0 and ev.value_transform
    assert (ev.fused_moves, ev.device_moves) == (sp.fused_moves, sp.device_moves)
    first = pipe.evaluate()
    episodes = pipe.eval_episodes
    second = pipe.evaluate()
    assert first == second and first['count'] == G == len(episodes) and pipe._evaluator[0] is ev   # (built once)
    assert first['length_min'] >= 1 and first['length_max'] <= pipe.env.max_episode_steps
    assert first['return_min'] <= first['return_mean'] <= first['return_max']
    if env == 'cartpole':
        assert first['return_mean'] == first['length_mean']
    else:
        assert first['return_max'] <= 0.0
    for ep in episodes:   # temperature 0: the move is an arg-max of the search's visit counts
        assert ep.policies[0][int(ep.actions[0])] == ep.policies[0].max()
    few = pipe.evaluate(n_envs=7)
    assert few['count'] == 7 and pipe._evaluator[0] is not ev
    # the training run does not notice: a twin pipeline that never evaluates collects the same episodes, before and after
    a, b = _pipeline(mod, env, whole_moves), _pipeline(mod, env, whole_moves)
    for k in range(2):
        got_a = episode_bytes(a.selfplay.collect(16))
        a.evaluate(n_envs=16)
        got_b = episode_bytes(b.selfplay.collect(16))
        assert got_a == got_b and (k == 0 or len(got_a) > 0)
    for x in (pipe, a, b):
        _close(x)


def test_the_trainers_flags_through_main(capsys):
    mod = load_trainer()
    argv = ['--envs', str(G), '--sims', '8', '--iterations', '2', '--device-replay', '--fused-learner', '--batch-size', '32',
            '--updates-per-iteration', '2', '--value-transform', '--eval-every', '2', '--eval-envs', '16']
    pipe = mod.main(argv)
    out = capsys.readouterr().out
    assert len([ln for ln in out.splitlines() if ln.startswith('batch i:')]) == 2
    evals = [ln for ln in out.splitlines() if ln.startswith('eval i:')]
    assert len(evals) == 1 and evals[0].startswith('eval i:2, episodes:16, return mean:'), out
    assert pipe.value_transform and pipe.selfplay.tree.value_transform and pipe._evaluator[1] == 16
    _close(pipe)
    plain = mod.main(argv[:-5])   # without the three flags: no evaluator, no transform, the lines as they were
    out = capsys.readouterr().out
    assert 'eval' not in out and not plain.value_transform and not plain.selfplay.tree.value_transform and plain._evaluator is None
    _close(plain)
