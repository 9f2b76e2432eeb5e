"""Gumbel MuZero's rule in the one-launch search (k_mz_search's GUMBEL instantiations, ``MuZeroTree.set_gumbel`` / ``search_gumbel``)
against the float64 twin rlzero_amd/muzero/gumbel.py, which is fed the kernel's own traced network outputs, the roots' raw values the
kernel kept and the same Gumbel draws: every node of every tree, the MinMax bounds, (parent, action, leaf) of every simulation, the move
and the most-visited set are EQUAL, pi' is within 1.2e-7 (one float32 rounding, 2^-24, plus the 1e-12 of exp / log) of the twin's.
A game whose smallest decision gap in the twin is below 1e-9 is left out of the exact comparison: at most one of the 40 per case.

40 games: two full workgroups of 16 and a partial one (ten of 4).  The nets are those of tests/test_mz_search_net_host.py (random, the
policy head with their logits gain); the roots' priors are the net's own policy.  The cases cover A in {2, 3, 5, 8}, max_considered in
{1, 3, 4, 16} (3 is no power of two, 16 clamps to A), n_sims in {1, 5, 16, 50} (budgets below m too), trees in LDS and in HBM (by the
plan, asserted), 16 and 4 games per workgroup, the value transform once, and g = 0 (the greedy move) once."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from rlzero_amd.muzero import gumbel as twin
import test_mz_env_gpu as mz_env
from test_mz_learner_host import copy_net
from test_mz_search_net_host import OBS_DIM, rolled_net

pytestmark = pytest.mark.gpu
DEV, GAMES = 'cuda:0', 40
#        A  m  n_sims gpw value-transform  g = 0   trees in LDS
CASES = [(2, 1, 1, 16, False, False, True), (2, 4, 5, 4, False, False, True), (2, 3, 50, 16, False, False, False),
         (3, 3, 16, 16, False, False, True), (3, 16, 50, 16, False, False, False), (3, 3, 1, 4, False, True, True),
         (5, 4, 16, 4, False, False, True), (5, 3, 50, 4, False, False, True), (5, 16, 5, 16, False, True, True),
         (8, 16, 50, 16, False, False, False), (8, 4, 16, 4, True, False, True), (8, 1, 5, 4, False, False, True),
         (8, 3, 50, 4, False, False, False)]
_runs = {}


def run(case):
    """One search and its twin: run once, shared by the tests below, never modified."""
    if case in _runs:
        return _runs[case]
    from rlzero_amd.muzero import inverse_value_transform
    from rlzero_amd.muzero.tree import MuZeroTree
    A, m, n_sims, gpw, vt, greedy, _ = case
    net32 = copy_net(rolled_net(A, 0), torch.float32, DEV).eval()
    tree = MuZeroTree(GAMES, A, n_sims, device=DEV).set_search_shape(gpw).set_value_transform(vt).set_gumbel(m)
    tree.load_model(net32)
    gen = torch.Generator().manual_seed(100 * A + n_sims + m)
    obs = torch.randn(GAMES, OBS_DIM, generator=gen).to(DEV)
    u = torch.rand(GAMES, A, generator=gen).clamp_(1e-6, 1.0 - 1e-6)
    g = (torch.zeros(GAMES, A) if greedy else -torch.log(-torch.log(u))).to(DEV, torch.float32).contiguous()
    hidden = torch.zeros((GAMES, tree.slots_per_game, 64), dtype=torch.float32, device=DEV)
    with torch.no_grad():
        s0, logits, v0 = net32.initial_inference(obs)
        hidden[:, 0] = s0
        v0 = inverse_value_transform(v0) if vt else v0
    tree.init_roots(torch.softmax(logits, dim=1).contiguous())
    action, pi, trace = tree.search_gumbel(hidden, n_sims, g, trace=True)
    tree.check()
    nodes, top = tree.nodes()
    _, _, vmin, vmax = (x.cpu().numpy().copy() for x in tree.root_stats())
    trace = {k: v.cpu().numpy() for k, v in trace.items()}
    got = {'nodes': nodes, 'top': top, 'lo': vmin, 'hi': vmax, 'trace': trace, 'action': action.cpu().numpy().copy(),
           'pi': pi.cpu().numpy().copy(), 'plan': tree.search_plan(False), 'root_value32': v0.cpu().numpy(), 'g': g.cpu().numpy()}
    tree.close()
    v_hat = nodes['pad'].view(np.float32)
    ref = twin.gumbel_search_reference(nodes['prior'][:, 1:1 + A], v_hat[:, 0], got['g'], trace['reward'], trace['probs'], trace['value'],
                                       twin.considered_visits(min(m, A), n_sims), tree.discount)
    _runs[case] = (got, ref, v_hat)
    return _runs[case]


@pytest.mark.parametrize('case', CASES)
def test_the_trees_the_moves_and_the_targets_are_the_twins(case):
    A, m, n_sims, gpw, vt, greedy, in_lds = case
    got, ref, v_hat = run(case)
    assert got['plan'] == dict(got['plan'], games_per_workgroup=gpw, tree_in_lds=in_lds), got['plan']
    assert np.abs(v_hat[:, 0] - got['root_value32']).max() <= 1e-5 * max(1.0, np.abs(got['root_value32']).max())   # the kernel's own root prediction
    keep = ref['min_gap'] >= 1e-9
    print('A=%d m=%d n_sims=%d gpw=%d: smallest decision gap %.3e, %d of %d games compared' % (A, m, n_sims, gpw, ref['min_gap'].min(), keep.sum(), GAMES))
    assert keep.sum() >= GAMES - 1
    nodes, trace = got['nodes'], got['trace']
    for gi in np.flatnonzero(keep):
        used = slice(0, int(ref['top'][gi]))
        assert got['top'][gi] == ref['top'][gi] == 1 + A * (n_sims + 1)
        for name in ('N', 'first_child', 'value_sum', 'prior', 'reward'):
            assert np.array_equal(nodes[name][gi, used], ref[name][gi, used]), (gi, name)
        assert v_hat[gi, used].tobytes() == ref['v_hat'][gi, used].tobytes(), gi
        assert got['lo'][gi] == ref['lo'][gi] and got['hi'][gi] == ref['hi'][gi], gi
        for name, key in (('parent', 'parent'), ('action', 'edge'), ('leaf', 'leaf')):
            assert np.array_equal(trace[name][:, gi], ref[key][:, gi]), (gi, name)
        assert got['action'][gi] == ref['action'][gi] and ref['most_visited'][gi, got['action'][gi]], gi
        root_n = nodes['N'][gi, 1:1 + A]
        assert np.array_equal(root_n == root_n.max(), ref['most_visited'][gi]) and root_n.sum() == n_sims, gi
    err = np.abs(got['pi'][keep].astype(np.float64) - ref['pi'][keep].astype(np.float32).astype(np.float64)).max()
    print('pi\': largest distance from the twin\'s float32 %.3e' % err)
    assert err <= 1.2e-7
    assert np.abs(got['pi'].astype(np.float64).sum(axis=1) - 1.0).max() <= (A + 1) * 2.0 ** -24
    if n_sims == 1:   # the single visited action is the arg-max of g + logit (sigma of the unvisited children is one constant)
        with np.errstate(divide='ignore'):
            first = np.array([twin.pick((got['g'][gi].astype(np.float64) + np.log(nodes['prior'][gi, 1:1 + A])).tolist())[0] for gi in range(GAMES)])
        assert np.array_equal(trace['action'][0][keep], first[keep]) and np.array_equal(got['action'][keep], first[keep])
    if m == 1:        # one considered action: every simulation goes through it
        assert (nodes['N'][:, 1:1 + A].max(axis=1) == n_sims).all()


def test_refusals_name_their_reason():
    from rlzero_amd import _hip
    from rlzero_amd.muzero.tree import MuZeroTree
    tree = MuZeroTree(GAMES, 3, 16, device=DEV)
    cv = twin.considered_visits(3, 16)

    def refused(rc, reason):
        assert rc != _hip.OK and reason in (tree.lib.rz_last_error() or b'').decode(), (tree.lib.rz_last_error(), reason)

    ptr = ctypes.c_void_p(cv.ctypes.data)
    refused(tree.lib.rz_mz_set_gumbel(tree.handle, 3, 50.0, 1.0, ptr, 15), 'must hold n_sims = 16 entries')
    refused(tree.lib.rz_mz_set_gumbel(tree.handle, 3, -1.0, 1.0, ptr, 16), 'finite and >= 0')
    refused(tree.lib.rz_mz_set_gumbel(tree.handle, 3, 50.0, float('nan'), ptr, 16), 'finite and >= 0')
    g = torch.zeros((GAMES, 3), dtype=torch.float32, device=DEV)
    hidden = torch.zeros((GAMES, tree.slots_per_game, 64), dtype=torch.float32, device=DEV)
    with pytest.raises(_hip.HipError, match='set_gumbel first'):
        tree.search_gumbel(hidden, 16, g)
    tree.set_gumbel(3)
    refused(tree.lib.rz_mz_play_cartpole(tree.handle, None, 16, 1, None, None), 'whole moves keep the pUCT rule')
    tree.load_model(copy_net(rolled_net(3, 0), torch.float32, DEV))
    with pytest.raises(_hip.HipError, match='schedule of n_sims = 16'):
        tree.search_gumbel(hidden, 8, g)
    tree.set_gumbel(0)   # off: whole moves are judged by their own checks again
    refused(tree.lib.rz_mz_play_cartpole(tree.handle, None, 16, 1, None, None), 'rz_mz_load_representation')
    tree.close()
    # MuZeroSelfPlay(search='gumbel') where the fused search cannot serve it: a ValueError that names the reason
    from rlzero_amd.muzero import MuZeroNet, MuZeroSelfPlay
    env = mz_env.make_env('acrobot')
    net = mz_env.make_net(env.obs_dim, env.n_actions)
    for kw, reason in ((dict(fused=False), 'fused=False was given'), (dict(fused_moves=True), 'whole moves keep the pUCT rule')):
        with pytest.raises(ValueError, match=reason):
            MuZeroSelfPlay(net, env, n_sims=5, search='gumbel', **kw)
    with pytest.raises(ValueError, match='does not serve this model'):
        MuZeroSelfPlay(MuZeroNet(env.obs_dim, env.n_actions, hidden=32).to(DEV), env, n_sims=5, search='gumbel')
    with pytest.raises(ValueError, match="'puct' or 'gumbel'"):
        MuZeroSelfPlay(net, env, n_sims=5, search='uct')


def test_the_device_move_takes_the_searchs_action_and_records_pi():
    """k_mz_env_move<EnvAcrobot, GUMBEL> behind ``search_gumbel``, 40 environments with a 12-step limit, half of them one step before
    it: the record holds the observation before the move, the search's action, the step's reward, pi' widened to doubles, value_sum / N
    of the root and done; the environment is the one a host-driven ``step`` with the same actions leaves; finished episodes are handed
    over to the arena."""
    from rlzero_amd.muzero import AcrobotBatch
    from rlzero_amd.muzero.tree import MuZeroTree
    A, D, n_sims, t = 3, 6, 5, 20
    net32 = copy_net(rolled_net(A, 0), torch.float32, DEV).eval()
    envs = [AcrobotBatch(GAMES, DEV, seed=4, max_episode_steps=12) for _ in range(2)]
    warm = torch.arange(GAMES, device=DEV) % 3
    for env in envs:
        for _ in range(3):
            env.step(warm)
        env.steps[GAMES // 2:] = 11
    env, host = envs
    before = env.observe()
    tree = MuZeroTree(GAMES, A, n_sims, device=DEV).set_gumbel(4)
    tree.load_model(net32)
    hidden = torch.zeros((GAMES, tree.slots_per_game, 64), dtype=torch.float32, device=DEV)
    with torch.no_grad():
        s0, logits, _ = net32.initial_inference(before)
        hidden[:, 0] = s0
    tree.init_roots(torch.softmax(logits, dim=1).contiguous())
    g = -torch.log(-torch.log(torch.rand(GAMES, A, generator=torch.Generator().manual_seed(2)).clamp_(1e-6, 1.0 - 1e-6))).to(DEV)
    action, pi = tree.search_gumbel(hidden, n_sims, g.contiguous())
    kw = dict(device=DEV)
    row = D + 4 + A
    ring, ep_start = torch.zeros((GAMES, 16, row), dtype=torch.float64, **kw), torch.full((GAMES, ), t - 3, dtype=torch.int64, **kw)
    arena, counters = torch.full((GAMES * 4, row), -7.0, dtype=torch.float64, **kw), torch.zeros(4, dtype=torch.int64, **kw)
    entries, obs = torch.full((GAMES, 4), -7, dtype=torch.int64, **kw), torch.zeros((GAMES, D), dtype=torch.float32, **kw)
    tree.env_move(env, 0, 1.0, (ring, ep_start), t, arena, counters, entries, obs, gumbel=True)
    want_obs, reward, terminated, truncated = host.step(action.long())
    n, vsum, _, _ = tree.root_stats()
    rec = ring[:, t % 16].cpu().numpy()
    done = (terminated | truncated).cpu().numpy()
    assert done[GAMES // 2:].all() and not done.all()
    assert np.array_equal(rec[:, :D], before.cpu().numpy().astype(np.float64)) and np.array_equal(rec[:, D], action.cpu().numpy())
    assert np.array_equal(rec[:, D + 1], reward.cpu().numpy().astype(np.float64))
    assert np.array_equal(rec[:, D + 2:D + 2 + A], pi.cpu().numpy().astype(np.float64))
    assert np.abs(rec[:, D + 2:D + 2 + A].sum(axis=1) - 1.0).max() <= (A + 1) * 2.0 ** -24
    assert np.array_equal(rec[:, D + 2 + A], (vsum / n.clamp_min(1)).cpu().numpy()) and np.array_equal(rec[:, D + 3 + A], done.astype(np.float64))
    assert torch.equal(obs, want_obs) and torch.equal(env.state, host.state) and torch.equal(env.steps, host.steps)
    assert torch.equal(env.episode_dev, host.episode_dev)
    counters, entries, arena = counters.cpu().numpy(), entries.cpu().numpy(), arena.cpu().numpy()
    assert counters[1] == done.sum() and counters[0] == 4 * done.sum() and counters[2] == 0
    for e in entries[:counters[1]]:   # (environment, end step, length, first arena row): the last row of a run is this move's record
        assert done[e[0]] and e[1] == t + 1 and e[2] == 4 and np.array_equal(arena[e[3] + 3], np.append(rec[e[0]][:-1], 1.0))
    tree.check()
    tree.close()


_HOST = {}


def gumbel_host_loop():
    if not _HOST:
        _HOST['run'] = mz_env.play('acrobot', False, search='gumbel')
    return _HOST['run']


@pytest.mark.parametrize('chunk', [5, 7, 30])
def test_device_moves_play_the_host_loops_episodes(chunk):
    """Acrobot, 40 environments, 30 moves of 10 simulations under search='gumbel': device moves in chunks of 5, 7 and 30 hand out the
    host loop's episodes record for record -- observations, actions, rewards, pi', root values -- and leave its environments."""
    want = gumbel_host_loop()
    mz_env.assert_same_run(mz_env.play('acrobot', True, search='gumbel', moves_per_launch=chunk), want)
    pols = np.concatenate([np.frombuffer(e[4], dtype=np.float32) for e in want['episodes']]).reshape(-1, 3)
    assert np.abs(pols.astype(np.float64).sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -24 and (pols.max(axis=1) < 1.0).any()   # pi', not counts


def test_both_buffers_read_the_targets_back_and_the_option_off_is_the_default():
    from rlzero_amd.muzero import MuZeroDeviceReplay, ReplayBuffer
    dev = MuZeroDeviceReplay(6, 3, 128, 12, device=DEV)
    got = mz_env.play('acrobot', True, replay=dev, search='gumbel')
    assert got['episodes'] == gumbel_host_loop()['episodes'] and len(dev) == len(got['episodes'])
    host = ReplayBuffer()
    for ep in got['eps']:
        host.add(ep)
    for kept, ep, mine in zip(dev.read(), got['eps'], host.episodes):   # the hand-over: pi' within one float32 rounding
        assert np.abs(np.asarray(kept.policies, dtype=np.float64) - np.asarray(ep.policies, dtype=np.float64)).max() <= 2.0 ** -24
        assert np.array_equal(mine.policies, ep.policies) and np.array_equal(kept.actions, ep.actions)
        assert np.array_equal(kept.root_values, ep.root_values)
    # search='puct' is the default route: the same run, byte for byte
    mz_env.assert_same_run(mz_env.play('acrobot', True, search='puct'), mz_env.play('acrobot', True))


def test_the_trainer_runs_with_the_gumbel_search(capsys):
    import sys
    sys.path.insert(0, REPO + '/tools')
    import train_muzero
    pipe = train_muzero.main(['--env', 'acrobot', '--max-episode-steps', '12', '--envs', '40', '--sims', '10', '--iterations', '2', '--batch-size', '32',
                              '--updates-per-iteration', '2', '--search', 'gumbel', '--gumbel-considered', '3', '--device-replay',
                              '--fused-learner', '--eval-every', '2', '--eval-envs', '8'])
    out = capsys.readouterr().out
    assert pipe.selfplay.gumbel and pipe.selfplay.device_moves and not pipe.selfplay.gumbel_greedy and pipe._evaluator[0].gumbel_greedy
    assert out.count('batch i:') == 2 and 'eval i:2, episodes:8' in out and len(pipe.buffer) > 0
    assert all(np.isfinite(float(x)) for line in out.splitlines() if line.startswith('batch') for x in [line.split('loss:')[1].split(',')[0]])
    pipe.selfplay.tree.check()
