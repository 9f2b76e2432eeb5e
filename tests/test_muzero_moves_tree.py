"""Whole MuZero moves in one launch (rz_mz_play_cartpole, k_mz_search<TREE_LDS, MOVES = true>) node by node.

The whole-move instantiations have no per-simulation trace, but after a launch of one move every game's complete tree is
in ``MuZeroTree.nodes()`` and every node's state in ``MuZeroSelfPlay.hidden_states()``: tests/mz_unfold.py reads the
simulations back out of the tree (order, parent, action, reward, probabilities, value).  With that the whole-move kernels
take the two strong tests of the f32 route: the CPython restatement of the pseudocode fed the device's own numbers, bit for
bit, and the network against a float64 reference, node by node.  Placements (asserted through ``search_plan``): trees in
LDS (50 simulations), trees in HBM (64 simulations: k_mz_search<false, true>), 8 games per workgroup (half-filled tiles).
G = 40 games is ragged: two workgroups of 16 and half of a third."""
import copy

import numpy as np
import pytest

from mz_unfold import slot_of_path, unfold
from oracle import muzero_ref as ref

G = 40
# case -> (n_sims, games per workgroup asked for (0 = auto), games per workgroup planned, trees in LDS)
PLACEMENTS = {'P1': (50, 0, 16, True), 'P2': (64, 0, 16, False), 'P3': (64, 8, 8, True)}


def _hexf(x):
    return float(x).hex()


class _BareEnv(object):
    """What MuZeroSelfPlay.search needs of an environment (no stepping): sizes, device, observations."""
    max_episode_steps = 500

    def __init__(self, n_envs, n_actions, obs):
        self.n_envs, self.n_actions, self.device, self._obs = n_envs, n_actions, obs.device, obs

    def observe(self):
        return self._obs


def _net(gain=1.0, seed=7):
    import torch
    from rlzero_amd.muzero import MuZeroNet
    torch.manual_seed(seed)
    net = MuZeroNet().to('cuda:0').eval()
    if gain != 1.0:   # (the weight scales of test_whole_moves_network_on_the_f16_pipe_agrees_with_the_f32_search)
        with torch.no_grad():
            for name, p_ in net.named_parameters():
                if name.split('.')[0] in ('dyn1', 'pre1') and name.endswith('weight'):
                    p_.mul_(gain)
    return net


_MOVES = {}


def _one_whole_move(case, noise, gain=1.0):
    """One whole move of G CartPole environments in one launch, in placement ``case``; everything the device left behind,
    as host arrays (computed once per module and shared: nothing below changes it)."""
    key = (case, noise, gain)
    if key not in _MOVES:
        from rlzero_amd.muzero import CartPoleBatch, MuZeroSelfPlay
        n_sims, gpw, want_gpw, want_lds = PLACEMENTS[case]
        kw = {} if noise else {'root_exploration_fraction': 0.0}
        sp = MuZeroSelfPlay(_net(gain), CartPoleBatch(G, 'cuda:0', seed=3), n_sims=n_sims, seed=9, temperature=1.0, fused=True,
                            fused_moves=True, moves_per_launch=1, **kw)
        sp.tree.set_search_shape(gpw)
        plan = sp.tree.search_plan(whole_moves=True)
        assert plan['games_per_workgroup'] == want_gpw and plan['tree_in_lds'] == want_lds, (case, plan)
        assert 0 < plan['lds_bytes'] <= 80 * 1024   # (two workgroups per CU either way: trees that do not fit stay out of it)
        sp.collect(1)
        nodes, top = sp.tree.nodes()
        ring, ep_start = sp.device_history()
        n, vsum, vmin, vmax = (x.cpu().numpy().copy() for x in sp.tree.root_stats())
        out = dict(n_sims=n_sims, discount=sp.discount, nodes=nodes, top=top, hidden=sp.hidden_states(), record=ring[:, 0].copy(),
                   root_n=n, root_sum=vsum, vmin=vmin, vmax=vmax, net=copy.deepcopy(sp.net).cpu())
        sp.tree.check()
        sp.close()
        _MOVES[key] = out
    return _MOVES[key]


# ------------------------------------------------------------------ a. the decoder on ground truth
@pytest.mark.gpu
@pytest.mark.parametrize('n_actions,n_sims,in_lds', [(2, 30, True), (3, 30, True), (2, 64, False), (6, 50, False)])
def test_unfold_reads_the_traced_simulations_back_out_of_the_device_tree(n_actions, n_sims, in_lds):
    """The f32 fused route HAS a trace: for every game, what ``unfold`` reads out of the final tree equals the traced parent,
    action, leaf, reward, probabilities and value of every simulation, bit for bit -- trees in LDS and in HBM.  This proves
    the instrument on the device before it is trusted on the kernels that have no trace."""
    import torch
    from rlzero_amd.muzero import MuZeroNet, MuZeroSelfPlay
    torch.manual_seed(30 + n_actions)
    n_games = 37
    net = MuZeroNet(n_actions=n_actions).to('cuda:0').eval()
    obs = torch.randn(n_games, 4, device='cuda:0')
    sp = MuZeroSelfPlay(net, _BareEnv(n_games, n_actions, obs), n_sims=n_sims, seed=3, fused=True)
    assert sp.fused and not sp.fused_moves
    plan = sp.tree.search_plan(whole_moves=False)
    assert plan['tree_in_lds'] == in_lds and plan['games_per_workgroup'] == 16, plan
    record = []
    sp.search(obs, add_noise=True, record=record)
    sims = [tuple(x.cpu().numpy() for x in r) for r in record[1:]]
    nodes, top = sp.tree.nodes()
    pri = sp.tree.root_children('prior').cpu().numpy()
    hidden = sp.hidden_states()
    assert hidden.dtype == np.float64 and np.array_equal(hidden, sp.hidden.cpu().numpy().astype(np.float64))
    assert nodes.shape == (n_games, sp.tree.slots_per_game) and (top == 1 + n_actions * (n_sims + 1)).all()
    for g in range(n_games):
        got, root_prior = unfold(nodes[g], top[g], n_actions, sp.discount)
        assert len(got) == n_sims and [_hexf(p) for p in root_prior] == [_hexf(p) for p in pri[g]]
        for e, (parent, action, leaf, reward, probs, value) in zip(got, sims):
            assert (e.parent, e.action, e.slot) == (parent[g], action[g], leaf[g]), (g, e)
            assert e.reward.tobytes() == reward[g].tobytes() and e.value.tobytes() == value[g].tobytes(), (g, e)
            assert e.probs.tobytes() == probs[g].tobytes(), (g, e)
    sp.tree.check()
    sp.close()


# ------------------------------------------------------------------ b. the whole-move tree is the pseudocode's
def _replay(run, g, tamper=None):
    """Game ``g`` of a whole move against the pseudocode: the root expanded with the STORED priors (doubles: no second noise
    step), ``run_mcts`` fed the unfolded network outputs in order -- and asked, simulation by simulation, about the very
    path the device took -- then every node, the MinMaxStats and the move's record compared bit for bit.
    ``tamper(expansions) -> expansions`` changes what the replay is fed (to show that the comparison can fail)."""
    nodes, top, n_sims = run['nodes'][g], int(run['top'][g]), run['n_sims']
    exps, root_prior = unfold(nodes, top, 2, run['discount'])
    assert len(exps) == n_sims and top == 1 + 2 * (n_sims + 1)
    if tamper is not None:
        exps = tamper(exps)
    root = ref.Node(0)
    ref.expand_node(root, None, 0.0, [float(p) for p in root_prior])
    step = [0]

    def model(hidden, action, path):
        e = exps[step[0]]
        assert path == e.path and action == e.action, (g, step[0], path, e.path)   # the device took the same edges
        step[0] += 1
        return None, float(e.reward), [float(p) for p in e.probs], float(e.value)

    stats = ref.run_mcts(ref.MuZeroConfig(num_simulations=n_sims, discount=run['discount']), root, model)
    dump = ref.tree_dump(root)
    assert len(dump) == top
    for path, (n, value_sum, reward, prior) in dump.items():
        nd = nodes[slot_of_path(nodes, path)]
        assert n == nd['N'], (g, path)
        assert (_hexf(value_sum), _hexf(reward), _hexf(prior)) == (_hexf(nd['value_sum']), _hexf(nd['reward']), _hexf(nd['prior'])), (g, path)
    assert root.visit_count == run['root_n'][g] == n_sims and _hexf(root.value_sum) == _hexf(run['root_sum'][g])
    assert _hexf(stats.minimum) == _hexf(run['vmin'][g]) and _hexf(stats.maximum) == _hexf(run['vmax'][g])
    rec = run['record'][g]   # obs (4) | action | reward | visits (2) | root value | done
    assert [int(v) for v in rec[6:8]] == [c.visit_count for c in root.children] and rec[6:8].sum() == n_sims
    assert _hexf(rec[8]) == _hexf(root.value())
    assert root.children[int(rec[4])].visit_count > 0


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(PLACEMENTS))
def test_whole_move_trees_are_the_pseudocodes_bit_for_bit(case):
    """Root noise at its default weight, temperature 1; every game of the ragged batch, every node of its tree.  And the test
    can fail: the replay fed ONE simulation's two probabilities the other way round is refused (a mutation of the test's
    inputs, not of the kernel)."""
    run = _one_whole_move(case, noise=True)
    for g in range(G):
        _replay(run, g)

    def swapped(exps, which):
        e = exps[which]
        assert e.probs[0] != e.probs[1]
        return exps[:which] + [e._replace(probs=e.probs[::-1].copy())] + exps[which + 1:]

    for g, which in ((0, 0), (17, 5), (G - 1, run['n_sims'] - 1)):
        with pytest.raises(AssertionError):
            _replay(run, g, tamper=lambda exps, which=which: swapped(exps, which))


@pytest.mark.gpu
def test_whole_move_root_priors_sum_to_one():
    """The stored root priors (network probabilities mixed with the kernel's Dirichlet draw) sum to 1 within 1e-12, in every
    game of P1, P2 and P3.

    This test found that they did not: the worst |sum - 1| over the 40 games was 5.70e-08 in each of P1, P2 and P3 (the first
    move's roots are the same in all three).  The kernel's softmax is float32 (exp / float32 sum: the two probabilities add up
    to 1 within a float32 ulp, 6e-8) and the two gamma draws were divided by their FLOAT32 sum, so both terms of
    prior * (1 - frac) + noise * frac were off by ~6e-8.  The whole-move kernel now normalises both in fp64 when it expands
    the root, once per move."""
    worst = {}
    for case in sorted(PLACEMENTS):
        pri = _one_whole_move(case, noise=True)['nodes']['prior'][:, 1:3]
        assert (pri > 0).all()
        worst[case] = float(np.max(np.abs(pri.sum(axis=1) - 1.0)))
        print('root prior sums, %s: worst |sum - 1| = %.3e' % (case, worst[case]))
    assert max(worst.values()) <= 1e-12, worst


# ------------------------------------------------------------------ c. the whole-move network against float64
def _units(got, want):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(1.0, np.abs(want))))


def _network_errors(run, decode=None):
    """-> ({quantity: worst error of the kernel}, {quantity: worst error of torch float32}) against ``net.double()`` on the
    CPU, every stage given the inputs the kernel had, in units of max(1, |want|)."""
    import torch
    hidden = run['hidden'] if decode is None else decode(run)
    ref64, ref32 = copy.deepcopy(run['net']).double(), copy.deepcopy(run['net']).float()
    t64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))   # noqa: E731
    softmax = lambda logits: torch.softmax(logits, dim=1).double().numpy()        # noqa: E731
    err = dict(state=0.0, reward=0.0, value=0.0, probs=0.0)
    e32 = dict(err)

    def note(quantity, got, got32, want):
        err[quantity] = max(err[quantity], _units(got, want))
        e32[quantity] = max(e32[quantity], _units(got32, want))

    with torch.no_grad():
        # the root: representation(obs) -> slot 0, softmax(prediction(slot 0)) -> the stored root priors (noise weight 0)
        obs = t64(run['record'][:, :4])   # the record's four float32 values
        s0 = t64(hidden[:, 0])
        note('state', hidden[:, 0], ref32.representation(obs.float()).double().numpy(), ref64.representation(obs).numpy())
        note('probs', run['nodes']['prior'][:, 1:3], softmax(ref32.prediction(s0.float())[0]), softmax(ref64.prediction(s0)[0]))
        # every expansion of every game, as one batch
        gi, parent, action, slot, reward, value, probs = [], [], [], [], [], [], []
        for g in range(G):
            for e in unfold(run['nodes'][g], run['top'][g], 2, run['discount'])[0]:
                gi.append(g)
                parent.append(e.parent)
                action.append(e.action)
                slot.append(e.slot)
                reward.append(e.reward)
                value.append(e.value)
                probs.append(e.probs)
        assert len(gi) == G * run['n_sims']
        gi, parent, slot = np.array(gi), np.array(parent), np.array(slot)
        act = torch.from_numpy(np.array(action, dtype=np.int64))
        sp_, sc = t64(hidden[gi, parent]), t64(hidden[gi, slot])
        nxt, rew = ref64.dynamics(sp_, act)
        nxt32, rew32 = ref32.dynamics(sp_.float(), act)
        note('state', hidden[gi, slot], nxt32.double().numpy(), nxt.numpy())
        note('reward', np.array(reward), rew32.double().numpy(), rew.numpy())
        logits, val = ref64.prediction(sc)
        logits32, val32 = ref32.prediction(sc.float())
        note('value', np.array(value), val32.double().numpy(), val.numpy())
        note('probs', np.array(probs), softmax(logits32), softmax(logits))
    return err, e32


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['P1', 'P2'])
@pytest.mark.parametrize('gain', [1.0, 20.0])
def test_whole_move_network_matches_float64_node_by_node(gain, case):
    """The f16-pipe layers (hi + lo operand pairs, states kept as f16 pieces, min-max scaling by a reciprocal), the initial
    inference on the tiles and the heads against ``net.double()`` on the CPU: root state and root priors, and for EVERY
    expansion dynamics(decoded parent state, action) -> decoded child state and reward, prediction(decoded child state) ->
    value and probabilities.  Limit per quantity: max(1e-5, 8 x e32), e32 = what the same MuZeroNet in torch float32 is off by
    on the same inputs (1e-5 is the f32 route's bound; 8 = operand pieces of 2^-22 instead of 2^-24, two per product, lo x lo
    dropped).  The yardstick is the reference's own float32 arithmetic, never a kernel.

    MEASURED, MI355X, worst error in units of max(1, |want|), kernel / torch float32 (e32):
      gain  1, P1 (LDS): state 3.24e-07 / 2.89e-07  reward 2.06e-08 / 2.19e-08  value 6.20e-08 / 8.81e-08  probs 7.02e-08 / 6.68e-08
      gain  1, P2 (HBM): state 3.24e-07 / 2.89e-07  reward 2.06e-08 / 2.19e-08  value 6.20e-08 / 8.81e-08  probs 7.15e-08 / 6.68e-08
      gain 20, P1 (LDS): state 3.97e-07 / 3.40e-07  reward 3.49e-07 / 3.83e-07  value 9.03e-07 / 9.66e-07  probs 1.04e-07 / 1.42e-07
      gain 20, P2 (HBM): state 3.97e-07 / 3.40e-07  reward 3.96e-07 / 3.83e-07  value 9.03e-07 / 9.66e-07  probs 1.04e-07 / 1.42e-07
    (every limit is therefore the 1e-5 floor: the f16-pipe route is as close to float64 as torch's float32 is)

    And the test can fail: the states decoded from their hi halves alone (a mutation of the test's inputs) miss the limit.
    (Swapping the two halves cannot: the decoding is their SUM.)"""
    run = _one_whole_move(case, noise=False, gain=gain)
    err, e32 = _network_errors(run)
    print('network vs float64, gain %g, %s: ' % (gain, case) +
          '  '.join('%s %.2e / %.2e' % (k, err[k], e32[k]) for k in ('state', 'reward', 'value', 'probs')))
    for k in err:
        assert err[k] <= max(1e-5, 8.0 * e32[k]), (k, err[k], e32[k])

    def hi_only(run_):   # hidden_states() is (hi + lo) / 16: drop lo by rounding the state's 16-fold to f16
        return (run_['hidden'] * 16.0).astype(np.float16).astype(np.float64) / 16.0

    bad, bad32 = _network_errors(run, decode=hi_only)
    assert any(bad[k] > max(1e-5, 8.0 * bad32[k]) for k in bad), (bad, bad32)


# ------------------------------------------------------------------ d. launch splits and workgroup shapes
def _play_12(n_sims, moves_per_launch, collects, gpw):
    from rlzero_amd.muzero import CartPoleBatch, MuZeroSelfPlay
    env = CartPoleBatch(G, 'cuda:0', seed=11)
    sp = MuZeroSelfPlay(_net(), env, n_sims=n_sims, seed=4, temperature=1.0, fused=True, fused_moves=True,
                        moves_per_launch=moves_per_launch)
    sp.tree.set_search_shape(gpw)
    plan = sp.tree.search_plan(whole_moves=True)
    assert plan['games_per_workgroup'] == gpw
    episodes = []
    for n in collects:
        episodes.extend(sp.collect(n))
    assert sp._t == 12
    ring, ep_start = sp.device_history()
    nodes, top = sp.tree.nodes()
    out = {
        'ring': np.ascontiguousarray(ring[:, :12]).view(np.uint64).tobytes(),
        'ep_start': ep_start.tobytes(),
        'state': env.state.cpu().numpy().view(np.uint64).tobytes(),
        'steps': env.steps.cpu().numpy().tobytes(),
        'episode': env.episode.tobytes(),
        'episodes': [tuple(np.asarray(getattr(ep, f)).tobytes() for f in ('obs', 'actions', 'rewards', 'policies', 'root_values'))
                     for ep in episodes],
        'top': top.tobytes(),
        'trees': [nodes[g, :top[g]].tobytes() for g in range(G)],
    }
    assert (top == 1 + 2 * (n_sims + 1)).all()
    sp.tree.check()
    sp.close()
    return out, plan['tree_in_lds'], len(episodes)


@pytest.mark.gpu
@pytest.mark.parametrize('n_sims', [20, 64])
def test_whole_moves_do_not_depend_on_launch_splits_or_workgroup_shape(n_sims):
    """12 moves of 40 environments (noise on, temperature 1) as 12 launches of one move, as 5 + 5 + 2, as one launch of 12 and
    as 7 + 5, with 16, 8 and 4 games per workgroup: the environment state, the episode starts and the noise keys cross a launch
    boundary through HBM and a move boundary through LDS, and a game is a column of another workgroup's tiles in every shape.
    Every run must leave the same records, environments, finished episodes and final trees, bit for bit.  (At 64 simulations
    16 games per workgroup keep their trees in HBM, 8 and 4 in LDS: the two tree codes against each other as well.)"""
    base, placements, ended = None, set(), 0
    for gpw in (16, 8, 4):
        for moves_per_launch, collects in ((1, (12, )), (5, (12, )), (12, (12, )), (12, (7, 5))):
            got, in_lds, ended = _play_12(n_sims, moves_per_launch, collects, gpw)
            placements.add((gpw, in_lds))
            if base is None:
                base = got
                continue
            for k in base:
                assert got[k] == base[k], (k, gpw, moves_per_launch, collects)
    assert placements == ({(16, True), (8, True), (4, True)} if n_sims == 20 else {(16, False), (8, True), (4, True)})
    print('%d simulations: %d episodes ended within the 12 moves' % (n_sims, ended))
    assert ended > 0   # (the comparison of finished episodes -- the arena's path -- is not an empty one)
