"""Whole MuZero moves in one launch for Acrobot-v1 (rz_mz_play_env, k_mz_search<TREE_LDS, MOVES = true, EnvAcrobot>): three actions,
six observations, reward -1 per step, the time limit an argument.  tests/test_muzero_moves_tree.py at A = 3 and D = 6, and
tests/test_mz_env_gpu.py's checks of a move on the records of whole moves.

G = 40 environments everywhere (but the one case of 16 that asks for more than 64 KB of LDS): two workgroups of 16 and half of a third.  Placements, by the plan's own formula for three actions
(asserted through ``search_plan(whole_moves=True)``): 30 simulations -> 16 games per workgroup, trees in LDS; 50 simulations -> 16,
trees in HBM; 50 simulations with 8 asked for -> 8, trees in LDS.  The yardsticks: oracle/muzero_ref.py fed the unfolded expansions
(tests/mz_unfold.py), ``net.double()`` on the CPU, tests/acrobot_twin.py set to the device's own state, tests/device_streams.py."""
import copy
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import acrobot_twin as twin
import device_streams as ds
from mz_unfold import slot_of_path, unfold
from oracle import muzero_ref as ref
from test_mz_replay_host import every_position, same_bits

pytestmark = pytest.mark.gpu

G = 40
DEV = 'cuda:0'
D, A = 6, 3
ROW = D + 4 + A
BOUND = 1e-9   # tests/test_mz_env_gpu.py: the environment against the twin, and its rule for decisions closer than that
# case -> (n_sims, games per workgroup asked for (0 = auto), games per workgroup planned, trees in LDS)
PLACEMENTS = {'P1': (30, 0, 16, True), 'P2': (50, 0, 16, False), 'P3': (50, 8, 8, True)}


def _hexf(x):
    return float(x).hex()


@pytest.fixture(scope='module', autouse=True)
def stream_pool_left_as_found():
    """torch hands out ``torch.cuda.Stream()`` from a fixed pool, round robin, and every whole-move player here draws one (its copy
    stream): about fifty draws.  Which pool streams a LATER test of the same process draws decides which hardware queues its streams
    share, and tests/test_trace.py's overlap figures of AlphaZero's four lanes move with that (measured at 4 hardware queues: CU time
    under trunk workgroups 0.31, 0.44, 0.34, 0.77 with 0, 1, 2, 3 streams used before it in the process; its bound is 0.3).  So this
    module leaves the pool's position where it found it: whatever runs behind it draws the streams it drew before this file existed."""
    import torch
    if not torch.cuda.is_available():
        yield
        return
    mark = torch.cuda.Stream(device=DEV).cuda_stream   # position p -> p + 1
    yield

    def draws_until_mark():
        for n in range(1, 1025):
            if torch.cuda.Stream(device=DEV).cuda_stream == mark:
                return n
        raise AssertionError('torch.cuda.Stream() did not come back to a stream it handed out: no round-robin pool?')
    draws_until_mark()            # the pool is behind the mark again: p + 1
    size = draws_until_mark()     # one turn of the pool: its size, and p + 1 again
    for _ in range(size - 1):     # p
        torch.cuda.Stream(device=DEV)


def make_net(gain=1.0, seed=7, obs_dim=D, n_actions=A):
    import torch
    from rlzero_amd.muzero import MuZeroNet
    torch.manual_seed(seed)
    net = MuZeroNet(obs_dim, n_actions).to(DEV).eval()
    if gain != 1.0:
        with torch.no_grad():
            for name, p_ in net.named_parameters():
                if name.split('.')[0] in ('dyn1', 'pre1') and name.endswith('weight'):
                    p_.mul_(gain)
    return net


def whole_moves(env, **kw):
    """MuZeroSelfPlay on whole moves for ``env`` (the constructor the parent commit refuses for Acrobot)."""
    from rlzero_amd.muzero import MuZeroSelfPlay
    net = kw.pop('net', None) or make_net()
    sp = MuZeroSelfPlay(net, env, fused=True, fused_moves=True, **kw)
    assert sp.fused_moves and not sp.device_moves
    return sp


_MOVES = {}


def _one_whole_move(case, noise, gain=1.0):
    """One whole move of G Acrobot environments in one launch, in placement ``case``; everything the device left behind, as host
    arrays (computed once per module and shared: nothing below changes it)."""
    key = (case, noise, gain)
    if key not in _MOVES:
        from rlzero_amd.muzero import AcrobotBatch
        n_sims, gpw, want_gpw, want_lds = PLACEMENTS[case]
        kw = {} if noise else {'root_exploration_fraction': 0.0}
        sp = whole_moves(AcrobotBatch(G, DEV, seed=3), net=make_net(gain), n_sims=n_sims, seed=9, temperature=1.0, moves_per_launch=1, **kw)
        sp.tree.set_search_shape(gpw)
        plan = sp.tree.search_plan(whole_moves=True)
        assert plan['games_per_workgroup'] == want_gpw and plan['tree_in_lds'] == want_lds, (case, plan)
        assert 0 < plan['lds_bytes'] <= 80 * 1024
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


# ------------------------------------------------------------------ 1. placements
@pytest.mark.parametrize('case', sorted(PLACEMENTS))
def test_three_action_placements(case):
    """The plan for the engine's action count: 30 simulations in LDS, 50 in HBM, 50 at 8 games per workgroup in LDS -- and each is the
    instantiation a whole move then runs (``_one_whole_move`` asserts the same plan before its launch)."""
    run = _one_whole_move(case, noise=True)
    assert (run['top'] == 1 + A * (run['n_sims'] + 1)).all() and (run['root_n'] == run['n_sims']).all()


def test_trees_in_lds_past_64_kb_without_the_value_transform():
    """Acrobot whole moves WITHOUT the value transform where the launch asks for more than 64 KB of dynamic LDS with the trees in it:
    the two instantiations the dynamic-LDS attribute was not set for until rz_mz_load_model began to walk the table the launcher
    reads.  16 environments (one full workgroup), 2 moves in one launch, the fewest simulations for which the plan says so -- found by
    asking the plan, not by the formula.  Then what the placements above assert: full trees, every root visited n_sims times, and every
    tree of the last move the pseudocode's bit for bit with its record."""
    from rlzero_amd.muzero import AcrobotBatch, MuZeroTree
    n_envs, n_sims = 16, None
    for n in range(1, 65):
        probe = MuZeroTree(n_envs, A, n, device=DEV)
        plan = probe.search_plan(whole_moves=True)
        probe.close()
        if plan['tree_in_lds'] and plan['lds_bytes'] > 65536:
            n_sims = n
            break
    assert n_sims is not None, 'no simulation count keeps 16 three-action trees in LDS past 64 KB'
    sp = whole_moves(AcrobotBatch(n_envs, DEV, seed=3), n_sims=n_sims, seed=9, temperature=1.0, moves_per_launch=2)
    plan = sp.tree.search_plan(whole_moves=True)
    print('trees in LDS past 64 KB: %d simulations, plan %r' % (n_sims, plan))
    assert plan['games_per_workgroup'] == 16 and plan['tree_in_lds'] and plan['lds_bytes'] > 65536
    assert not sp.tree.value_transform and not getattr(sp.net, 'value_transform', False)
    sp.collect(2)
    nodes, top = sp.tree.nodes()
    ring, _ = sp.device_history()
    n, vsum, vmin, vmax = (x.cpu().numpy().copy() for x in sp.tree.root_stats())
    run = dict(n_sims=n_sims, discount=sp.discount, nodes=nodes, top=top, record=ring[:, 1].copy(), root_n=n, root_sum=vsum, vmin=vmin, vmax=vmax)
    sp.tree.check()
    sp.close()
    assert (top == 1 + A * (n_sims + 1)).all() and (n == n_sims).all()
    assert (ring[:, :2, D + 2:D + 2 + A].sum(axis=2) == n_sims).all()   # both moves' visit counts
    for g in range(n_envs):
        _replay(run, g)


# ------------------------------------------------------------------ 2. the tree is the pseudocode's
def _replay(run, g, tamper=None):
    """Game ``g`` of a whole move against the pseudocode (tests/test_muzero_moves_tree.py ``_replay`` at three actions)."""
    nodes, top, n_sims = run['nodes'][g], int(run['top'][g]), run['n_sims']
    exps, root_prior = unfold(nodes, top, A, run['discount'])
    assert len(exps) == n_sims and top == 1 + A * (n_sims + 1)
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
    rec = run['record'][g]   # obs (6) | action | reward | visits (3) | root value | done
    assert [int(v) for v in rec[D + 2:D + 2 + A]] == [c.visit_count for c in root.children] and rec[D + 2:D + 2 + A].sum() == n_sims
    assert _hexf(rec[D + 2 + A]) == _hexf(root.value())
    assert root.children[int(rec[D])].visit_count > 0


@pytest.mark.parametrize('case', sorted(PLACEMENTS))
def test_whole_move_trees_are_the_pseudocodes_bit_for_bit(case):
    """Root noise at its default weight, temperature 1; every game, every node: N, value_sum, reward, prior, the MinMax bounds, the
    root's N and value_sum, the record's three visit counts and root value.  And the test can fail: the replay fed ONE simulation's
    three probabilities rotated by one is refused.  The root priors sum to 1 within 1e-12 (the bound and the reason of
    test_whole_move_root_priors_sum_to_one: both distributions are normalised in fp64 at the root)."""
    run = _one_whole_move(case, noise=True)
    for g in range(G):
        _replay(run, g)

    def rotated(exps, which):
        e = exps[which]
        assert len(set(e.probs.tolist())) == A
        return exps[:which] + [e._replace(probs=np.roll(e.probs, 1).copy())] + exps[which + 1:]

    for g, which in ((0, 0), (17, 5), (G - 1, run['n_sims'] - 1)):
        with pytest.raises(AssertionError):
            _replay(run, g, tamper=lambda exps, which=which: rotated(exps, which))
    pri = run['nodes']['prior'][:, 1:1 + A]
    assert (pri > 0).all()
    worst = float(np.max(np.abs(pri.sum(axis=1) - 1.0)))
    print('root prior sums, %s: worst |sum - 1| = %.3e' % (case, worst))
    assert worst <= 1e-12


# ------------------------------------------------------------------ 3. the network against float64
def _units(got, want):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(1.0, np.abs(want))))


def _network_errors(run, decode=None):
    """tests/test_muzero_moves_tree.py ``_network_errors`` at A = 3 and D = 6 -> ({quantity: worst error of the kernel}, {quantity:
    worst error of torch float32}) against ``net.double()`` on the CPU, every stage given the inputs the kernel had, in units of
    max(1, |want|)."""
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
        obs = t64(run['record'][:, :D])   # the record's six float32 values
        s0 = t64(hidden[:, 0])
        note('state', hidden[:, 0], ref32.representation(obs.float()).double().numpy(), ref64.representation(obs).numpy())
        note('probs', run['nodes']['prior'][:, 1:1 + A], softmax(ref32.prediction(s0.float())[0]), softmax(ref64.prediction(s0)[0]))
        gi, parent, action, slot, reward, value, probs = [], [], [], [], [], [], []
        for g in range(G):
            for e in unfold(run['nodes'][g], run['top'][g], A, run['discount'])[0]:
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


@pytest.mark.parametrize('case', ['P1', 'P2'])
@pytest.mark.parametrize('gain', [1.0, 20.0])
def test_whole_move_network_matches_float64_node_by_node(gain, case):
    """The f16-pipe layers with a third action column of dyn1, the initial inference from six observation rows and the heads over
    three actions against ``net.double()`` on the CPU: root state, root priors, and for EVERY expansion the state, reward, value and
    probabilities.  Limit per quantity: max(1e-5, 8 x e32), e32 = torch float32's error on the same inputs (the project's limit for
    the f16-pipe route, tests/test_muzero_moves_tree.py).  A wrong action column, a one-hot of the wrong action or a softmax over the
    wrong count miss it by orders of magnitude.

    MEASURED, MI355X, worst error in units of max(1, |want|), kernel / torch float32 (e32) (profiles/mz_whole_env/errors.txt):
      gain  1, P1 (LDS, 30 simulations): state 3.08e-07 / 2.36e-07  reward 3.38e-08 / 3.17e-08  value 5.38e-08 / 6.72e-08  probs 4.21e-08 / 5.35e-08
      gain  1, P2 (HBM, 50 simulations): state 3.08e-07 / 2.56e-07  reward 3.38e-08 / 3.17e-08  value 5.38e-08 / 6.72e-08  probs 4.41e-08 / 5.35e-08
      gain 20, P1 (LDS, 30 simulations): state 3.33e-07 / 3.04e-07  reward 4.85e-07 / 5.10e-07  value 4.78e-07 / 5.51e-07  probs 1.53e-07 / 1.36e-07
      gain 20, P2 (HBM, 50 simulations): state 3.33e-07 / 3.04e-07  reward 4.85e-07 / 5.10e-07  value 4.78e-07 / 5.51e-07  probs 1.53e-07 / 1.36e-07
    (every limit is therefore the 1e-5 floor: with a third action the f16-pipe route is as close to float64 as torch's float32 is)

    And the test can fail: the states decoded from their hi halves alone (a mutation of the test's inputs) miss the limit."""
    run = _one_whole_move(case, noise=False, gain=gain)
    met = {e.action for g in range(G) for e in unfold(run['nodes'][g], run['top'][g], A, run['discount'])[0]}
    assert len(met) >= 2 and (gain != 1.0 or met == set(range(A))), met   # (at gain 1 every column of dyn1's one-hot rows is met)
    err, e32 = _network_errors(run)
    print('network vs float64, gain %g, %s: ' % (gain, case) +
          '  '.join('%s %.2e / %.2e' % (k, err[k], e32[k]) for k in ('state', 'reward', 'value', 'probs')))
    for k in err:
        assert err[k] <= max(1e-5, 8.0 * e32[k]), (k, err[k], e32[k])

    def hi_only(run_):   # hidden_states() is (hi + lo) / 16: drop lo by rounding the state's 16-fold to f16
        return (run_['hidden'] * 16.0).astype(np.float16).astype(np.float64) / 16.0

    bad, bad32 = _network_errors(run, decode=hi_only)
    assert any(bad[k] > max(1e-5, 8.0 * bad32[k]) for k in bad), (bad, bad32)


# ------------------------------------------------------------------ 4. the move
GOAL_STATE = (3.0, 0.0, 0.0, 0.0)   # both links almost straight up, at rest: the tip stays above the line whatever the torque
GOAL_ENVS = (0, 7, 16, 23, 39)


def _six_moves(temperature, moves_per_launch):
    """Six moves of G environments, five of them set to GOAL_STATE; -> records [G, 6, ROW], and, when the moves are six launches,
    the device's own (state, steps, episode) before every move and after the last."""
    from rlzero_amd.muzero import AcrobotBatch
    env = AcrobotBatch(G, DEV, seed=21)
    states = env.state.cpu().numpy()
    mask = np.zeros(G, dtype=bool)
    mask[list(GOAL_ENVS)] = True
    states[mask] = GOAL_STATE
    env.set_states(states, mask)
    sp = whole_moves(env, n_sims=12, seed=13, temperature=temperature, moves_per_launch=moves_per_launch)
    seen = []
    for _ in range(6 // moves_per_launch):
        seen.append((env.state.cpu().numpy(), env.steps.cpu().numpy(), env.episode.copy()))
        sp.collect(moves_per_launch)
    seen.append((env.state.cpu().numpy(), env.steps.cpu().numpy(), env.episode.copy()))
    ring, ep_start = sp.device_history()
    sp.tree.check()
    sp.close()
    return ring[:, :6].copy(), seen, ep_start


@pytest.mark.parametrize('temperature', [1.0, 0.0])
def test_whole_move_writes_every_word_of_the_record(temperature):
    """Six moves of ONE launch, every word of every record.  The device's own state before each move comes from the same run played
    as six launches of one move, whose records and final environments are first shown to be the one launch's, bit for bit."""
    from rlzero_amd.muzero import acrobot_initial_states
    for a in range(A):   # the crafted states reach the goal under any torque, clear of every decision (the twin, on the CPU)
        new, _, r, t1, _ = twin.step(GOAL_STATE, 0, a)
        assert t1 and r == 0.0 and twin.decision_margin(GOAL_STATE, a) >= 1e-3
    rec, seen1, ep_start = _six_moves(temperature, 6)
    rec6, seen, ep_start6 = _six_moves(temperature, 1)
    assert same_bits(rec, rec6) and np.array_equal(ep_start, ep_start6)
    for x, y in zip(seen1[-1], seen[-1]):
        assert same_bits(x, y)
    inv_t = 1.0 / temperature if temperature > 0 else 0.0
    g = np.arange(G)
    left_out, n_done, n_goal = 0, 0, 0
    for t in range(6):
        before, steps_before, episode_before = seen[t]
        after, steps_after, episode_after = seen[t + 1]
        r = rec[:, t]
        visits = r[:, D + 2:D + 2 + A].astype(np.int64)
        assert (visits.sum(axis=1) == 12).all() and same_bits(r[:, D + 2:D + 2 + A], visits.astype(np.float64))
        want_action, gap = ds.muzero_action(13, g, episode_before, steps_before, visits, inv_t)
        keep = ~((gap < 1e-9) & (inv_t != 1.0))   # (the near-tie rule of tests/device_streams.py's users: never met at T = 1 and T = 0)
        assert keep.all() and np.array_equal(r[:, D].astype(np.int64), want_action)
        if temperature > 0 and t == 0:
            assert (r[:, D] != np.argmax(visits, axis=1)).any()   # (a draw, not the arg-max)
        assert np.isfinite(r[:, D + 2 + A]).all() and (r[:, D + 2 + A] != 0.0).any()
        for i in range(G):
            st, a = tuple(before[i]), int(r[i, D])
            if twin.decision_margin(st, a) < BOUND:
                left_out += 1
                continue
            assert np.abs(r[i, :D] - twin.observe(st).astype(np.float64)).max() <= BOUND
            assert same_bits(r[i, :D], r[i, :D].astype(np.float32).astype(np.float64))
            new, new_steps, reward, t1, t2 = twin.step(st, int(steps_before[i]), a, 500)
            assert r[i, D + 1] == reward and r[i, D + 3 + A] == float(t1 or t2), (t, i)
            if t == 0 and i in GOAL_ENVS:
                n_goal += 1
                assert t1 and r[i, D + 1] == 0.0 and r[i, D + 3 + A] == 1.0
            if t1 or t2:
                n_done += 1
                assert same_bits(after[i], acrobot_initial_states(21, i, episode_before[i] + 1)[0])
                assert steps_after[i] == 0 and episode_after[i] == episode_before[i] + 1
            else:
                assert np.abs(after[i] - np.array(new)).max() <= BOUND, (t, i)
                assert steps_after[i] == new_steps and episode_after[i] == episode_before[i]
    print('T = %g: 6 moves of %d environments, %d left out, %d episodes ended (%d at the goal from the crafted states)'
          % (temperature, G, left_out, n_done, n_goal))
    assert left_out == 0 and n_goal == len(GOAL_ENVS) >= 4 and n_done >= n_goal
    assert (ep_start[list(GOAL_ENVS)] >= 1).all()


def test_whole_move_root_noise_for_three_actions_is_the_restatement():
    """root_exploration_fraction = 1: the stored root priors behind a launch are muzero_eta for three actions of (episode, steps)
    before the launch's last move -- the tolerance rule and the margin filter of test_whole_move_root_noise_is_the_restatement
    (tests/test_noise_streams_gpu.py: MARGIN 1e-4, at most a tenth left out, four times the restatement's own float32 spread)."""
    from rlzero_amd.muzero import AcrobotBatch
    seed, alpha, chunk, chunks = 9, 0.25, 5, 6
    env = AcrobotBatch(G, DEV, seed=9, max_episode_steps=12)
    sp = whole_moves(env, n_sims=2, seed=seed, root_dirichlet_alpha=alpha, root_exploration_fraction=1.0, temperature=1.0, moves_per_launch=chunk)
    priors = []
    for _ in range(chunks):
        sp.collect(chunk)
        priors.append(sp.tree.root_children('prior').cpu().numpy().copy())
    ring, _ = sp.device_history()
    n_moves = chunk * chunks
    assert ring.shape[1] >= n_moves
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
        want, margin, _ = ds.muzero_eta(seed, g, episode[t], steps[t], A, alpha)
        want32, _, _ = ds.muzero_eta(seed, g, episode[t], steps[t], A, alpha, dtype=np.float32)
        assert pri.dtype == np.float64 and pri.shape == want.shape
        assert np.max(np.abs(pri.sum(axis=1) - 1.0)) <= 1e-12 and (pri >= 0).all()
        keep = margin.min(axis=1) >= 1e-4
        t_rel = 4.0 * ds.relative_spread(want[keep], want32[keep])
        rel = np.abs(pri[keep] - want[keep]) / want[keep]
        assert t_rel < 1e-2 and (rel <= t_rel).all(), (i, float(rel.max()), t_rel)
        left_out, total, later, worst = left_out + int((~keep).sum()), total + G, later + int((episode[t][keep] > 0).sum()), max(worst, float(rel.max()))
    print('whole-move root noise, 3 actions: %d moves, %d left out, %d in a later episode, worst relative difference %.3e' % (total, left_out, later, worst))
    assert left_out <= 0.10 * total and later >= G
    sp.tree.check()
    sp.close()


# ------------------------------------------------------------------ 5. launch splits and workgroup shapes
def episode_bytes(eps):
    return [tuple(np.asarray(getattr(ep, f)).tobytes() for f in ('obs', 'actions', 'rewards', 'policies', 'root_values')) for ep in eps]


def _play_12(n_sims, moves_per_launch, collects, gpw, arena_rows=None, replay=None):
    """12 moves with a time limit of 5: every environment ends two episodes at the limit, through the arena."""
    from rlzero_amd.muzero import AcrobotBatch
    env = AcrobotBatch(G, DEV, seed=11, max_episode_steps=5)
    sp = whole_moves(env, n_sims=n_sims, seed=4, temperature=1.0, moves_per_launch=moves_per_launch, arena_rows=arena_rows)
    sp.tree.set_search_shape(gpw)
    plan = sp.tree.search_plan(whole_moves=True)
    assert plan['games_per_workgroup'] == (gpw or 16)
    missed = []
    inner = sp._episodes_of_launch

    def spy(buf, replay=None):
        out = inner(buf, replay)
        missed.append(int(buf[1][0].numpy()[2]))
        return out
    sp._episodes_of_launch = spy
    episodes = []
    for n in collects:
        episodes.extend(sp.collect(n, replay=replay))
    assert sp._t == sum(collects)
    ring, ep_start = sp.device_history()
    nodes, top = sp.tree.nodes()
    n_ring = min(sp._t, ring.shape[1])
    out = {
        'ring': np.ascontiguousarray(ring[:, :n_ring]).view(np.uint64).tobytes(),
        'ep_start': ep_start.tobytes(),
        'state': env.state.cpu().numpy().view(np.uint64).tobytes(),
        'steps': env.steps.cpu().numpy().tobytes(),
        'episode': env.episode.tobytes(),
        'episodes': episode_bytes(episodes),
        'top': top.tobytes(),
        'trees': [nodes[g, :top[g]].tobytes() for g in range(G)],
    }
    assert (top == 1 + A * (n_sims + 1)).all()
    sp.tree.check()
    extra = dict(in_lds=plan['tree_in_lds'], ended=len(episodes), missed=sum(missed), eps=episodes, ring_steps=ring.shape[1])
    sp.close()
    return out, extra


@pytest.mark.parametrize('n_sims', [20, 50])
def test_whole_moves_do_not_depend_on_launch_splits_or_workgroup_shape(n_sims):
    """12 moves of 40 environments (noise on, temperature 1, episodes of 5 steps) as 12 launches of one move, as 5 + 5 + 2, as one
    launch of 12 and as 7 + 5, with 16, 8 and 4 games per workgroup: records, states, step and episode counters, finished episodes and
    final trees are the same, bit for bit.  At 50 simulations 16 games per workgroup keep their trees in HBM, 8 and 4 in LDS."""
    base, placements, ended = None, set(), 0
    for gpw in (16, 8, 4):
        for moves_per_launch, collects in ((1, (12, )), (5, (12, )), (12, (12, )), (12, (7, 5))):
            # (an arena of 512 rows: the 40 episodes that end in the same launch fit it at every split -- the default arena of a
            # one-move launch does not hold them all, and a launch whose episodes come partly from the arena and partly from the
            # ring hands them out in another order; the next test reads every episode from the ring)
            got, extra = _play_12(n_sims, moves_per_launch, collects, gpw, arena_rows=512)
            placements.add((gpw, extra['in_lds']))
            ended = extra['ended']
            assert extra['missed'] == 0
            if base is None:
                base = got
                continue
            for k in base:
                assert got[k] == base[k], (k, gpw, moves_per_launch, collects)
    assert placements == ({(16, True), (8, True), (4, True)} if n_sims == 20 else {(16, False), (8, True), (4, True)})
    print('%d simulations: %d episodes ended within the 12 moves' % (n_sims, ended))
    assert ended >= 2 * G   # (every environment ran into the limit of 5 twice: the arena's path)


# ------------------------------------------------------------------ 6. arena too small, the ring wrapping
def test_whole_moves_with_an_arena_too_small_and_a_wrapping_ring():
    """An arena of 3 rows holds no episode of 5 steps: every entry has row -1 and its records come back from the ring -- the same
    bytes as from an arena that fits, over 35 moves in launches of 5 through a ring of 27 steps that wraps."""
    want, w = _play_12(20, 5, (35, ), 0)
    got, e = _play_12(20, 5, (35, ), 0, arena_rows=3)
    assert e['ring_steps'] < 35 and w['missed'] == 0
    assert e['missed'] == e['ended'] == w['ended'] >= 7 * G
    for k in want:
        assert got[k] == want[k], k


# ------------------------------------------------------------------ 7. hand-over to the device replay
def test_whole_moves_hand_over_to_the_device_replay():
    """collect(replay=...) ingests from the launch arenas on the device; a second buffer is given the returned episodes through add.
    Every (episode, position) gathered from both: six tensors bit for bit, with rewards of -1 and value targets below zero."""
    from rlzero_amd.muzero import MuZeroDeviceReplay
    a = MuZeroDeviceReplay(D, A, 128, 5, device=DEV)
    b = MuZeroDeviceReplay(D, A, 128, 5, device=DEV)
    got, extra = _play_12(20, 5, (12, ), 0, replay=a)
    b.add(extra['eps'])
    assert len(a) == len(b) == extra['ended'] >= 2 * G and np.array_equal(a.lengths(), b.lengths())
    draws = every_position(a.lengths(), a.K, A, np.random.RandomState(4))
    x, y = (tuple(v.cpu().numpy() for v in buf.gather(*draws)) for buf in (a, b))
    for name, u, v in zip(('obs', 'actions', 'tv', 'tr', 'tp', 'mask'), x, y):
        assert same_bits(u, v), name
    assert x[2].min() < -1.0 and -1.0 in set(np.unique(x[3]))
    for buf in (a, b):
        assert buf.poll_errors() == 0
        buf.close()


# ------------------------------------------------------------------ 8. CartPole through the new entry point
def test_cartpole_through_play_env_is_play_cartpole():
    """rz_mz_play_env(RZ_MZ_ENV_CARTPOLE, max_episode_steps 500) and rz_mz_play_cartpole from the same start: the same ring, states,
    counters and trees, bit for bit (40 environments, 3 moves, noise on)."""
    import torch
    from rlzero_amd.muzero import CartPoleBatch, MuZeroNet, MuZeroSelfPlay
    runs = []
    for through_env in (False, True):
        torch.manual_seed(7)
        net = MuZeroNet().to(DEV).eval()
        env = CartPoleBatch(G, DEV, seed=3)
        sp = MuZeroSelfPlay(net, env, n_sims=20, seed=9, temperature=1.0, fused=True, fused_moves=True, moves_per_launch=3)
        calls = []
        if through_env:
            def play(*args, tree=sp.tree):
                calls.append(1)
                return tree.play_env(*args)
            sp.tree.play_cartpole = play
        sp.collect(3)
        assert len(calls) == (1 if through_env else 0)
        ring, ep_start = sp.device_history()
        nodes, top = sp.tree.nodes()
        runs.append((ring.tobytes(), ep_start.tobytes(), env.state.cpu().numpy().tobytes(), env.steps.cpu().numpy().tobytes(),
                     env.episode.tobytes(), top.tobytes(), [nodes[g, :top[g]].tobytes() for g in range(G)]))
        assert ring[:, :3, 5].min() == 1.0 and ring.shape[2] == 10
        sp.tree.check()
        sp.close()
    assert runs[0] == runs[1]


# ------------------------------------------------------------------ 9. refusals
def test_whole_moves_refuse_what_they_cannot_serve():
    import torch
    from rlzero_amd._hip import HipError
    from rlzero_amd.muzero import AcrobotBatch, MuZeroNet, MuZeroSelfPlay, MuZeroTree
    env = AcrobotBatch(G, DEV, seed=2, max_episode_steps=12)
    with pytest.raises(ValueError, match='actions'):
        MuZeroSelfPlay(make_net(n_actions=2), env, fused_moves=True)
    with pytest.raises(ValueError, match='obs_dim'):
        MuZeroSelfPlay(make_net(obs_dim=4), env, fused_moves=True)
    with pytest.raises(ValueError, match='fused search'):
        MuZeroSelfPlay(make_net(), env, fused=False, fused_moves=True)
    with pytest.raises(HipError, match='0.1'):
        MuZeroSelfPlay(make_net(), env, fused_moves=True, root_dirichlet_alpha=0.05)

    class Unknown(object):
        n_envs, n_actions, obs_dim, max_episode_steps, device, kind = G, 3, 6, 12, env.device, 'pendulum'

        def observe(self):
            return None
    with pytest.raises(ValueError, match='kind'):
        MuZeroSelfPlay(make_net(), Unknown(), fused_moves=True)

    # the library itself: nothing is launched, the buffers and the environments stay as they were
    sp = whole_moves(env, n_sims=8, seed=1, moves_per_launch=4)
    (counters, entries, arena), _, _ = sp._fused_state()[0]
    history = (sp._ring, sp._ep_start_dev)
    before = env.state.clone()

    def play(tree=sp.tree, hidden=sp.hidden, n_moves=4, alpha=0.25, hist=history, **kw):
        tree.play_env(hidden, 8, n_moves, env, 1, 0.25, alpha, 1.0, hist, 0, arena, counters, entries, **kw)

    with pytest.raises(HipError, match='unknown environment kind'):
        play(kind=7)
    with pytest.raises(HipError, match='0.1'):
        play(alpha=0.05)
    with pytest.raises(HipError, match='ring_steps'):
        play(max_episode_steps=sp._ring.shape[1])   # the ring does not cover an episode + the launch
    two = MuZeroTree(G, 2, 8, device=DEV)
    two.load_model(make_net(n_actions=2))
    two.load_representation(make_net(n_actions=2))
    hidden2 = torch.zeros((G, two.slots_per_game, 64), dtype=torch.float32, device=DEV)
    with pytest.raises(HipError, match='the tree has 2 actions, the environment 3'):
        play(tree=two, hidden=hidden2)
    four = MuZeroTree(G, 3, 8, device=DEV)
    four.load_model(make_net(obs_dim=4))
    with pytest.raises(HipError, match='rz_mz_load_representation'):
        play(tree=four, hidden=sp.hidden)   # no representation loaded
    four.load_representation(make_net(obs_dim=4))
    with pytest.raises(HipError, match='obs_dim 4'):
        play(tree=four, hidden=sp.hidden)
    torch.cuda.synchronize()
    assert not sp._ring.any() and not arena.any() and not entries.any() and same_bits(before.cpu().numpy(), env.state.cpu().numpy())
    assert not env.steps.any()
    for tree in (sp.tree, two, four):
        tree.check()
    two.close()
    four.close()
    sp.close()


# ------------------------------------------------------------------ 10. the trainer
def load_trainer():
    spec = importlib.util.spec_from_file_location('train_muzero', os.path.join(REPO, 'tools', 'train_muzero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _progress(out, n):
    from test_mz_env_gpu import NEW_LINE
    lines = [ln for ln in out.splitlines() if ln.startswith('batch i:')]
    assert len(lines) == n, out
    for line in lines:
        m = NEW_LINE.match(line)   # (the line carries episode_return)
        assert m and int(m.group(2)) > 0 and float(m.group(4)) < 0.0, line
        assert all(np.isfinite(float(m.group(i))) for i in (5, 6, 7, 8)), line


def test_the_trainer_runs_acrobot_on_whole_moves(capsys):
    mod = load_trainer()
    kw = dict(env='acrobot', n_envs=64, n_sims=8, max_episode_steps=12, batch_size=32, updates_per_iteration=2, device_replay=True,
              fused_learner=True)
    pipe = mod.MuZeroPipeline(whole_moves=True, **kw)
    assert pipe.selfplay.fused_moves and not pipe.selfplay.device_moves and 'Acrobot step' in pipe.selfplay.sim_step_label
    pipe.run(2)
    _progress(capsys.readouterr().out, 2)
    pipe.agent.check()
    assert pipe.buffer.poll_errors() == 0
    pipe.selfplay.tree.check()
    pipe.selfplay.close()
    pipe.buffer.close()
    default = mod.MuZeroPipeline(**kw)   # without the flag nothing changes: Acrobot stays on device moves
    assert default.selfplay.device_moves and not default.selfplay.fused_moves
    default.selfplay.close()
    default.buffer.close()
    with pytest.raises(ValueError, match='fused_moves needs the fused search'):
        _refused_pipeline(mod)


def _refused_pipeline(mod):
    """--whole-moves where whole moves cannot run is refused as MuZeroSelfPlay refuses it (here: the fused search switched off)."""
    from rlzero_amd.muzero import MuZeroSelfPlay
    inner = MuZeroSelfPlay.__init__

    def no_fused(self, *args, **kw):
        return inner(self, *args, fused=False, **kw)
    MuZeroSelfPlay.__init__ = no_fused
    try:
        mod.MuZeroPipeline(whole_moves=True, env='acrobot', n_envs=64, n_sims=8, max_episode_steps=12)
    finally:
        MuZeroSelfPlay.__init__ = inner


@pytest.mark.parametrize('side_stream', [False, True], ids=['launch_stream', 'side_stream'])
def test_the_trainers_whole_moves_flag(capsys, side_stream):
    import torch
    mod = load_trainer()
    argv = ['--env', 'acrobot', '--whole-moves', '--envs', '64', '--sims', '8', '--iterations', '2', '--max-episode-steps', '12',
            '--device-replay', '--fused-learner', '--batch-size', '32', '--updates-per-iteration', '2']
    assert mod.build_parser().parse_args(argv).whole_moves and not mod.build_parser().parse_args([]).whole_moves
    if side_stream:
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            pipe = mod.main(argv)
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
    else:
        pipe = mod.main(argv)
    _progress(capsys.readouterr().out, 2)
    assert pipe.selfplay.fused_moves and pipe.env_name == 'acrobot'
    pipe.agent.check()
    pipe.selfplay.tree.check()
    pipe.selfplay.close()
    pipe.buffer.close()
