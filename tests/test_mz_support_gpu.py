"""k_mz_search's CAT instantiations -- categorical reward and value heads read as h^-1 of their expectation -- on the GPU.

Per case a traced search of the float32 copy of a float64 support net.  Every traced reward and value against the float64 net (the
expectation by the twin rlzero_amd/muzero/support.py) on the kernel's OWN parent states and actions, within 4 times the error of the torch
float32 route on the same inputs, floored at 2^-23 max |value| (tests/test_mz_search_net_gpu.py's rule; profiles/mz_support/errors.txt).
Then every tree, MinMax bound and visit count bit-equal to the pseudocode tree fed the traced outputs.  ``gain`` scales the heads' weights;
``pin`` adds 200 to the bias of the reward head's lowest and the value head's highest bin: the expectation rounds to the support's end."""
import functools
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import muzero_ref as ref
from rlzero_amd import _hip
from rlzero_amd.muzero import (AcrobotBatch, MuZeroDeviceReplay, MuZeroNet, MuZeroReanalyser, MuZeroSelfPlay, MuZeroTree, gumbel,
                               inverse_value_transform, support as sup)

pytestmark = pytest.mark.gpu
DEV, GAMES, OBS, YARDSTICK, U = 'cuda:0', 37, 6, 4.0, 2.0 ** -23
#        S  A n_sims gain rule gpw pin  trees in LDS
CASES = [(1, 2, 12, 1.0, 'puct', 16, False, True), (20, 3, 20, 1.0, 'puct', 4, False, True), (31, 8, 6, 20.0, 'puct', 16, True, False),
         (31, 8, 20, 1.0, 'puct', 16, False, False), (20, 2, 20, 20.0, 'puct', 16, False, False), (1, 3, 20, 20.0, 'gumbel', 4, False, True),
         (20, 8, 20, 1.0, 'gumbel', 16, False, False), (31, 2, 12, 1.0, 'gumbel', 4, False, True), (31, 3, 16, 20.0, 'puct', 4, False, True),
         (20, 3, 8, 1.0, 'gumbel', 16, False, False)]


@functools.lru_cache(maxsize=None)
def nets(A, S, gain=1.0, pin=False):   # -> (a float64 support net on the CPU, its float32 copy on the GPU)
    torch.manual_seed(7 * S + A)
    net = MuZeroNet(OBS, A, 64, value_transform=True, support=S).double()
    with torch.no_grad():
        for name, p in net.named_parameters():
            p.mul_(2.0) if name.endswith('weight') else p.copy_(torch.randn_like(p) * 0.3)
        net.rew2.weight.mul_(gain)
        net.val.weight.mul_(gain)
        if pin:
            net.rew2.bias[0] += 200.0
            net.val.bias[-1] += 200.0
    net32 = MuZeroNet(OBS, A, 64, value_transform=True, support=S).to(DEV)
    net32.load_state_dict({k: v.float() for k, v in net.state_dict().items()})
    return net.eval(), net32.eval()


@pytest.mark.parametrize('S,A,n_sims,gain,rule,gpw,pin,in_lds', CASES)
def test_every_traced_node_and_every_tree(S, A, n_sims, gain, rule, gpw, pin, in_lds):
    net64, net32 = nets(A, S, gain, pin)
    tree = MuZeroTree(GAMES, A, n_sims, device=DEV).set_search_shape(gpw).set_value_transform(True).set_support(S)
    tree.load_model(net32)
    hidden = torch.zeros((GAMES, tree.slots_per_game, 64), dtype=torch.float32, device=DEV)
    with torch.no_grad():
        hidden[:, 0], logits, _ = net32.initial_inference(torch.randn(GAMES, OBS, generator=torch.Generator().manual_seed(S + A)).to(DEV))
    tree.init_roots(torch.softmax(logits, dim=1).contiguous())
    if rule == 'gumbel':
        g = torch.randn(GAMES, A, generator=torch.Generator().manual_seed(3)).to(DEV).contiguous()
        trace = tree.set_gumbel(4).search_gumbel(hidden, n_sims, g, trace=True)[2]
    else:
        trace = tree.search_fused(hidden, n_sims, trace=True)
    assert tree.search_plan(False) == dict(tree.search_plan(False), games_per_workgroup=gpw, tree_in_lds=in_lds)
    tree.check()
    nodes, top = tree.nodes()
    n, vsum, vmin, vmax = (x.cpu().numpy().copy() for x in tree.root_stats())
    tree.close()
    parent, action = trace['parent'].reshape(-1).long(), trace['action'].reshape(-1).long()
    states = hidden[torch.arange(GAMES, device=DEV).repeat(n_sims), parent]
    with torch.no_grad():   # the torch float32 route and the float64 net on the kernel's own inputs
        _, r32, _, v32 = net32.recurrent_inference(states, action)
        nxt64, rh = net64.dynamics_logits(states.double().cpu(), action.cpu())
        vh = net64.prediction_logits(nxt64)[1]
    for name, head, r in (('reward', rh, r32), ('value', vh, v32)):
        want = inverse_value_transform(torch.from_numpy(sup.support_expectation(head.numpy(), S))).numpy()
        got, r = trace[name].reshape(-1).double().cpu().numpy(), inverse_value_transform(r).double().cpu().numpy()
        err, yard = float(np.abs(got - want).max()), max(float(np.abs(r - want).max()), U * float(np.abs(want).max()))
        print('S=%d A=%d n_sims=%d gain=%g %s gpw=%d %s: HIP error %.3e, torch-f32 yardstick %.3e, ratio %.2f' % (S, A, n_sims, gain, rule, gpw, name, err, yard, err / yard))
        assert np.isfinite(got).all() and err <= YARDSTICK * yard
        if pin:   # h^-1 of the support's end after the rounding to float32
            assert (got == inverse_value_transform(torch.tensor([-S if name == 'reward' else S], dtype=torch.float64)).float().item()).all()
    tr = {k: v.cpu().numpy() for k, v in trace.items()}
    if rule == 'gumbel':
        want = gumbel.gumbel_search_reference(nodes['prior'][:, 1:1 + A], nodes['pad'].view(np.float32)[:, 0], g.cpu().numpy(), tr['reward'], tr['probs'], tr['value'],
                                              gumbel.considered_visits(min(4, A), n_sims), tree.discount)
        assert len(keep := np.flatnonzero(want['min_gap'] >= 1e-9)) >= GAMES - 1
        for gi in keep:
            used = slice(0, int(want['top'][gi]))
            assert top[gi] == want['top'][gi] and vmin[gi] == want['lo'][gi] and vmax[gi] == want['hi'][gi]
            assert all(np.array_equal(nodes[k][gi, used], want[k][gi, used]) for k in ('N', 'first_child', 'value_sum', 'prior', 'reward'))
        return
    for gi in range(GAMES):
        root, step = ref.Node(0), [0]
        ref.expand_node(root, None, 0.0, [float(p) for p in nodes['prior'][gi, 1:1 + A]])

        def model(hidden_state, a, path):
            s, step[0] = step[0], step[0] + 1
            assert tr['action'][s, gi] == a
            return None, float(tr['reward'][s, gi]), [float(p) for p in tr['probs'][s, gi]], float(tr['value'][s, gi])
        stats = ref.run_mcts(ref.MuZeroConfig(num_simulations=n_sims), root, model)
        assert (stats.minimum, stats.maximum, root.visit_count, root.value_sum) == (vmin[gi], vmax[gi], n[gi], vsum[gi])
        for path, (cnt, value_sum, reward, prior) in ref.tree_dump(root).items():
            slot = functools.reduce(lambda s, a: nodes['first_child'][gi, s] + a, path, 0)
            assert tuple(nodes[k][gi, slot] for k in ('N', 'value_sum', 'reward', 'prior')) == (cnt, value_sum, np.float32(reward), prior), (gi, path)


def play(device_moves, replay=None):   # 30 arg-max moves of 40 Acrobot environments, 10 simulations, no noise -> (episodes as bytes, self-play)
    sp = MuZeroSelfPlay(nets(3, 20)[1], AcrobotBatch(40, DEV, seed=9, max_episode_steps=12), n_sims=10, temperature=0.0, root_exploration_fraction=0.0,
                        seed=4, moves_per_launch=7, device_moves=device_moves)
    eps = sp.collect(30, replay=replay)
    sp.tree.check()
    return [tuple(np.asarray(getattr(e, f)).tobytes() for f in e.FIELDS) for e in eps], sp


def test_device_moves_play_the_host_loops_episodes_and_reanalyse_writes_a_searchs_root_value():
    replay = MuZeroDeviceReplay(OBS, 3, 128, 12, device=DEV, value_transform=True)
    want, host = play(False)
    got, dev = play(True, replay)
    assert got == want and len(got) >= 40 and torch.equal(dev.env.state, host.env.state) and dev.device_moves and not host.device_moves
    dev.close()
    ep_idx, pos = np.arange(40) % len(replay), np.arange(40) % 5
    rean = MuZeroReanalyser(nets(3, 20)[1], replay, n_sims=10, batch=40)
    assert rean.tree.support == 20 and rean.reanalyse(ep_idx, pos) == 40
    kept = replay.read()
    obs = torch.from_numpy(np.stack([kept[e].obs[p] for e, p in zip(ep_idx, pos)])).to(DEV)
    root_value = host.search(obs, add_noise=False)[1]
    assert np.array_equal([kept[e].root_values[p] for e, p in zip(ep_idx, pos)], root_value.cpu().numpy())
    rean.close()
    host.close()


def test_the_plan_and_the_refusals():
    net = nets(3, 20)[1]
    tree = MuZeroTree(GAMES, 3, 20, device=DEV)
    scalar = [tree.set_search_shape(gpw).search_plan(False) for gpw in (4, 16)]
    tree.set_value_transform(True).set_support(20)
    cat = [tree.set_search_shape(gpw).search_plan(False) for gpw in (4, 16)]
    assert all(p['tree_in_lds'] for p in scalar) and cat[0]['tree_in_lds'] and not cat[1]['tree_in_lds'] and \
        cat[0]['lds_bytes'] - scalar[0]['lds_bytes'] == (64 * 16 + 2 * 16 * 65 + 2 * 64 * 64 + 2 * 64) * 4   # 16 games of 65 nodes leave LDS
    hidden = torch.zeros((GAMES, tree.slots_per_game, 64), dtype=torch.float32, device=DEV)
    tree.init_roots(torch.full((GAMES, 3), 1.0 / 3, dtype=torch.float32, device=DEV))
    assert tree.lib.rz_mz_play_cartpole(tree.handle, None, 16, 1, None, None) != _hip.OK and b'whole moves keep scalar heads' in tree.lib.rz_last_error()
    for model, S, vt, why in ((MuZeroNet(OBS, 3, 64, value_transform=True).to(DEV), 20, True, 'support'), (net, None, True, 'support'),
                              (net, 20, False, 'value transform')):   # a scalar model, a scalar search, no transform
        tree.set_support(S).set_value_transform(vt).load_model(model)
        with pytest.raises(_hip.HipError, match=why):
            tree.search_fused(hidden, 20)
    tree.close()
    for kw, why in ((dict(net=MuZeroNet(OBS, 3, 32, value_transform=True, support=20).to(DEV)), 'hidden size 64'), (dict(net=net, fused_moves=True), 'whole moves')):
        with pytest.raises(ValueError, match=why):
            MuZeroSelfPlay(kw.pop('net'), AcrobotBatch(8, DEV, seed=0), n_sims=8, **kw)


def test_the_trainer_runs_with_a_support(capsys):
    sys.path.insert(0, REPO + '/tools')
    import train_muzero
    pipe = train_muzero.main(['--env', 'acrobot', '--max-episode-steps', '12', '--envs', '40', '--sims', '10', '--iterations', '2', '--batch-size', '32',
                              '--updates-per-iteration', '2', '--value-transform', '--support', '20', '--device-replay'])
    out = capsys.readouterr().out
    assert pipe.agent.net.support == 20 and pipe.selfplay.tree.support == 20 and out.count('batch i:') == 2 and len(pipe.buffer) > 0
    assert all(np.isfinite(float(line.split('loss:')[1].split(',')[0])) for line in out.splitlines() if line.startswith('batch'))
    pipe.selfplay.tree.check()
