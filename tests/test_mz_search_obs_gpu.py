"""The search from raw observations in one launch (rz_mz_search_obs; k_mz_search's ROOTS instantiations; MuZeroTree.search_from_obs):
(1) root state, softmax row and root value (row 0 of the trace; raw under the value transform) against ``initial_inference`` on float64
copies, within YARDSTICK = 4 times torch float32's error on the same inputs, measured in the case (one run: profiles/mz_search_obs/
errors.txt); (2) everything behind the root bit for bit against ``init_roots`` of the launch's own softmax rows + ``search_fused`` on a
second tree, with and without noise; (3) Reanalyse with ``fused='observations'`` against the same refresh made by hand; (4) refusals.
Shapes: D 1, 6, 9 (past the whole moves' 8), 16 (the padded tile full); A 1, 3, 8; trees in LDS / HBM (forced through the tree's n_sims
and the games per workgroup, proved by ``search_plan``); gpw + 1 games at 4 and 16 per workgroup; 8 simulations."""
import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from test_mz_learner_host import YARDSTICK, copy_net, sharp_net

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_SIMS = 8
U = 2.0 ** -23
# (D, A, value transform, trees in LDS, games per workgroup, the tree's n_sims: what puts the trees where the case wants them)
CASES = [(1, 1, False, True, 4, 8), (6, 3, False, True, 16, 8), (6, 3, True, False, 16, 60), (9, 3, False, False, 16, 60),
         (9, 8, True, True, 4, 8), (16, 8, False, False, 16, 40), (16, 8, True, True, 16, 8), (16, 1, True, True, 16, 8),
         (1, 8, False, False, 4, 100), (9, 1, False, True, 16, 8), (6, 8, True, False, 4, 100), (16, 3, False, True, 4, 8)]
IDS = ['D%d-A%d-%s-%s-gpw%d' % (D, A, 'vt' if vt else 'raw', 'lds' if lds else 'hbm', gpw) for D, A, vt, lds, gpw, _ in CASES]


def make_tree(G, A, n_sims, gpw, vt, net32=None):
    from rlzero_amd.muzero.tree import MuZeroTree
    tree = MuZeroTree(G, A, n_sims, device=DEV).set_search_shape(gpw)
    if vt:
        tree.set_value_transform(True)
    if net32 is not None:
        tree.load_model(net32)
        tree.load_root_model(net32)
    hidden = torch.zeros((G, tree.slots_per_game, 64), dtype=torch.float32, device=DEV)
    return tree, hidden


def tree_state(tree):
    """What a finished search left: the node records below every game's top, the root visits and the root statistics."""
    nodes, top = tree.nodes()
    return [nodes[g, :top[g]].tobytes() for g in range(len(top))], tree.root_visits().cpu().numpy().copy(), \
        [x.cpu().numpy().copy() for x in tree.root_stats()]


_runs = {}


def case(D, A, vt, lds, gpw, tree_sims):
    """One case, run once and shared: the launch without and with noise, and the twin tree's search behind the launch's own roots."""
    key = (D, A, vt, lds, gpw)
    if key in _runs:
        return _runs[key]
    G = gpw + 1
    net64 = sharp_net(D, A, seed=300 + 10 * D + A)
    net32 = copy_net(net64, torch.float32, DEV).eval()
    gen = torch.Generator().manual_seed(17 * D + A)
    obs = 2.0 * torch.randn(G, D, generator=gen)   # both signs
    obs[1] = 0.0                                   # one all-zero row
    noise = torch.distributions.Dirichlet(torch.full((A, ), 0.25, dtype=torch.float64)).sample((G, )).to(DEV).contiguous()
    tree, hidden = make_tree(G, A, tree_sims, gpw, vt, net32)
    twin, hidden2 = make_tree(G, A, tree_sims, gpw, vt, net32)
    plan = tree.search_plan('observations')
    assert plan['games_per_workgroup'] == gpw and plan['tree_in_lds'] == lds, plan
    out = {'obs': obs, 'net64': net64, 'net32': net32, 'pairs': []}
    for eta in (None, noise):
        hidden.zero_()
        probs = torch.zeros((G, A), dtype=torch.float32, device=DEV)
        trace = tree.search_from_obs(obs.to(DEV), hidden, N_SIMS, noise=eta, noise_frac=0.25, root_probs=probs, trace=True)
        tree.check()
        hidden2.zero_()
        hidden2[:, 0] = hidden[:, 0]
        twin.init_roots(probs, eta, 0.25)
        twin.search_fused(hidden2, N_SIMS)
        twin.check()
        out['pairs'].append((tree_state(tree), tree_state(twin), torch.equal(hidden, hidden2)))
        if eta is None:
            out.update(state=hidden[:, 0].cpu().numpy().copy(), probs=probs.cpu().numpy().copy(), value=trace['value'][0].cpu().numpy().copy(),
                       trace={k: v.cpu().numpy() for k, v in trace.items()})
    tree.close()
    twin.close()
    _runs[key] = out
    return out


def initial(net, obs, vt):
    """(root state, softmax row, root value -- raw under the transform) of ``net.initial_inference`` as float64 numpy arrays."""
    from rlzero_amd.muzero.network import inverse_value_transform
    p = next(net.parameters())
    with torch.no_grad():
        s, logits, v = net.initial_inference(obs.to(p.device, p.dtype))
        v = inverse_value_transform(v) if vt else v
    return [x.double().cpu().numpy() for x in (s, torch.softmax(logits, dim=1), v)]


@pytest.mark.parametrize('D,A,vt,lds,gpw,tree_sims', CASES, ids=IDS)
def test_the_root_against_the_float64_model(D, A, vt, lds, gpw, tree_sims):
    run = case(D, A, vt, lds, gpw, tree_sims)
    want, ref32 = initial(run['net64'], run['obs'], vt), initial(run['net32'], run['obs'], vt)
    for name, got, w, r in zip(('root state', 'root probs', 'root value'), (run['state'], run['probs'], run['value']), want, ref32):
        err = float(np.abs(got.astype(np.float64) - w).max())
        yard = max(float(np.abs(r - w).max()), U * float(np.abs(w).max()))
        print('D=%d A=%d vt=%d %s gpw=%d %s: HIP error %.3e, torch-f32 yardstick %.3e' % (D, A, vt, 'LDS' if lds else 'HBM', gpw, name, err, yard))
        assert np.isfinite(got).all() and err <= YARDSTICK * yard, (name, err, yard)
    assert (run['state'].min(axis=1) == 0.0).all() and (run['state'].max(axis=1) == 1.0).all()   # every root state spans [0, 1] exactly
    t = run['trace']
    assert (t['parent'][0] == -1).all() and (t['action'][0] == -1).all() and (t['leaf'][0] == 0).all() and (t['reward'][0] == 0.0).all()
    assert np.array_equal(t['probs'][0], run['probs']) and (t['parent'][1] == 0).all() and (t['leaf'][1:] >= 1).all()


@pytest.mark.parametrize('D,A,vt,lds,gpw,tree_sims', CASES, ids=IDS)
def test_everything_behind_the_root_is_the_fused_search_bit_for_bit(D, A, vt, lds, gpw, tree_sims):
    for (nodes, visits, stats), (nodes2, visits2, stats2), same_hidden in case(D, A, vt, lds, gpw, tree_sims)['pairs']:
        assert nodes == nodes2 and np.array_equal(visits, visits2) and same_hidden
        assert (stats[0] == N_SIMS).all() and int(visits.sum()) == N_SIMS * (gpw + 1)
        for a, b in zip(stats, stats2):
            assert a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------------------------- 3. Reanalyse end to end
BATCH, LENGTHS = 8, [5, 7, 7]   # 19 steps: chunks of 8, 8 and 3


def filled_replay(D, A):
    from rlzero_amd.muzero import MuZeroDeviceReplay
    from test_mz_replay_host import MAX_STEPS, packed_block
    dev = MuZeroDeviceReplay(D, A, 4, MAX_STEPS, unroll_steps=2, td_steps=3, discount=0.997, seed=3)
    assert dev.add_packed(packed_block(np.random.RandomState(5), LENGTHS, D, A), LENGTHS) == len(LENGTHS)
    return dev


def refresh_by_hand(dev, A, search):
    """Every stored step refreshed through ``positions`` / ``update`` with an independent tree: ``search(tree, hidden, rows)`` runs
    on BATCH rows, a short last chunk padded with its first observation; only the chunk's own rows are written."""
    ep = np.repeat(np.arange(len(LENGTHS)), LENGTHS).astype(np.int64)
    pos = np.concatenate([np.arange(n) for n in LENGTHS]).astype(np.int64)
    where, obs, ticket = dev.positions(ep, pos)
    tree, hidden = make_tree(BATCH, A, N_SIMS, 0, False)
    for a in range(0, len(ep), BATCH):
        rows = obs[a:a + BATCH]
        m = int(rows.shape[0])
        search(tree, hidden, torch.cat((rows, rows[:1].expand(BATCH - m, -1))).contiguous())
        n, vsum, _, _ = tree.root_stats()
        dev.update(where[a:a + m].contiguous(), tree.root_visits()[:m].contiguous(), n[:m].contiguous(), vsum[:m].contiguous(), ticket)
    tree.check()
    tree.close()


def held(dev):
    return [(e.obs.tobytes(), e.actions.tobytes(), e.rewards.tobytes(), e.policies.tobytes(), e.root_values.tobytes()) for e in dev.read()]


def test_reanalyse_from_observations_end_to_end():
    from rlzero_amd.muzero import MuZeroNet, MuZeroReanalyser
    D, A = 6, 3
    torch.manual_seed(11)
    net = MuZeroNet(obs_dim=D, n_actions=A, hidden=64).to(DEV).eval()

    def from_obs(tree, hidden, rows):
        tree.load_model(net)
        tree.load_root_model(net)
        tree.search_from_obs(rows, hidden, N_SIMS)

    def through_torch(tree, hidden, rows):
        tree.load_model(net)
        with torch.no_grad():
            s0, logits, _ = net.initial_inference(rows)
            hidden[:, 0] = s0
            tree.init_roots(torch.softmax(logits, dim=1).contiguous(), None)
        tree.search_fused(hidden, N_SIMS)

    for fused, by_hand in (('observations', from_obs), (None, through_torch)):
        dev, want = filled_replay(D, A), filled_replay(D, A)
        before = held(dev)
        rean = MuZeroReanalyser(net, dev, n_sims=N_SIMS, batch=BATCH, fused=fused, seed=21)
        assert rean.from_obs == (fused == 'observations') and rean.reanalyse_all() == sum(LENGTHS)
        refresh_by_hand(want, A, by_hand)
        after = held(dev)
        assert after == held(want), fused
        for was, now in zip(before, after):   # every step was refreshed, nothing else moved
            assert was[:3] == now[:3] and was[3] != now[3] and was[4] != now[4]
        assert dev.poll_errors() == 0
        rean.close()
        dev.close()
        want.close()


# ----------------------------------------------------------------------------------------------- 4. the refusals
def direct(tree, obs, hidden):   # (past the binding's own check for a root model)
    from rlzero_amd.engine import _ptr, check
    check(tree.lib.rz_mz_search_obs(tree.handle, _ptr(obs), _ptr(hidden), N_SIMS, None, 0.0, None, *([None] * 6), tree.stream()))


def other_net(**kw):
    from rlzero_amd.muzero import MuZeroNet
    return MuZeroNet(**dict(dict(obs_dim=6, n_actions=3, hidden=64), **kw))


REFUSALS = {'gumbel': (lambda t, o, h: t.set_gumbel(4).search_from_obs(o, h, N_SIMS), 'pUCT rule'),
            'support': (lambda t, o, h: t.set_value_transform(True).set_support(3).search_from_obs(o, h, N_SIMS), 'scalar heads'),
            'too many simulations': (lambda t, o, h: t.search_from_obs(o, h, N_SIMS + 1), 'n_sims'),
            'no root model': (direct, 'rz_mz_load_root_model has not been called'),
            'wide observations': (lambda t, o, h: t.load_root_model(other_net(obs_dim=17)), '1 .. 16 observation features'),
            'another hidden size': (lambda t, o, h: t.load_root_model(other_net(hidden=32)), 'hidden size 64')}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_the_refusals_name_their_reason(what):
    from rlzero_amd import _hip
    attempt, reason = REFUSALS[what]
    net = other_net()
    tree, hidden = make_tree(5, 3, N_SIMS, 4, False)
    tree.load_model(net)
    if what != 'no root model':
        tree.load_root_model(net)
    with pytest.raises(_hip.HipError, match=reason):
        attempt(tree, torch.zeros((5, 6), device=DEV), hidden)
    tree.close()


@pytest.mark.parametrize('D,A,hidden,support,reason', [(6, 3, 32, None, 'hidden size 32'), (6, 3, 64, 3, 'categorical heads')])
def test_the_reanalyser_names_what_the_route_does_not_serve(D, A, hidden, support, reason):
    """(More than 8 actions or 16 observation features never get this far: the device replay itself holds at most that.)"""
    from rlzero_amd.muzero import MuZeroDeviceReplay, MuZeroNet, MuZeroReanalyser
    net = MuZeroNet(obs_dim=D, n_actions=A, hidden=hidden, value_transform=support is not None, support=support).to(DEV)
    dev = MuZeroDeviceReplay(D, A, 4, 12, unroll_steps=2, td_steps=3, discount=0.997, seed=3, value_transform=support is not None)
    with pytest.raises(ValueError, match=reason):
        MuZeroReanalyser(net, dev, n_sims=N_SIMS, batch=BATCH, fused='observations')
    dev.close()
