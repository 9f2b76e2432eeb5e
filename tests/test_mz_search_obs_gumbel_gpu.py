"""The Gumbel search from raw observations in one launch (rz_mz_search_obs_gumbel; k_mz_search's GUMBEL ROOTS instantiations;
MuZeroTree.search_gumbel_from_obs): (1) root state, softmax row and root value (row 0 of the trace: raw under the value transform, h^-1 of
the support's expectation with a support) against ``initial_inference`` on float64 copies, within the YARDSTICK = 4 times torch float32's
error on the same inputs that tests/test_mz_search_obs_gpu.py allows (one run: profiles/mz_search_obs_gumbel/errors.txt); (2) everything
behind the root bit for bit against ``init_roots`` of the launch's own softmax rows + ``search_gumbel`` on a second tree: moves, pi', trace
rows 1 .., node records with v_hat; (3) Gumbel device moves of self-play with ``fused_roots`` against the same moves made by hand; (4) refusals.
Shapes: D 1, 16; A 1, 3, 8; max_considered 4 and >= A; gpw + 1 games at 4 and 16 per workgroup; supports 3 and 31; g = 0 once.  8
simulations, but 12 where scalar heads must leave LDS: the Gumbel schedule pins a launch's n_sims to the tree's, and 16 games of 8 actions
with 8 simulations still fit (74 KB)."""
import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from test_mz_learner_host import YARDSTICK
from test_mz_search_obs_gpu import initial, make_tree

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -23
#        D   A  vt    S   m gpw sims LDS  g = 0
CASES = [(1, 1, False, 0, 4, 4, 8, True, False), (16, 3, True, 0, 4, 16, 8, True, True), (16, 8, False, 0, 4, 16, 12, False, False),
         (1, 8, True, 0, 8, 16, 12, False, False), (16, 3, True, 3, 4, 4, 8, True, False), (1, 8, True, 31, 4, 16, 8, False, False),
         (16, 8, True, 31, 8, 4, 8, True, False), (1, 3, True, 3, 4, 16, 8, False, False)]
IDS = ['D%d-A%d-%s-S%d-m%d-gpw%d-%s' % (D, A, 'vt' if vt else 'raw', S, m, gpw, 'lds' if lds else 'hbm') for D, A, vt, S, m, gpw, _, lds, _ in CASES]
_runs = {}


def nets(D, A, vt, S, seed):   # -> (a float64 net on the CPU with wide weights and biases, its float32 copy on the GPU)
    from rlzero_amd.muzero import MuZeroNet
    torch.manual_seed(seed)
    kw = dict(value_transform=vt, support=S or None)
    net = MuZeroNet(D, A, 64, **kw).double()
    with torch.no_grad():
        for name, p in net.named_parameters():
            p.mul_(2.0) if name.endswith('weight') else p.copy_(torch.randn_like(p) * 0.3)
    net32 = MuZeroNet(D, A, 64, **kw).to(DEV)
    net32.load_state_dict({k: v.float() for k, v in net.state_dict().items()})
    return net.eval(), net32.eval()


def gumbel_tree(G, A, n_sims, gpw, vt, S, m, net32, roots=True):
    tree, hidden = make_tree(G, A, n_sims, gpw, vt)
    tree.set_support(S).set_gumbel(m).load_model(net32)
    if roots:
        tree.load_root_model(net32)
    return tree, hidden


def searched(tree, trace):
    """What a finished Gumbel search left: node records (v_hat in the last word) below every top, MinMax bounds, trace rows of the simulations."""
    nodes, top = tree.nodes()
    stats = [x.cpu().numpy().tobytes() for x in tree.root_stats()]
    return [nodes[g, :top[g]].tobytes() for g in range(len(top))], stats, {k: v.cpu().numpy().copy() for k, v in trace.items()}


def case(D, A, vt, S, m, gpw, n_sims, lds, greedy):
    """One case, run once and shared: the launch, and the twin tree's ``init_roots`` + ``search_gumbel`` behind the launch's own roots."""
    key = (D, A, vt, S, m, gpw)
    if key in _runs:
        return _runs[key]
    G = gpw + 1
    net64, net32 = nets(D, A, vt, S, 500 + 10 * D + A + S)
    gen = torch.Generator().manual_seed(17 * D + A + S)
    obs = 2.0 * torch.randn(G, D, generator=gen)
    obs[1] = 0.0
    u = torch.rand(G, A, generator=gen).clamp_(1e-6, 1.0 - 1e-6)
    g = (torch.zeros(G, A) if greedy else -torch.log(-torch.log(u))).to(DEV, torch.float32).contiguous()
    tree, hidden = gumbel_tree(G, A, n_sims, gpw, vt, S, m, net32)
    twin, hidden2 = gumbel_tree(G, A, n_sims, gpw, vt, S, m, net32, roots=False)
    for t, which in ((tree, 'observations_gumbel'), (twin, False)):
        plan = t.search_plan(which)
        assert plan['games_per_workgroup'] == gpw and plan['tree_in_lds'] == lds, plan
    probs = torch.zeros((G, A), dtype=torch.float32, device=DEV)
    action, pi, trace = tree.search_gumbel_from_obs(obs.to(DEV), hidden, n_sims, g, root_probs=probs, trace=True)
    tree.check()
    hidden2[:, 0] = hidden[:, 0]
    twin.init_roots(probs, None)
    action2, pi2, trace2 = twin.search_gumbel(hidden2, n_sims, g, trace=True)
    twin.check()
    out = {'obs': obs, 'net64': net64, 'net32': net32, 'state': hidden[:, 0].cpu().numpy().copy(), 'probs': probs.cpu().numpy().copy(),
           'new': searched(tree, {k: v[1:] for k, v in trace.items()}) + (action.cpu().numpy().copy(), pi.cpu().numpy().copy()),
           'old': searched(twin, trace2) + (action2.cpu().numpy().copy(), pi2.cpu().numpy().copy()),
           'row0': {k: v[0].cpu().numpy().copy() for k, v in trace.items()}, 'same_hidden': torch.equal(hidden, hidden2)}
    tree.close()
    twin.close()
    _runs[key] = out
    return out


@pytest.mark.parametrize('D,A,vt,S,m,gpw,n_sims,lds,greedy', CASES, ids=IDS)
def test_the_root_against_the_float64_model(D, A, vt, S, m, gpw, n_sims, lds, greedy):
    run = case(D, A, vt, S, m, gpw, n_sims, lds, greedy)
    r0 = run['row0']
    want, ref32 = initial(run['net64'], run['obs'], vt), initial(run['net32'], run['obs'], vt)
    for name, got, w, r in zip(('root state', 'root probs', 'root value'), (run['state'], r0['probs'], r0['value']), want, ref32):
        err = float(np.abs(got.astype(np.float64) - w).max())
        yard = max(float(np.abs(r - w).max()), U * float(np.abs(w).max()))
        print('D=%d A=%d vt=%d S=%d %s gpw=%d %s: HIP error %.3e, torch-f32 yardstick %.3e, ratio %.2f' % (
            D, A, vt, S, 'LDS' if lds else 'HBM', gpw, name, err, yard, err / yard))
        assert np.isfinite(got).all() and err <= YARDSTICK * yard, (name, err, yard)
    assert (r0['parent'] == -1).all() and (r0['action'] == -1).all() and (r0['leaf'] == 0).all() and (r0['reward'] == 0.0).all()
    assert np.array_equal(r0['probs'], run['probs'])


@pytest.mark.parametrize('D,A,vt,S,m,gpw,n_sims,lds,greedy', CASES, ids=IDS)
def test_everything_behind_the_root_is_the_gumbel_search_bit_for_bit(D, A, vt, S, m, gpw, n_sims, lds, greedy):
    run = case(D, A, vt, S, m, gpw, n_sims, lds, greedy)
    (nodes, stats, trace, action, pi), (nodes2, stats2, trace2, action2, pi2) = run['new'], run['old']
    assert nodes == nodes2 and stats == stats2 and run['same_hidden']
    assert np.array_equal(action, action2) and pi.tobytes() == pi2.tobytes() and (pi.sum(axis=1) > 0.999).all()
    for k in trace:
        assert trace[k].tobytes() == trace2[k].tobytes(), k
    v_hat = np.frombuffer(nodes[0], dtype='<f4')[7]   # (the last word of game 0's root record)
    assert v_hat == run['row0']['value'][0]


def test_device_moves_with_fused_roots_are_the_moves_made_by_hand():
    """Three Gumbel device moves of 9 Acrobot environments with ``fused_roots``; then, from the recorded observations, every move again
    through ``search_gumbel_from_obs``'s own roots + ``init_roots`` + ``search_gumbel`` with the same Gumbel rows: actions and stored pi'."""
    from rlzero_amd.muzero import AcrobotBatch, MuZeroSelfPlay
    G, MOVES, SIMS = 9, 3, 8
    _, net32 = nets(6, 3, True, 3, 77)

    def player(**kw):
        return MuZeroSelfPlay(net32, AcrobotBatch(G, DEV, seed=5, max_episode_steps=50), n_sims=SIMS, seed=4, moves_per_launch=MOVES,
                              search='gumbel', **kw)
    sp = player(fused_roots=True)
    assert sp.device_moves and sp.fused_roots
    sp.collect(MOVES)
    ring = sp.device_history()[0][:, :MOVES]   # obs (6) | action | reward | pi' (3) | root value | done
    sp.close()
    ref = player()   # (its generator gives the same Gumbel rows in the same order)
    tree, probs = ref.tree, torch.zeros((G, 3), dtype=torch.float32, device=DEV)
    tree.load_root_model(net32)
    scratch = torch.zeros_like(ref.hidden)
    for k in range(MOVES):
        obs = torch.from_numpy(ring[:, k, :6]).to(DEV, torch.float32).contiguous()
        g = ref._gumbel_draws()
        tree.search_gumbel_from_obs(obs, scratch, SIMS, g, root_probs=probs)
        ref.hidden.zero_()
        ref.hidden[:, 0] = scratch[:, 0]
        tree.init_roots(probs, None)
        action, pi = tree.search_gumbel(ref.hidden, SIMS, g)
        assert np.array_equal(ring[:, k, 6], action.cpu().numpy().astype(np.float64))
        assert np.array_equal(ring[:, k, 8:11], pi.cpu().numpy().astype(np.float64))
    tree.check()
    ref.close()


def no_root_model(tree, obs, hidden, g):   # (past the binding's own check)
    from rlzero_amd.engine import _ptr, check
    check(tree.lib.rz_mz_search_obs_gumbel(tree.handle, _ptr(obs), _ptr(hidden), 8, _ptr(g), _ptr(tree.gumbel_action), _ptr(tree.gumbel_pi), None,
                                           *([None] * 6), tree.stream()))


def gumbel_off(tree, obs, hidden, g):
    tree.set_gumbel(0).search_gumbel_from_obs(obs, hidden, 8, g)


REFUSALS = {'gumbel off': (gumbel_off, 'not switched the Gumbel search on'),
            'another support': (lambda t, o, h, g: t.set_value_transform(True).set_support(3).search_gumbel_from_obs(o, h, 8, g), 'the loaded model has support 0'),
            'no root model': (no_root_model, 'rz_mz_load_root_model has not been called'),
            'other simulations': (lambda t, o, h, g: t.search_gumbel_from_obs(o, h, 7, g), 'schedule of n_sims = 8'),
            'paths past LDS': (lambda t, o, h, g: t.search_gumbel_from_obs(o, h, 2400, g), 'paths do not fit in LDS')}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_the_refusals_name_their_reason(what):
    from rlzero_amd import _hip
    attempt, reason = REFUSALS[what]
    n_sims = 2400 if what == 'paths past LDS' else 8
    tree, hidden = gumbel_tree(5, 3, n_sims, 16, False, 0, 4, nets(6, 3, False, 0, 1)[1], roots=what != 'no root model')
    with pytest.raises(_hip.HipError, match=reason):
        attempt(tree, torch.zeros((5, 6), device=DEV), hidden, torch.zeros((5, 3), device=DEV))
    tree.close()
