"""The network k_mz_search<.., MOVES = false> evaluates inside the kernel -- dynamics, reward head, min-max scaling, prediction with
softmax on v_mfma_f32_16x16x4_f32 -- against the float64 twin (tests/mz_net_twin.py) at 1, 2, 3, 4, 5 and 8 actions.

Per case: ``MuZeroTree`` directly on the current stream, G = 37 games (ragged against 16, 8 and 4 games per workgroup),
``load_model`` of the float32 copy of a net of tests/test_mz_search_net_host.py, the root state from torch's initial inference,
uniform root priors, ``search_fused(trace=True)``.  Per simulation and game the twin is applied to the kernel's OWN float32 parent
state ``hidden[g, parent]`` (read as float64) and the traced action, and compared with the traced reward / probabilities / value and
the state the kernel stored for the leaf.

The tolerance is measured in the case: the YARDSTICK of a quantity is the largest error of ``net32.recurrent_inference`` (torch
float32 on the GPU, simulation by simulation on the same inputs) against the twin, floored at 2^-23 max |twin|; the kernel may be
``YARDSTICK`` = 4 of them away (it sums in another order than rocBLAS; the learner's kernels are held to the same factor).  The host
test shows that every wrong term it knows of lands 2e5 yardsticks or more away.  One run's figures: profiles/mz_search_net/errors.txt.

From the traces, as conditions: every action is an edge at every A; per A, over the four variants (dyn2's rows rolled by 0 / 16 / 32
/ 48), the arg-min and the arg-max of the unscaled next state fall into every wave's 16 rows; both tree placements (LDS, HBM) ran at
A = 3 and at A = 8.

This file takes no stream from torch's pool and builds no self-play pipeline in the suite's process (the docstring of
tests/test_mz_learner_gpu.py says why)."""
import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
import mz_net_twin as twin
from test_mz_learner_host import YARDSTICK, copy_net
from test_mz_search_net_host import GAMES, OBS_DIM, ROLLS, assert_covered, errors, rolled_net

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = ((1, 12), (2, 30), (3, 30), (4, 25), (5, 30), (8, 12), (8, 40))   # (A, n_sims), each at four rolls and 16 games per workgroup
CASES = [(A, n, roll, 16) for A, n in SHAPES for roll in ROLLS] + [(3, 40, 0, 16)] + \
        [(A, n, roll, 4) for A, n in ((3, 30), (8, 40)) for roll in ROLLS]
U = 2.0 ** -23


class Search(object):
    """A tree of GAMES games with ``net64``'s float32 copy loaded; ``run`` searches from fixed observations and returns numpy arrays."""

    def __init__(self, net64, n_sims, gpw):
        from rlzero_amd.muzero.tree import MuZeroTree
        self.A, self.n_sims = net64.n_actions, n_sims
        self.tree = MuZeroTree(GAMES, self.A, n_sims, device=DEV).set_search_shape(gpw)
        self.hidden = torch.zeros((GAMES, self.tree.slots_per_game, 64), dtype=torch.float32, device=DEV)
        self.obs = torch.randn(GAMES, OBS_DIM, generator=torch.Generator().manual_seed(1000 + 10 * self.A + n_sims)).to(DEV)
        self.priors = torch.full((GAMES, self.A), 1.0 / self.A, dtype=torch.float32, device=DEV)
        self.load(net64)

    def load(self, net64):
        self.net64, self.net32 = net64, copy_net(net64, torch.float32, DEV).eval()
        self.tree.load_model(self.net32)

    def start(self):
        self.hidden.zero_()
        with torch.no_grad():
            self.hidden[:, 0] = self.net32.initial_inference(self.obs)[0]
        self.tree.init_roots(self.priors)

    def run(self):
        """-> dict: the trace and the hidden states as numpy arrays, the plan, the torch-f32 outputs on the kernel's inputs."""
        self.start()
        trace = self.tree.search_fused(self.hidden, self.n_sims, trace=True)
        rows = torch.arange(GAMES, device=DEV)
        ref32 = []
        with torch.no_grad():
            for s in range(self.n_sims):
                nxt, r, logits, v = self.net32.recurrent_inference(self.hidden[rows, trace['parent'][s].long()], trace['action'][s].long())
                ref32.append((nxt, r, torch.softmax(logits, dim=1), v))
        out = {k: v.cpu().numpy() for k, v in trace.items()}
        out['hidden'] = self.hidden.cpu().numpy()
        out['ref32'] = tuple(torch.cat([x[i] for x in ref32]).double().cpu().numpy() for i in range(4))
        out['plan'] = self.tree.search_plan(False)
        n, _, _, _ = self.tree.root_stats()
        assert (n.cpu().numpy() == self.n_sims).all()
        self.tree.check()
        return out

    def close(self):
        self.tree.close()


def compare(what, out, sd, report=True):
    """The kernel's four quantities against the twin of the model ``sd`` on the kernel's own inputs.
    -> (twin outputs, kernel outputs, HIP errors [4], yardsticks [4]); prints a line per quantity."""
    S, G = out['parent'].shape
    games = np.broadcast_to(np.arange(G), (S, G))
    states = out['hidden'][games, out['parent']].reshape(S * G, 64)
    assert out['action'].min() >= 0 and out['leaf'].min() >= 1 and (out['parent'] != out['leaf']).all()
    want = twin.recurrent(sd, states.astype(np.float64), out['action'].reshape(-1))
    got = (out['hidden'][games, out['leaf']].reshape(S * G, 64), out['reward'].reshape(-1), out['probs'].reshape(S * G, -1), out['value'].reshape(-1))
    for x in got:
        assert np.isfinite(x).all(), what
    err = errors(got, want)
    yard = [max(e, U * float(np.abs(w).max())) for e, w in zip(errors(out['ref32'], want), want[:4])]
    if report:
        for name, e, y in zip(twin.QUANTITIES, err, yard):
            print('%s %s: HIP error %.3e, torch-f32 yardstick %.3e' % (what, name, e, y))
    return want, got, err, yard


def assert_within(what, err, yard):
    for name, e, y in zip(twin.QUANTITIES, err, yard):
        assert e <= YARDSTICK * y, (what, name, e, y)


def assert_probabilities(got, A):
    probs = got[2]
    assert (probs >= 0.0).all() and (probs <= 1.0).all()
    assert np.abs(probs.astype(np.float64).sum(axis=1) - 1.0).max() <= (A + 1) * U


_runs = {}


def case(A, n_sims, roll, gpw):
    """One search of a variant and its comparison with the twin: run once, shared by the tests below, never modified."""
    key = (A, n_sims, roll, gpw)
    if key not in _runs:
        net64 = rolled_net(A, roll)
        search = Search(net64, n_sims, gpw)
        out = search.run()
        search.close()
        what = 'A=%d n_sims=%d roll=%d gpw=%d (%s)' % (A, n_sims, roll, gpw, 'LDS' if out['plan']['tree_in_lds'] else 'HBM')
        _runs[key] = (what, out) + compare(what, out, twin.state_dict64(net64))
    return _runs[key]


@pytest.mark.parametrize('A,n_sims,roll,gpw', CASES)
def test_the_kernels_network_against_the_twin(A, n_sims, roll, gpw):
    what, out, want, got, err, yard = case(A, n_sims, roll, gpw)
    assert out['plan']['games_per_workgroup'] == gpw
    assert_within(what, err, yard)
    # what needs no tolerance
    assert (got[0].min(axis=1) == 0.0).all() and (got[0].max(axis=1) == 1.0).all()   # every stored leaf state spans [0, 1] exactly
    assert_probabilities(got, A)
    if A == 1:
        assert (got[2] == 1.0).all()
    assert set(np.unique(out['action']).tolist()) == set(range(A))   # every action is an edge (and none outside)


@pytest.mark.parametrize('A', sorted(set(a for a, _ in SHAPES)))
def test_the_kernels_own_parents_put_extremes_in_every_waves_rows(A):
    ts = [case(a, n, roll, 16)[2].t for a, n in SHAPES if a == A for roll in ROLLS]
    assert_covered(A, ts, 'kernel parents')


def test_both_tree_placements_ran_at_3_and_at_8_actions():
    for A in (3, 8):
        seen = set(case(*c)[1]['plan']['tree_in_lds'] for c in CASES if c[0] == A)
        assert seen == {True, False}, (A, seen)
    assert case(3, 30, 0, 16)[1]['plan']['tree_in_lds'] and not case(3, 40, 0, 16)[1]['plan']['tree_in_lds']
    assert case(8, 12, 0, 16)[1]['plan']['tree_in_lds'] and not case(8, 40, 0, 16)[1]['plan']['tree_in_lds']


def edited(net64, edit):
    net = copy_net(net64, torch.float64)
    with torch.no_grad():
        edit(net)
    return net.eval()


def test_a_degenerate_state_takes_the_clamp():
    """dyn2 = (0, 0.3): t is constant, hi - lo = 0 < 1e-5 and the scaled state is 0 / 1e-5 = 0 exactly; the heads see f(0)."""
    def flat(net):
        net.dyn2.weight.zero_()
        net.dyn2.bias.fill_(0.3)

    net64 = edited(rolled_net(3, 0), flat)
    search = Search(net64, 30, 16)
    out = search.run()
    search.close()
    sd = twin.state_dict64(net64)
    want, got, err, yard = compare('degenerate A=3 n_sims=30', out, sd)
    assert (want.t == 0.3).all() and (want.next_state == 0.0).all()
    assert (got[0] == 0.0).all()
    assert_within('degenerate', err, yard)
    assert_probabilities(got, 3)
    f0 = twin.recurrent(sd, np.zeros((1, 64)), np.zeros(1, dtype=np.int64))   # (the prediction does not depend on the parent)
    assert np.abs(got[2] - f0.probs).max() <= YARDSTICK * yard[2] and np.abs(got[3] - f0.value).max() <= YARDSTICK * yard[3]


@pytest.mark.parametrize('A,n_sims', [(3, 30), (8, 40)])
def test_a_saturated_policy(A, n_sims):
    """pol.weight x 128: the twin's logits span more than 110 in some rows, where float32 expf(logit - max) is exactly 0."""
    net64 = edited(rolled_net(A, 16), lambda net: net.pol.weight.mul_(128.0))
    search = Search(net64, n_sims, 16)
    out = search.run()
    search.close()
    what = 'saturated A=%d n_sims=%d' % (A, n_sims)
    want, got, err, yard = compare(what, out, twin.state_dict64(net64))
    with np.errstate(divide='ignore'):
        span = np.log(want.probs.max(axis=1)) - np.log(want.probs.min(axis=1))
    print('%s: the twin\'s logits span up to %.1f, more than 110 in %d of %d rows' % (what, span.max(), int((span > 110.0).sum()), span.size))
    assert (span > 110.0).any()
    assert (got[2][want.probs < 2.0 ** -150] == 0.0).all()   # (below half the smallest float32: zero however expf rounds)
    assert_within(what, err, yard)
    assert_probabilities(got, A)


@pytest.mark.parametrize('A', [3, 5])
def test_a_weight_reload_is_what_the_next_search_runs(A):
    net_a = rolled_net(A, 32)
    gen = torch.Generator().manual_seed(50 + A)

    def step(net):
        for p in net.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=gen, dtype=torch.float64))

    net_b = edited(net_a, step)
    search = Search(net_a, 30, 16)
    first = search.run()
    search.load(net_b)
    second = search.run()
    search.close()
    _, _, err, yard = compare('before the reload A=%d' % A, first, twin.state_dict64(net_a))
    assert_within('before the reload', err, yard)
    _, _, err, yard = compare('after the reload A=%d' % A, second, twin.state_dict64(net_b))
    assert_within('after the reload', err, yard)
    _, _, stale, _ = compare('after the reload, the old model', second, twin.state_dict64(net_a), report=False)
    assert all(s > 100.0 * y for s, y in zip(stale, yard) if y > 0.0)   # (the old weights are nowhere near: every quantity moved)


@pytest.mark.parametrize('A,n_sims', [(3, 30), (8, 40)])
def test_launch_shape_independence_away_from_two_actions(A, n_sims):
    """4, 8 or 16 games per workgroup (and the automatic choice): bit-identical visits, root values, hidden states and value sums."""
    search = Search(rolled_net(A, 48), n_sims, 16)
    got, placements = [], set()
    for gpw in (16, 8, 4, 0):
        search.tree.set_search_shape(gpw)
        search.start()
        search.tree.search_fused(search.hidden, n_sims)
        n, vsum, _, _ = search.tree.root_stats()
        got.append((search.tree.root_visits().clone(), n.clone(), vsum.clone(), search.hidden.clone(), search.tree.root_children('value_sum')))
        placements.add(search.tree.search_plan(False)['tree_in_lds'])
    search.tree.check()
    search.close()
    assert (got[0][1] == n_sims).all() and int(got[0][0].sum()) == GAMES * n_sims
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert torch.equal(a, b)
    if A == 8:
        assert placements == {True, False}   # (16 games of 8 x 41 + 1 nodes stay in HBM, 4 fit the LDS budget)
