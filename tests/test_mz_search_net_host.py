"""The float64 twin of k_mz_search's network (tests/mz_net_twin.py) on the CPU: that it IS the model, that the test nets reach every
wave's part of the min-max reduction, and what a tolerance of a few torch-float32 errors catches.

* The nets: ``sharp_net(6, A, seed=100 + A, gain=2.0)`` of tests/test_mz_learner_host.py at A = 1, 2, 3, 4, 5, 8 -- the softmax a
  constant, CartPole, Acrobot, a full quad of the one-hot, the first count that uses its second half (a = q + 4 j, j = 1) and the
  strided child scan, and KX = 72 with no padding row -- each in four variants: the rows of dyn2.weight / dyn2.bias rolled by 0, 16,
  32, 48 units, which moves the extremes of the unscaled next state from one wave's 16 rows to the next's.
* The inputs: a chain of 30 recurrent steps over 37 states from ``representation``, random actions, every step's input rounded to
  float32 first (what the kernel is given).
* The twin equals ``MuZeroNet.double().recurrent_inference`` to 1e-12 on every quantity.
* COVERAGE: per A, over the four variants, the arg-min and the arg-max of t fall in each of the four 16-unit blocks.  Without the
  rolls nearly every extreme of an A sits in one or two blocks, and the minimum taken over 48 units moved nothing at A = 5.
* SENSITIVITY: the yardstick of a quantity is torch float32 (CPU) against the twin; every wrong variant of the twin that exists at an
  A moves some quantity by at least 100 yardsticks -- tests/test_mz_search_net_gpu.py allows the kernel 4."""
import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import mz_net_twin as twin
from test_mz_learner_host import copy_net, sharp_net

ACTION_COUNTS = (1, 2, 3, 4, 5, 8)
ROLLS = (0, 16, 32, 48)
OBS_DIM, GAMES, CHAIN = 6, 37, 30

_nets = {}


def rolled_net(A, roll, gain=2.0):
    """The float64 test net of ``A`` actions with dyn2's output rows rolled by ``roll`` (cached: shared, never modified)."""
    key = (A, roll, gain)
    if key not in _nets:
        net = sharp_net(OBS_DIM, A, seed=100 + A, gain=gain)
        with torch.no_grad():
            net.dyn2.weight.copy_(torch.roll(net.dyn2.weight, roll, dims=0))
            net.dyn2.bias.copy_(torch.roll(net.dyn2.bias, roll, dims=0))
        _nets[key] = net.eval()
    return _nets[key]


def chain_inputs(net64, A, seed):
    """-> (states float32 [CHAIN * GAMES, 64], actions int64 [CHAIN * GAMES]): the inputs of a chain of recurrent steps."""
    rng = np.random.RandomState(seed)
    sd = twin.state_dict64(net64)
    with torch.no_grad():
        state = net64.representation(torch.from_numpy(rng.standard_normal((GAMES, OBS_DIM)))).numpy()
    states, actions = [], []
    for _ in range(CHAIN):
        state32 = state.astype(np.float32)
        action = rng.randint(A, size=GAMES).astype(np.int64)
        states.append(state32)
        actions.append(action)
        state = twin.recurrent(sd, state32.astype(np.float64), action).next_state
    return np.concatenate(states), np.concatenate(actions)


def torch_recurrent(net, states, actions):
    """``net.recurrent_inference`` + softmax in the net's own dtype and on its device -> the four quantities as float64 numpy arrays."""
    p = next(net.parameters())
    with torch.no_grad():
        nxt, reward, logits, value = net.recurrent_inference(torch.from_numpy(states).to(p.device, p.dtype), torch.from_numpy(actions).to(p.device))
        probs = torch.softmax(logits, dim=1)
    return tuple(x.double().cpu().numpy() for x in (nxt, reward, probs, value))


def errors(got, want):
    """Per quantity: max |got - want|."""
    return [float(np.abs(np.asarray(g, dtype=np.float64) - w).max()) for g, w in zip(got, want[:4])]


_cases = {}


def host_case(A, roll, gain=2.0):
    """(net64, state dict, states, actions, the twin's outputs) of a variant: computed once."""
    key = (A, roll, gain)
    if key not in _cases:
        net = rolled_net(A, roll, gain)
        states, actions = chain_inputs(net, A, seed=7 * A + roll)
        sd = twin.state_dict64(net)
        _cases[key] = (net, sd, states, actions, twin.recurrent(sd, states.astype(np.float64), actions))
    return _cases[key]


@pytest.mark.parametrize('A', ACTION_COUNTS)
def test_the_twin_is_the_model(A):
    for roll in ROLLS:
        net, sd, states, actions, want = host_case(A, roll)
        got = torch_recurrent(net, states.astype(np.float64), actions)
        for name, err in zip(twin.QUANTITIES, errors(got, want)):
            assert err <= 1e-12, (A, roll, name, err)
        assert want.probs.shape == (CHAIN * GAMES, A) and np.abs(want.probs.sum(axis=1) - 1.0).max() <= 1e-14
        assert want.next_state.min() == 0.0 and want.next_state.max() == 1.0
        assert 0.0 < np.abs(want.reward).max() and 0.0 < np.abs(want.value).max()


def assert_covered(A, ts, what):
    """The coverage condition over the unscaled next states ``ts`` of the four variants of ``A``; prints the counts."""
    lo_n, hi_n = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    for t in ts:
        a, b = twin.extreme_blocks(t)
        lo_n += a
        hi_n += b
    print('%s A=%d: arg-min of t per 16-unit block %s, arg-max %s' % (what, A, lo_n.tolist(), hi_n.tolist()))
    assert (lo_n >= 1).all() and (hi_n >= 1).all(), (what, A, lo_n, hi_n)
    return lo_n, hi_n


@pytest.mark.parametrize('A', ACTION_COUNTS)
def test_the_rolled_variants_put_extremes_in_every_waves_rows(A):
    assert_covered(A, [host_case(A, roll)[4].t for roll in ROLLS], 'host chain')


def sensitivity(A, gain=2.0):
    """-> (yardsticks per quantity, {perturbation: largest move in yardsticks}) over the four variants of ``A``."""
    yard, scale = np.zeros(4), np.zeros(4)
    moved = {p: np.zeros(4) for p in twin.PERTURBATIONS if twin.exists(p, A)}
    for roll in ROLLS:
        net, sd, states, actions, want = host_case(A, roll, gain)
        yard = np.maximum(yard, errors(torch_recurrent(copy_net(net, torch.float32), states, actions), want))
        scale = np.maximum(scale, [float(np.abs(w).max()) for w in want[:4]])
        for p in moved:
            moved[p] = np.maximum(moved[p], errors(twin.recurrent(sd, states.astype(np.float64), actions, perturb=p), want))
    yard = np.maximum(yard, 2.0 ** -23 * scale)   # (the floor of the GPU test: at A = 1 both evaluations give the probability 1.0 exactly)
    return yard, {p: float((m / yard).max()) for p, m in moved.items()}


@pytest.mark.parametrize('A', ACTION_COUNTS)
def test_every_wrong_variant_lands_100_yardsticks_away(A):
    """(gain 2.0 sufficed for every perturbation at every A: none was raised.)"""
    yard, moved = sensitivity(A)
    print('A=%d torch-f32 yardsticks: %s' % (A, ', '.join('%s %.2e' % (n, y) for n, y in zip(twin.QUANTITIES, yard))))
    for p in twin.PERTURBATIONS:
        print('A=%d %-24s %s' % (A, p, '%.3g yardsticks' % moved[p] if p in moved else 'does not exist at this A'))
    assert set(moved) == set(p for p in twin.PERTURBATIONS if twin.exists(p, A))
    assert len(moved) >= (4 if A == 1 else 7)
    for p, m in moved.items():
        assert m >= 100.0, (A, p, m)
