"""The TWIN of the recurrent inference k_mz_search evaluates inside the kernel: rlzero_amd/muzero/network.py written out in plain
numpy on float64 arrays, no torch module involved.

``recurrent(sd, state, action)`` takes the model as a dict of float64 arrays under the names of ``MuZeroNet.state_dict()`` (torch
layout: weight [out][in]) and returns what ``MuZeroNet.recurrent_inference`` + softmax return, and the raw dyn2 output ``t`` (whose
arg-min / arg-max decide which wave of the kernel holds a game's extremes).

``perturb=`` names a WRONG variant -- each is a mistake the kernel or its weight upload could make -- for the sensitivity table of
tests/test_mz_search_net_host.py: a tolerance is worth what it catches."""
import collections

import numpy as np

H = 64
PERTURBATIONS = ('action_plus_one', 'last_action_column_zero', 'policy_rows_reversed', 'reward_without_relu', 'value_bias_dropped',
                 'extremes_of_48_units', 'softmax_over_8', 'dyn1_transposed_block')
QUANTITIES = ('next_state', 'reward', 'probs', 'value')
Recurrent = collections.namedtuple('Recurrent', QUANTITIES + ('t', ))


def exists(perturb, A):
    """Whether ``perturb`` differs from the definition at ``A`` actions at all."""
    if perturb in ('action_plus_one', 'last_action_column_zero', 'policy_rows_reversed', 'dyn1_transposed_block'):
        return A >= 2   # (one action: the same one-hot, and a [64][1] block is its own transpose; its only column is still needed)
    if perturb == 'softmax_over_8':
        return A < 8
    return True


def state_dict64(net):
    """The parameters of a MuZeroNet as float64 numpy arrays (copies)."""
    return {k: v.detach().cpu().double().numpy().copy() for k, v in net.state_dict().items()}


def relu(x):
    return np.maximum(x, 0.0)


def recurrent(sd, state, action, perturb=''):
    """state float64 [B, 64], action int [B] -> Recurrent(next_state [B, 64], reward [B], probs [B, A], value [B], t [B, 64])."""
    assert perturb == '' or perturb in PERTURBATIONS, perturb
    state = np.asarray(state, dtype=np.float64)
    action = np.asarray(action, dtype=np.int64)
    B = state.shape[0]
    w1 = sd['dyn1.weight']
    A = w1.shape[1] - H
    assert state.shape == (B, H) and action.shape == (B, ) and (action >= 0).all() and (action < A).all()
    if perturb == 'action_plus_one':
        action = (action + 1) % A
    if perturb == 'last_action_column_zero':
        w1 = w1.copy()
        w1[:, H + A - 1] = 0.0
    if perturb == 'dyn1_transposed_block':   # the [64][A] block of the action columns read as if it were stored [A][64]
        w1 = w1.copy()
        w1[:, H:] = np.ascontiguousarray(w1[:, H:]).reshape(A, H).T
    onehot = np.zeros((B, A), dtype=np.float64)
    onehot[np.arange(B), action] = 1.0
    x = np.concatenate((state, onehot), axis=1)
    h = relu(x @ w1.T + sd['dyn1.bias'])
    t = h @ sd['dyn2.weight'].T + sd['dyn2.bias']
    seen = t[:, :48] if perturb == 'extremes_of_48_units' else t
    lo = seen.min(axis=1, keepdims=True)
    hi = seen.max(axis=1, keepdims=True)
    nxt = (t - lo) / np.maximum(hi - lo, 1e-5)
    r1 = h @ sd['rew1.weight'].T + sd['rew1.bias']
    if perturb != 'reward_without_relu':
        r1 = relu(r1)
    reward = (r1 @ sd['rew2.weight'].T + sd['rew2.bias'])[:, 0]
    p = relu(nxt @ sd['pre1.weight'].T + sd['pre1.bias'])
    wp = sd['pol.weight'][::-1] if perturb == 'policy_rows_reversed' else sd['pol.weight']   # (the biases stay in their slots)
    logits = p @ wp.T + sd['pol.bias']
    if perturb == 'softmax_over_8':
        logits = np.concatenate((logits, np.zeros((B, 8 - A))), axis=1)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    probs = (e / e.sum(axis=1, keepdims=True))[:, :A]
    value = (p @ sd['val.weight'].T)[:, 0]
    if perturb != 'value_bias_dropped':
        value = value + sd['val.bias'][0]
    return Recurrent(nxt, reward, probs, value, t)


def extreme_blocks(t):
    """-> (counts of the arg-min's 16-unit block [4], of the arg-max's [4]) over the rows of ``t``: a block is one wave's rows."""
    return (np.bincount(t.argmin(axis=1) // 16, minlength=4), np.bincount(t.argmax(axis=1) // 16, minlength=4))
