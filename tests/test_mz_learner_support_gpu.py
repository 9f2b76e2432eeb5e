"""The fused MuZero learner with categorical heads (k_mzl_grad<R, true>; MuZeroAgent(fused_learner=True, support=S)) on the GPU against
the float64 twin: ``agent.support_losses`` -- the PyTorch route's own expressions -- under autograd on ``net.double()``.  The tolerance is
tests/test_mz_learner_host.py's yardstick, measured in the same test: 4 times the torch float32 route's own error against that twin.
Sharpened weights, targets across and beyond the support (tests/test_mz_learner_support_host.py), every third row masked from some
step on.  As tests/test_mz_learner_gpu.py, this file draws no stream and runs the trainer as a process of its own."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_mz_learner_gpu import LR, moments, on_device
from test_mz_learner_host import assert_losses_within_yardstick, assert_within_yardstick, flat
from test_mz_learner_support_host import support_batch, support_net, twin

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRAD_SHAPES = [(1, 1, 1, 1, 1), (5, 5, 2, 4, 20), (17, 5, 3, 6, 31), (9, 16, 8, 16, 31)]   # (n, K, A, D, S): tiles of 4 rows, and of 2 at K = 16


def agent_of(net64, K, max_batch, fused=True, weight_decay=1e-4, support=None):
    """A MuZeroAgent on the GPU holding float32 copies of ``net64``'s parameters (``support``: another S than the net's, no copy)."""
    from rlzero_amd.muzero import MuZeroAgent
    agent = MuZeroAgent(obs_dim=net64.obs_dim, n_actions=net64.n_actions, lr=LR, weight_decay=weight_decay, device=DEV, fused_learner=fused,
                        unroll_steps=K, max_batch=max_batch, value_transform=True, support=support or net64.support)
    if support is None:
        agent.net.load_state_dict({k: v.to(DEV, torch.float32) for k, v in net64.state_dict().items()})
    return agent


_refs = {}


def reference(n, K, A, D, S, weighted):
    """(net64, batch, weights, twin gradient and losses, torch-f32 gradient and losses) of a shape: computed once."""
    key = (n, K, A, D, S, weighted)
    if key not in _refs:
        net = support_net(D, A, S, seed=100 + n)
        batch, weights = support_batch(n, K, A, D, S, seed=n + K)
        weights = weights if weighted else None
        _refs[key] = (net, batch, weights) + twin(net, batch, weights) + twin(net, batch, weights, torch.float32, DEV)
    return _refs[key]


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('n,K,A,D,S', GRAD_SHAPES)
def test_grads_against_the_twin(n, K, A, D, S, weighted):
    net, batch, weights, want, want_losses, ref32, ref32_losses = reference(n, K, A, D, S, weighted)
    agent = agent_of(net, K, n)
    assert agent.fused.n_params == want.size
    before = flat(agent.net.parameters())
    db, dw = on_device(batch, weights)
    grad, out4 = agent.fused.grads(db, dw)
    again = agent.fused.grads(db, dw)
    assert torch.equal(grad, again[0]) and torch.equal(out4, again[1])   # the same call twice gives the same bits
    what = 'support grads %r%s' % ((n, K, A, D, S), ' weighted' if weighted else '')
    assert_within_yardstick(net, grad.cpu().numpy(), ref32, want, what)
    assert_losses_within_yardstick(out4.cpu().numpy(), ref32_losses, want_losses, what)
    assert agent.fused.poll_errors() == 0 and np.array_equal(before, flat(agent.net.parameters()))   # grads updates nothing
    agent.fused.close()


def twin_step(net, opt, batch, weights):
    """One update of the PyTorch route on the float64 twin itself (clip 5.0, then torch's single-tensor Adam) -> the gradient's norm."""
    from rlzero_amd.muzero.agent import support_losses
    tb = tuple(torch.from_numpy(a) if a.dtype == np.int64 else torch.from_numpy(a).double() for a in batch)
    opt.zero_grad()
    support_losses(net, *tb, torch.from_numpy(weights).double())[0].backward()
    norm = float(torch.nn.utils.clip_grad_norm_(net.parameters(), 5.0))
    opt.step()
    return norm


def assert_state_within_yardstick(hip, ref, net64, opt64, what):
    assert_within_yardstick(net64, flat(hip.net.parameters()), flat(ref.net.parameters()), flat(net64.parameters()), what + ' parameters')
    for i, name in enumerate(('exp_avg', 'exp_avg_sq')):
        assert_within_yardstick(net64, getattr(hip.fused, name).cpu().numpy(), moments(ref.optimizer, ref.net)[i], moments(opt64, net64)[i], what + ' ' + name)


@pytest.mark.parametrize('loss_scale,clip_active', [(0.1, False), (3.0, True)])
def test_five_steps_on_five_batches(loss_scale, clip_active):
    """Parameters and both moments after five updates: twin (float64, CPU), the agent's PyTorch route (float32) and HIP from one start."""
    n, K, A, D, S = 33, 5, 2, 4, 20
    net64 = support_net(D, A, S, seed=21, gain=3.0)
    hip, ref = agent_of(net64, K, n), agent_of(net64, K, n, fused=False)
    opt64 = torch.optim.Adam(net64.parameters(), lr=LR, weight_decay=1e-4, foreach=False)
    for s in range(5):
        batch, weights = support_batch(n, K, A, D, S, seed=50 + s)
        weights = weights * np.float32(loss_scale)
        want = twin(net64, batch, weights)[1]
        norm = twin_step(net64, opt64, batch, weights)
        assert (norm > 5.0) == clip_active and not 4.0 < norm < 6.5, norm   # (far from the threshold either way)
        got32 = np.array(ref.learn(batch, weights=weights))
        assert_losses_within_yardstick(hip.learn_async(*on_device(batch, weights)).cpu().numpy(), got32, want, 'support step %d' % s)
    hip.check()
    assert hip.fused.step_count == 5
    assert_state_within_yardstick(hip, ref, net64, opt64, 'support five steps, clip %s' % clip_active)
    hip.fused.close()


@pytest.mark.parametrize('fused_saves', [True, False])
def test_a_checkpoint_moves_between_the_routes(tmp_path, fused_saves):
    """Two steps on one route, save, load into the other route, the float64 twin and a PyTorch-route agent; one more step each."""
    n, K, A, D, S = 33, 5, 2, 4, 20
    net0 = support_net(D, A, S, seed=51)
    saver = agent_of(net0, K, n, fused=fused_saves)
    for s in range(2):
        saver.learn(*support_batch(n, K, A, D, S, seed=70 + s))
    path = str(tmp_path / 'mz.pt')
    saver.save_model(path)
    loader, ref = agent_of(net0, K, n, fused=not fused_saves), agent_of(net0, K, n, fused=False)
    loader.load_model(path), ref.load_model(path)
    with pytest.raises(ValueError, match='support'):   # a checkpoint of another S
        agent_of(net0, K, n, support=S - 1).load_model(path)
    ck = torch.load(path, map_location='cpu')
    assert ck['support'] == S and [tuple(e['exp_avg'].shape) for e in ck['optimizer']['state'].values()][-2:] == [(2 * S + 1, 64), (2 * S + 1, )]
    net64 = support_net(D, A, S, seed=51)
    net64.load_state_dict({k: v.double() for k, v in ck['model'].items()})
    opt64 = torch.optim.Adam(net64.parameters(), lr=LR, weight_decay=1e-4, foreach=False)
    opt64.load_state_dict(ck['optimizer'])
    batch, weights = support_batch(n, K, A, D, S, seed=80)
    want = twin(net64, batch, weights)[1]
    twin_step(net64, opt64, batch, weights)
    got32 = np.array(ref.learn(batch, weights=weights))
    hip = loader if fused_saves is False else saver   # (the fused side takes the step from the state it loaded, or the one it saved)
    assert_losses_within_yardstick(np.array(hip.learn(batch, weights=weights)), got32, want, 'support checkpoint')
    assert hip.fused.step_count == 3
    assert_state_within_yardstick(hip, ref, net64, opt64, 'support checkpoint')
    if fused_saves:
        assert np.array(loader.learn(batch, weights=weights)).tolist() == got32.tolist()   # (torch read the fused file as it reads its own)
    hip.fused.close()


def test_the_trainer_runs_fused_with_a_support_and_refuses_whole_moves():
    script = os.path.join(REPO, 'tools', 'train_muzero.py')
    args = ['--value-transform', '--support', '20', '--device-replay', '--fused-learner', '--env', 'acrobot', '--max-episode-steps', '12', '--envs', '40',
            '--sims', '10', '--batch-size', '32', '--updates-per-iteration', '2', '--iterations', '2']
    runs = [subprocess.Popen([sys.executable, script] + args + more, stdout=subprocess.PIPE, stderr=subprocess.PIPE) for more in ([], ['--whole-moves'])]
    (out, err), (_, refused) = (proc.communicate() for proc in runs)
    assert runs[0].returncode == 0, err.decode()[-2000:]
    lines = [re.search(r'loss:(\S+), value:(\S+), reward:(\S+), policy:([^,\s]+)', line) for line in out.decode().splitlines() if line.startswith('batch i:')]
    assert len(lines) == 2 and all(m and all(math.isfinite(float(x)) for x in m.groups()) for m in lines), out.decode()
    assert runs[1].returncode != 0 and 'whole moves keep scalar heads' in refused.decode()


def test_the_entry_point_refuses_a_support_past_31():
    import ctypes
    from rlzero_amd import _hip
    lib, handle = _hip.load(), ctypes.c_void_p()
    cfg = _hip.RzMzLearnerConfig(_hip.ABI_VERSION, 4, 2, 64, 5, 32, 0, 32, LR, 1e-4, 0.9, 0.999, 1e-8, 5.0)
    assert lib.rz_mz_learner_create(ctypes.byref(cfg), ctypes.byref(handle)) == -1 and not handle.value   # RZ_ERR_ARG
    assert b'support 32' in lib.rz_last_error()
