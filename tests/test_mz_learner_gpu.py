"""The fused MuZero learner (rz_mz_learner_*, rlzero_amd/muzero/learner.py) on the GPU, against the float64 twin.

Every comparison is between the HIP result and the TWIN of tests/test_mz_learner_host.py -- the expressions of
``MuZeroAgent.learn`` under torch autograd on float64 copies of the same parameters and batch (on the CPU) -- and the tolerance
is measured in the same test: the error of the existing torch float32 route (on the GPU) against that twin.  Per parameter
tensor the HIP result may be at most 4 times the largest torch-f32 error anywhere in the flat vector away from the twin, each
of the four losses at most 4 times the largest torch-f32 error among the four (test_mz_learner_host.py shows what a wrong term
does to that).  Sharpened weights (no gradient term is negligible); every third row has mask 0 from some step on.

This file takes NO stream from torch's default pool in the suite's process: the engine's lanes draw theirs from that pool in
turn (rlzero_amd/selfplay.py), which streams share a hardware queue depends on where the turn stands, and
tests/test_trace.py::test_trace_of_the_four_lane_layout measures the lanes' overlap.  Three draws here (a side stream, and the copy
stream of each of two in-process pipelines) moved the turn onto four streams that overlap too little for its bound.  So the
trainer runs as the command-line tool in processes of its own, and the side stream is a high-priority one (another pool)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_mz_learner_host import (as_torch, assert_losses_within_yardstick, assert_within_yardstick, copy_net, flat, make_batch, sharp_net,
                                  twin_grad, twin_losses)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LR = 3e-3
GRAD_SHAPES = [(1, 1, 2, 4), (7, 5, 2, 4), (16, 5, 2, 4), (17, 5, 3, 6), (256, 5, 2, 4), (64, 16, 8, 16)]   # (n, K, A, D)


def fused_agent(net64, K, max_batch, weight_decay=1e-4, fused=True):
    """A MuZeroAgent on the GPU holding float32 copies of ``net64``'s parameters."""
    from rlzero_amd.muzero import MuZeroAgent
    agent = MuZeroAgent(obs_dim=net64.obs_dim, n_actions=net64.n_actions, lr=LR, weight_decay=weight_decay, device=DEV, fused_learner=fused,
                        unroll_steps=K, max_batch=max_batch)
    agent.net.load_state_dict({k: v.to(DEV, torch.float32) for k, v in net64.state_dict().items()})
    return agent


def on_device(batch, weights):
    return tuple(torch.from_numpy(a).to(DEV) for a in batch), (None if weights is None else torch.from_numpy(weights).to(DEV))


_refs = {}


def reference(n, K, A, D, weighted):
    """(net64, batch, weights, twin gradient, twin losses, torch-f32 gradient, torch-f32 losses) of a shape: computed once."""
    key = (n, K, A, D, weighted)
    if key not in _refs:
        net = sharp_net(D, A, seed=100 + n)
        batch, weights = make_batch(n, K, A, D, seed=n + K)
        weights = weights if weighted else None
        want, want_losses = twin_grad(net, *as_torch(batch, weights, torch.float64))
        ref32, ref32_losses = twin_grad(copy_net(net, torch.float32, DEV), *as_torch(batch, weights, torch.float32, DEV))
        _refs[key] = (net, batch, weights, want, want_losses, ref32, ref32_losses)
    return _refs[key]


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('n,K,A,D', GRAD_SHAPES)
def test_grads_against_the_twin(n, K, A, D, weighted):
    net, batch, weights, want, want_losses, ref32, ref32_losses = reference(n, K, A, D, weighted)
    agent = fused_agent(net, K, n)
    before = flat(agent.net.parameters())
    grad, out4 = agent.fused.grads(*on_device(batch, weights))
    what = 'grads %r%s' % ((n, K, A, D), ' weighted' if weighted else '')
    assert_within_yardstick(net, grad.cpu().numpy(), ref32, want, what)
    assert_losses_within_yardstick(out4.cpu().numpy(), ref32_losses, want_losses, what)
    assert agent.fused.poll_errors() == 0 and agent.fused.step_count == 0
    assert np.array_equal(before, flat(agent.net.parameters()))   # grads updates nothing
    agent.fused.close()


def twin_optimizer(net, weight_decay):
    return torch.optim.Adam(net.parameters(), lr=LR, weight_decay=weight_decay, foreach=False)


def twin_step(net, opt, batch, weights):
    """One update of MuZeroAgent.learn on a torch net of any dtype / device (clip 5.0, then the optimizer)."""
    losses = twin_losses(net, batch, weights)
    opt.zero_grad()
    losses[0].backward()
    torch.nn.utils.clip_grad_norm_(net.parameters(), 5.0)
    opt.step()
    return np.array([float(x.detach()) for x in losses])


def moments(opt, net):
    return (flat([opt.state[p]['exp_avg'] for p in net.parameters()]), flat([opt.state[p]['exp_avg_sq'] for p in net.parameters()]))


@pytest.mark.parametrize('weight_decay', [0.0, 1e-4])
@pytest.mark.parametrize('loss_scale,clip_active', [(0.002, False), (3.0, True)])
def test_five_steps_on_five_batches(weight_decay, loss_scale, clip_active):
    """The parameters and both moments after five updates: twin (float64, CPU), torch float32 (the agent's PyTorch route) and HIP
    from one start.  ``loss_scale`` multiplies the importance weights, i.e. the loss: the clip inactive / active throughout."""
    n, K, A, D = 33, 5, 2, 4
    net64 = sharp_net(D, A, seed=21, gain=3.0)
    hip, ref = fused_agent(net64, K, n, weight_decay), fused_agent(net64, K, n, weight_decay, fused=False)
    opt64 = twin_optimizer(net64, weight_decay)
    for s in range(5):
        batch, weights = make_batch(n, K, A, D, seed=50 + s)
        weights = weights * np.float32(loss_scale)
        tb, tw = as_torch(batch, weights, torch.float64)
        norm = math.sqrt(sum(float((g ** 2).sum()) for g in torch.autograd.grad(twin_losses(net64, tb, tw)[0], list(net64.parameters()))))
        assert (norm > 5.0) == clip_active and not 4.0 < norm < 6.5, norm   # (far from the threshold either way)
        want = twin_step(net64, opt64, tb, tw)
        got32 = np.array(ref.learn(batch, weights=weights))
        got = hip.learn_async(*on_device(batch, weights)).cpu().numpy()
        assert_losses_within_yardstick(got, got32, want, 'step %d losses' % s)
    hip.check()
    assert hip.fused.step_count == 5
    what = 'five steps wd %g clip %s' % (weight_decay, clip_active)
    assert_within_yardstick(net64, flat(hip.net.parameters()), flat(ref.net.parameters()), flat(net64.parameters()), what + ' parameters')
    m64, v64 = moments(opt64, net64)
    m32, v32 = moments(ref.optimizer, ref.net)
    assert_within_yardstick(net64, hip.fused.exp_avg.cpu().numpy(), m32, m64, what + ' exp_avg')
    assert_within_yardstick(net64, hip.fused.exp_avg_sq.cpu().numpy(), v32, v64, what + ' exp_avg_sq')
    hip.fused.close()


@pytest.mark.parametrize('loss_scale', [0.002, 3.0])
def test_the_update_rule_alone(loss_scale):
    """HIP's own gradient in ``.grad`` of a float64 twin and of a float32 torch copy, torch's clip and Adam on both: HIP's step
    lands where the twin does, as closely as torch float32 does.  Two steps, so that the moments and the bias corrections of a
    step beyond the first take part."""
    n, K, A, D = 33, 5, 2, 4
    net64 = sharp_net(D, A, seed=22, gain=3.0)
    hip = fused_agent(net64, K, n)
    net32 = copy_net(net64, torch.float32, DEV)
    opt64, opt32 = twin_optimizer(net64, 1e-4), twin_optimizer(net32, 1e-4)
    for s in range(2):
        batch, weights = make_batch(n, K, A, D, seed=60 + s)
        db, dw = on_device(batch, weights * np.float32(loss_scale))
        # (the twins follow HIP's parameters step by step: only the update rule is compared)
        for twin, dtype in ((net64, torch.float64), (net32, torch.float32)):
            twin.load_state_dict({k: v.to(dtype) for k, v in hip.net.state_dict().items()})
        grad, _ = hip.fused.grads(db, dw)
        at = 0
        for p64, p32 in zip(net64.parameters(), net32.parameters()):
            g = grad[at:at + p64.numel()].view_as(p32)
            p64.grad, p32.grad = g.cpu().double(), g.clone()
            at += p64.numel()
        for twin, opt in ((net64, opt64), (net32, opt32)):
            torch.nn.utils.clip_grad_norm_(twin.parameters(), 5.0)
            opt.step()
        hip.learn_async(db, dw)
        what = 'update rule, step %d, loss scale %g' % (s, loss_scale)
        assert_within_yardstick(net64, flat(hip.net.parameters()), flat(net32.parameters()), flat(net64.parameters()), what + ' parameters')
        m64, v64 = moments(opt64, net64)
        m32, v32 = moments(opt32, net32)
        assert_within_yardstick(net64, hip.fused.exp_avg.cpu().numpy(), m32, m64, what + ' exp_avg')
        assert_within_yardstick(net64, hip.fused.exp_avg_sq.cpu().numpy(), v32, v64, what + ' exp_avg_sq')
    hip.fused.close()


def test_a_degenerate_state():
    """rep2 all zero: the raw state of step 0 is constant, hi - lo = 0 < 1e-5, the clamp is active and every element ties for
    arg-min and arg-max.  The losses and the gradients that no tie reaches -- pre1 / pol / val, whose step-0 part sees the scaled
    state 0 -- agree with the twin; everything is finite.  (rep1 / rep2 receive the gradient of the tied element: not compared.)"""
    n, K, A, D = 7, 5, 2, 4
    net = sharp_net(D, A, seed=31)
    with torch.no_grad():
        net.rep2.weight.zero_(), net.rep2.bias.zero_()
    batch, weights = make_batch(n, K, A, D, seed=32)
    want, want_losses = twin_grad(net, *as_torch(batch, weights, torch.float64))
    ref32, ref32_losses = twin_grad(copy_net(net, torch.float32, DEV), *as_torch(batch, weights, torch.float32, DEV))
    agent = fused_agent(net, K, n)
    grad, out4 = agent.fused.grads(*on_device(batch, weights))
    grad = grad.cpu().numpy()
    assert np.isfinite(grad).all()
    assert_losses_within_yardstick(out4.cpu().numpy(), ref32_losses, want_losses, 'degenerate state')
    at, compared = 0, []
    for name, p in net.named_parameters():
        if name.split('.')[0] in ('pre1', 'pol', 'val'):
            compared.append((name, slice(at, at + p.numel())))
        at += p.numel()
    yard = max(np.abs(ref32[sl] - want[sl]).max() for _, sl in compared)   # (the yardstick too leaves out what a tie decides)
    for name, sl in compared:
        err = np.abs(grad[sl] - want[sl]).max()
        print('degenerate state %s: error %.3e, torch-f32 yardstick %.3e' % (name, err, yard))
        assert np.abs(want[sl]).max() > 0.0 and err <= 4.0 * yard, name
    agent.fused.close()


def test_the_same_call_twice_gives_the_same_bits_on_any_stream():
    n, K, A, D = 256, 5, 2, 4
    net, batch, weights, *_ = reference(n, K, A, D, True)
    a, b = fused_agent(net, K, n), fused_agent(net, K, n)
    db, dw = on_device(batch, weights)
    g1, l1 = a.fused.grads(db, dw)
    g2, l2 = a.fused.grads(db, dw)
    assert torch.equal(g1, g2) and torch.equal(l1, l2)
    side = torch.cuda.Stream(device=DEV, priority=-1)   # (not one of the pool the engine's lanes draw their streams from in turn)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g3, l3 = a.fused.grads(db, dw)
        s_side = b.learn_async(db, dw)
    torch.cuda.current_stream().wait_stream(side)
    s_main = a.learn_async(db, dw)
    assert torch.equal(g1, g3) and torch.equal(l1, l3) and torch.equal(s_main, s_side) and torch.equal(s_main, l1)
    for p, q in zip(a.net.parameters(), b.net.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(a.fused.exp_avg, b.fused.exp_avg) and torch.equal(a.fused.exp_avg_sq, b.fused.exp_avg_sq)
    assert not torch.equal(a.fused.exp_avg, torch.zeros_like(a.fused.exp_avg))
    a.fused.close(), b.fused.close()


def test_a_fused_step_reaches_the_search():
    """The step raises every parameter's version: MuZeroSelfPlay._refresh_model sees another tuple, uploads again, and the search
    gives what an independent search object loaded with the new weights gives."""
    from rlzero_amd.muzero import CartPoleBatch, MuZeroSelfPlay
    n, K, A, D = 32, 5, 2, 4
    net = sharp_net(D, A, seed=41, gain=1.0)
    agent = fused_agent(net, K, n)
    sp = MuZeroSelfPlay(agent.net, CartPoleBatch(16, DEV, seed=5), n_sims=16, seed=2, fused_moves=False)
    obs = sp.env.observe().clone()
    before = sp.search(obs, add_noise=False)
    seen = sp._model_seen
    batch, weights = make_batch(n, K, A, D, seed=42, target_scale=4.0)
    for _ in range(3):
        agent.learn_async(*on_device(batch, weights))
    agent.check()
    assert tuple((p.data_ptr(), p._version) for p in agent.net.parameters()) != seen
    assert all(p._version > v for p, (_, v) in zip(agent.net.parameters(), seen))
    after = sp.search(obs, add_noise=False)
    assert sp._model_seen != seen
    fresh = MuZeroSelfPlay(agent.net, CartPoleBatch(16, DEV, seed=5), n_sims=16, seed=2, fused_moves=False)
    want = fresh.search(obs, add_noise=False)
    assert torch.equal(after[0], want[0]) and torch.equal(after[1], want[1])
    assert not torch.equal(after[1], before[1])   # (the weights did move the search)
    sp.close(), fresh.close(), agent.fused.close()


@pytest.mark.parametrize('fused_saves', [True, False])
def test_a_checkpoint_moves_between_the_routes(tmp_path, fused_saves):
    """Two steps on one route, save, load into the other route, a float64 twin and a torch float32 agent; one step each from that
    state: the route that loaded agrees with the twin as closely as torch float32 does."""
    n, K, A, D = 33, 5, 2, 4
    net0 = sharp_net(D, A, seed=51)
    saver = fused_agent(net0, K, n, fused=fused_saves)
    for s in range(2):
        batch, weights = make_batch(n, K, A, D, seed=70 + s, target_scale=4.0)
        saver.learn(on_device(batch, weights)[0], weights=weights)
    path = str(tmp_path / 'mz.pt')
    saver.save_model(path)
    ck = torch.load(path, map_location='cpu')
    assert sorted(ck['optimizer']) == ['param_groups', 'state'] and len(ck['optimizer']['state']) == 18
    assert all(float(e['step']) == 2.0 and e['step'].dtype == torch.float32 for e in ck['optimizer']['state'].values())
    assert [tuple(e['exp_avg'].shape) for e in ck['optimizer']['state'].values()] == [tuple(p.shape) for p in saver.net.parameters()]
    loader, ref = fused_agent(net0, K, n, fused=not fused_saves), fused_agent(net0, K, n, fused=False)
    loader.load_model(path), ref.load_model(path)
    fused_side = loader if loader.fused is not None else saver
    if loader.fused is not None:
        assert loader.fused.step_count == 2
    net64 = copy_net(net0, torch.float64)
    net64.load_state_dict({k: v.double() for k, v in ck['model'].items()})
    opt64 = twin_optimizer(net64, 1e-4)
    opt64.load_state_dict(ck['optimizer'])
    batch, weights = make_batch(n, K, A, D, seed=80, target_scale=4.0)
    want = twin_step(net64, opt64, *as_torch(batch, weights, torch.float64))
    got32 = np.array(ref.learn(batch, weights=weights))
    hip = loader if loader.fused is not None else None
    if hip is None:   # torch loaded a fused checkpoint: the fused saver takes the same step from the state it saved
        hip, got = saver, np.array(saver.learn(batch, weights=weights))
        assert np.array(loader.learn(batch, weights=weights)).tolist() == got32.tolist()   # (the same torch route from the same file)
    else:
        got = np.array(hip.learn(batch, weights=weights))
    assert_losses_within_yardstick(got, got32, want, 'checkpoint losses')
    assert_within_yardstick(net64, flat(hip.net.parameters()), flat(ref.net.parameters()), flat(net64.parameters()), 'checkpoint parameters')
    m64, v64 = moments(opt64, net64)
    m32, v32 = moments(ref.optimizer, ref.net)
    assert_within_yardstick(net64, hip.fused.exp_avg.cpu().numpy(), m32, m64, 'checkpoint exp_avg')
    assert_within_yardstick(net64, hip.fused.exp_avg_sq.cpu().numpy(), v32, v64, 'checkpoint exp_avg_sq')
    assert hip.fused.step_count == 3
    fused_side.fused.close()


LINE = re.compile(r'^batch i:(\d+), episodes:(\d+), episode_len:([\d.]+), loss:(\S+), value:(\S+), reward:(\S+), policy:(\S+?)(, reanalysed:(\d+))?$')
TRAINER_RUNS = {
    # MuZeroPipeline(n_envs=64, fused_learner=True, device_replay=True, prioritized_replay=True, reanalyse=64).run(3), as the tool
    'fused': ['--envs', '64', '--fused-learner', '--device-replay', '--prioritized-replay', '--reanalyse', '64', '--iterations', '3'],
    'off': ['--envs', '64', '--sims', '8', '--batch-size', '32', '--updates-per-iteration', '2', '--device-replay', '--iterations', '2'],
}


@pytest.fixture(scope='module')
def trainer_lines():
    """tools/train_muzero.py as the command-line tool, the two runs side by side in processes of their own (as
    tests/test_mz_reanalyse_gpu.py runs it: whole pipelines -- searches, their copy streams, a replay buffer -- leave nothing behind
    in the process the rest of the suite runs in) -> the 'batch i:' lines of each."""
    script = os.path.join(REPO, 'tools', 'train_muzero.py')
    runs = {name: subprocess.Popen([sys.executable, script] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE) for name, args in TRAINER_RUNS.items()}
    out = {}
    for name, proc in runs.items():
        stdout, stderr = proc.communicate()
        assert proc.returncode == 0, stderr.decode()[-2000:]
        out[name] = [line for line in stdout.decode().splitlines() if line.startswith('batch i:')]
    return out


def test_the_pipeline_runs_fused_with_everything_on(trainer_lines):
    lines = trainer_lines['fused']
    assert 1 <= len(lines) <= 3
    for line in lines:
        m = LINE.match(line)
        assert m and m.group(9) is not None and int(m.group(9)) == 64, line
        assert all(math.isfinite(float(m.group(i))) for i in (4, 5, 6, 7)), line


def test_the_pipeline_with_the_flag_off_prints_what_it_prints_today(trainer_lines):
    lines = trainer_lines['off']
    assert len(lines) == 2 and all(LINE.match(line) and ', reanalysed' not in line for line in lines), lines
    assert all(math.isfinite(float(LINE.match(line).group(i))) for line in lines for i in (4, 5, 6, 7))


def test_an_action_out_of_range_raises_and_changes_nothing():
    from rlzero_amd._hip import HipError
    n, K, A, D = 9, 5, 2, 4
    net = sharp_net(D, A, seed=61)
    agent = fused_agent(net, K, n)
    batch, weights = make_batch(n, K, A, D, seed=62)
    agent.learn_async(*on_device(batch, weights))
    agent.check()
    before = [p.clone() for p in agent.net.parameters()] + [agent.fused.exp_avg.clone(), agent.fused.exp_avg_sq.clone()]
    bad = tuple(a.copy() for a in batch)
    bad[1][4, 2] = A
    agent.learn_async(*on_device(bad, weights))
    agent.learn_async(*on_device(batch, weights))   # behind a refused update nothing is applied either, until the flag is read
    with pytest.raises(HipError, match='outside 0 .. 1'):
        agent.check()
    after = list(agent.net.parameters()) + [agent.fused.exp_avg, agent.fused.exp_avg_sq]
    assert all(torch.equal(x, y) for x, y in zip(before, after)) and agent.fused.step_count == 1
    agent.learn_async(*on_device(batch, weights))
    agent.check()
    assert agent.fused.step_count == 2 and not torch.equal(before[0], next(agent.net.parameters()))
    agent.fused.close()
