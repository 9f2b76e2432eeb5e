"""The arithmetic of the fused MuZero learner (rlzero_amd/csrc/rz_mz_learn.h) on the CPU, against torch autograd.

A driver with its own main is compiled against the header with ROCm's clang++ (by tests/host_driver.py),
-ffp-contract=off, fed binary inputs and compared with the TWIN: the expressions of ``MuZeroAgent.learn`` run by torch autograd on
float64 copies of the same parameters and batch (``twin_losses`` below restates them so that they can also be perturbed).

* ``mzl_row_grad<double>`` over small batches equals the twin to rounding (relative 1e-11): every scaling and every route of the
  math -- the 1 / K, the halved state gradient, the arg-min / arg-max terms of scale_hidden, the mask, the weights -- is pinned.
* The YARDSTICK of every float32 comparison (here and in tests/test_mz_learner_gpu.py): the error of the torch float32 route
  against the twin, measured in the same test.  Per parameter tensor the result under test may be at most 4 times the largest
  torch-f32 error anywhere in the flat vector away from the twin (both are f32 evaluations that differ in summation order), and each
  of the four losses at most 4 times the largest torch-f32 error among the four.
* The perturbation check shows what that tolerance catches: the twin with the 1 / K dropped, the halving dropped, the arg-min route
  cut, or the clip applied after the weight decay lands more than 100 tolerances away.
* The clip coefficient and the Adam element against torch's single-tensor Adam over 5 steps.
* The same driver built with -fsanitize=address,undefined and run as a stand-alone program over all inputs.
* The refusals of the limits, and the trainer's parser."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import host_driver
from rlzero_amd.muzero import network
from rlzero_amd.muzero.agent import MuZeroAgent, scale_gradient
from rlzero_amd.muzero.network import MuZeroNet

YARDSTICK = 4.0

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rz_mz_learn.h"

namespace rl = rzmzl;

template <typename T>
static std::vector<T> load(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (bytes && fread(v.data(), 1, (size_t)bytes, f) != (size_t)bytes) exit(2);
    fclose(f);
    return v;
}
template <typename T>
static void store(const char *path, const std::vector<T> &v) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror(path); exit(2); }
    fclose(f);
}

// grad D A K n use_weights params [P] obs [n][D] actions.i64 [n][K] tv tr [n][K+1] tp [n][K+1][A] mask [n][K+1] weights [n]
//   -> grad [P], losses [4] (means), bad.i32 [1]
template <typename T>
static int grad(char **a) {
    const int D = atoi(a[0]), A = atoi(a[1]), K = atoi(a[2]), n = atoi(a[3]), use_w = atoi(a[4]);
    int off[RZ_MZL_TENSORS + 1];
    rl::tensor_offsets(D, A, off);
    const int P = off[RZ_MZL_TENSORS];
    const std::vector<T> params = load<T>(a[5]), obs = load<T>(a[6]);
    const std::vector<int64_t> actions = load<int64_t>(a[7]);
    const std::vector<T> tv = load<T>(a[8]), tr = load<T>(a[9]), tp = load<T>(a[10]), mask = load<T>(a[11]), weights = load<T>(a[12]);
    if ((int)params.size() != P || (int)obs.size() != n * D || (int)actions.size() != n * K || (int)tv.size() != n * (K + 1) ||
        (int)tr.size() != n * (K + 1) || (int)tp.size() != n * (K + 1) * A || (int)mask.size() != n * (K + 1) || (int)weights.size() != n)
        return 4;
    // (heap copies of exactly each tensor's size: a read past a tensor's end is the sanitizer's to report)
    std::vector<std::vector<T>> tensors;
    const T *ptrs[RZ_MZL_TENSORS];
    for (int t = 0; t < RZ_MZL_TENSORS; ++t) tensors.emplace_back(params.begin() + off[t], params.begin() + off[t + 1]);
    for (int t = 0; t < RZ_MZL_TENSORS; ++t) ptrs[t] = tensors[t].data();
    std::vector<T> g((size_t)P, (T)0), losses(4, (T)0);
    std::vector<int32_t> bad(1, 0);
    for (int b = 0; b < n; ++b) {
        const std::vector<T> o(obs.begin() + b * D, obs.begin() + (b + 1) * D);
        const std::vector<long long> ac(actions.begin() + b * K, actions.begin() + (b + 1) * K);
        const std::vector<T> v(tv.begin() + b * (K + 1), tv.begin() + (b + 1) * (K + 1)), r(tr.begin() + b * (K + 1), tr.begin() + (b + 1) * (K + 1));
        const std::vector<T> p(tp.begin() + b * (K + 1) * A, tp.begin() + (b + 1) * (K + 1) * A), m(mask.begin() + b * (K + 1), mask.begin() + (b + 1) * (K + 1));
        int flag = 0;
        rl::mzl_row_grad<T>(D, A, K, ptrs, o.data(), ac.data(), v.data(), r.data(), p.data(), m.data(), use_w ? weights[b] : (T)1, n, g.data(),
                            losses.data(), &flag);
        bad[0] |= flag;
    }
    for (int i = 0; i < 4; ++i) losses[i] /= (T)n;
    store(a[13], g);
    store(a[14], losses);
    store(a[15], bad);
    return 0;
}

// adam steps hyper.f64 [lr wd b1 b2 eps max_norm] p0.f32 [N] grads.f32 [steps][N] -> p m v .f32 [N], coef.f32 [steps]
static int adam(char **a) {
    const int steps = atoi(a[0]);
    const std::vector<double> hy = load<double>(a[1]);
    std::vector<float> p = load<float>(a[2]);
    const std::vector<float> grads = load<float>(a[3]);
    const size_t N = p.size();
    if (hy.size() != 6 || grads.size() != N * steps) return 4;
    std::vector<float> m(N, 0.0f), v(N, 0.0f), coefs;
    for (int s = 1; s <= steps; ++s) {
        const float *g = grads.data() + (size_t)(s - 1) * N;
        float sq = 0.0f;
        for (size_t i = 0; i < N; ++i) sq += g[i] * g[i];
        const float coef = rl::clip_coef(sqrtf(sq), (float)hy[5]);
        coefs.push_back(coef);
        double b1s = 1.0, b2s = 1.0;
        for (int i = 0; i < s; ++i) b1s *= hy[2], b2s *= hy[3];
        rl::AdamStep<float> h;
        h.step_size = (float)(hy[0] / (1.0 - b1s)), h.bc2_sqrt = (float)sqrt(1.0 - b2s);
        h.w1 = (float)(1.0 - hy[2]), h.beta2 = (float)hy[3], h.w2 = (float)(1.0 - hy[3]), h.eps = (float)hy[4], h.weight_decay = (float)hy[1];
        for (size_t i = 0; i < N; ++i) rl::adam_elem(g[i] * coef, h, &p[i], &m[i], &v[i]);
    }
    store(a[4], p);
    store(a[5], m);
    store(a[6], v);
    store(a[7], coefs);
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "grad64" && argc == 18) return grad<double>(argv + 2);
    if (what == "grad32" && argc == 18) return grad<float>(argv + 2);
    if (what == "adam" && argc == 10) return adam(argv + 2);
    return 4;
}
'''


drv = host_driver.fixture('mz_learn', DRIVER)


# ----------------------------------------------------------------------------------------------- nets, batches, the twin
def sharp_net(D, A, seed, gain=2.0):
    """A float64 MuZeroNet on the CPU whose weights are ``gain`` times torch's initialisation and whose biases are drawn wide: the
    relu patterns differ from row to row, the states spread and no term of the gradient is negligible."""
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = MuZeroNet(D, A, 64).double()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith('weight'):
                p.mul_(gain)
            else:
                p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.3)
    return net


def make_batch(n, K, A, D, seed, target_scale=1.0):
    """The six numpy arrays of a mini-batch: every third row has mask 0 from some step on, with filler actions there."""
    rng = np.random.RandomState(seed)
    obs = rng.standard_normal((n, D)).astype(np.float32)
    actions = rng.randint(A, size=(n, K)).astype(np.int64)
    tv = (rng.standard_normal((n, K + 1)) * target_scale).astype(np.float32)
    tr = (rng.standard_normal((n, K + 1)) * target_scale).astype(np.float32)
    logits = rng.standard_normal((n, K + 1, A)) * 2.0
    tp = np.exp(logits - logits.max(axis=2, keepdims=True))
    tp = (tp / tp.sum(axis=2, keepdims=True)).astype(np.float32)
    mask = np.ones((n, K + 1), dtype=np.float32)
    for b in range(1, n, 3):
        end = 1 + (b // 3) % (K + 1)   # the first step past the episode's end: 1 .. K + 1
        mask[b, end:] = 0.0
        tv[b, end:] = 0.0
        tp[b, end:] = np.float32(1.0 / A)
    weights = rng.uniform(0.25, 3.0, size=n).astype(np.float32)
    return (obs, actions, tv, tr, tp, mask), weights


def as_torch(batch, weights, dtype, device='cpu'):
    obs, actions, tv, tr, tp, mask = (torch.from_numpy(a).to(device) for a in batch)
    w = None if weights is None else torch.from_numpy(weights).to(device, dtype)
    return (obs.to(dtype), actions, tv.to(dtype), tr.to(dtype), tp.to(dtype), mask.to(dtype)), w


def twin_losses(net, batch, weights=None, perturb=''):
    """The expressions of MuZeroAgent.learn -> (loss, lv.mean(), lr.mean(), lp.mean()).  ``perturb``: '' (the definition),
    'no_1_over_K', 'no_half' or 'argmin_cut' (no gradient to the arg-min element of scale_hidden) -- wrong on purpose."""
    obs, actions, tv, tr, tp, mask = batch
    K = actions.shape[1]
    keep = network.scale_hidden
    if perturb == 'argmin_cut':
        def cut(s):
            lo = s.min(dim=1, keepdim=True)[0]
            hi = s.max(dim=1, keepdim=True)[0]
            return (s - lo.detach()) / (hi - lo.detach()).clamp_min(1e-5)
        network.scale_hidden = cut
    try:
        state, logits, value = net.initial_inference(obs)
        lv = F.mse_loss(value, tv[:, 0], reduction='none')
        lr_ = torch.zeros_like(lv)
        lp = -(tp[:, 0] * F.log_softmax(logits, dim=1)).sum(dim=1) * mask[:, 0]
        for k in range(1, K + 1):
            state, reward, logits, value = net.recurrent_inference(state, actions[:, k - 1])
            g = 1.0 if perturb == 'no_1_over_K' else 1.0 / K
            lv = lv + scale_gradient(F.mse_loss(value, tv[:, k], reduction='none'), g)
            lr_ = lr_ + scale_gradient(F.mse_loss(reward, tr[:, k], reduction='none'), g)
            lp = lp + scale_gradient(-(tp[:, k] * F.log_softmax(logits, dim=1)).sum(dim=1) * mask[:, k], g)
            if perturb != 'no_half':
                state = scale_gradient(state, 0.5)
    finally:
        network.scale_hidden = keep
    if weights is None:
        loss = (0.25 * lv + lr_ + lp).mean()
    else:
        loss = ((0.25 * lv + lr_ + lp) * weights).mean()
    return loss, lv.mean(), lr_.mean(), lp.mean()


def flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).cpu().numpy()


def twin_grad(net, batch, weights=None, perturb=''):
    """-> (flat gradient, the four losses) as numpy arrays of the net's dtype."""
    losses = twin_losses(net, batch, weights, perturb)
    grads = torch.autograd.grad(losses[0], list(net.parameters()))
    return flat(grads), np.array([float(x.detach()) for x in losses])


def copy_net(net, dtype, device='cpu'):
    out = MuZeroNet(net.obs_dim, net.n_actions, net.hidden).to(device, dtype)
    out.load_state_dict({k: v.to(device, dtype) for k, v in net.state_dict().items()})
    return out


def tensor_slices(net):
    at, out = 0, []
    for name, p in net.named_parameters():
        out.append((name, slice(at, at + p.numel())))
        at += p.numel()
    return out


def assert_within_yardstick(net, got, ref32, twin, what, report=None):
    """Per parameter tensor: max |got - twin| <= 4 max |ref32 - twin| (the latter over the whole flat vector)."""
    got, ref32, twin = (np.asarray(a, dtype=np.float64) for a in (got, ref32, twin))
    assert np.isfinite(got).all(), what
    yard = float(np.abs(ref32 - twin).max())
    assert yard > 0.0, what
    worst = 0.0
    for name, sl in tensor_slices(net):
        err = float(np.abs(got[sl] - twin[sl]).max())
        worst = max(worst, err)
        print('%s %s: error %.3e, torch-f32 yardstick %.3e' % (what, name, err, yard))
        assert err <= YARDSTICK * yard, (what, name, err, yard)
    if report is not None:
        report.append((what, worst, yard))
    return worst, yard


def assert_losses_within_yardstick(got, ref32, twin, what, report=None):
    got, ref32, twin = (np.asarray(a, dtype=np.float64) for a in (got, ref32, twin))
    yard = float(np.abs(ref32 - twin).max())
    err = np.abs(got - twin)
    print('%s losses: errors %s, torch-f32 errors %s' % (what, err, np.abs(ref32 - twin)))
    assert np.isfinite(got).all() and yard > 0.0 and (err <= YARDSTICK * yard).all(), (what, err, yard)
    if report is not None:
        report.append((what + ' losses', float(err.max()), yard))


def driver_grad(drv, net, batch, weights, kind):
    dt = np.float64 if kind == 'grad64' else np.float32
    obs, actions, tv, tr, tp, mask = batch
    n, K = actions.shape
    params = flat(net.parameters()).astype(dt)
    w = np.ones(n, dtype=dt) if weights is None else weights.astype(dt)
    g, losses, bad = drv.run(kind, [net.obs_dim, net.n_actions, K, n, int(weights is not None)],
                             [params, obs.astype(dt), actions, tv.astype(dt), tr.astype(dt), tp.astype(dt), mask.astype(dt), w], [dt, dt, np.int32])
    return g, losses, int(bad[0])


SHAPES = [(1, 1, 2, 4), (5, 3, 3, 6), (9, 5, 2, 4), (4, 16, 8, 16)]   # (n, K, A, D)


# ----------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize('n,K,A,D', SHAPES)
@pytest.mark.parametrize('weighted', [False, True])
def test_row_grad_double_equals_the_twin(drv, n, K, A, D, weighted):
    net = sharp_net(D, A, seed=100 + n)
    batch, weights = make_batch(n, K, A, D, seed=n + K)
    weights = weights if weighted else None
    tb, tw = as_torch(batch, weights, torch.float64)
    want, want_losses = twin_grad(net, tb, tw)
    got, losses, bad = driver_grad(drv, net, batch, weights, 'grad64')
    assert bad == 0
    for name, sl in tensor_slices(net):
        scale = np.abs(want[sl]).max()
        assert scale > 0.0, name   # no tensor's gradient is negligible, let alone absent
        assert np.abs(got[sl] - want[sl]).max() <= 1e-11 * scale, name
    assert np.abs(losses - want_losses).max() <= 1e-11 * np.abs(want_losses).max()


@pytest.mark.parametrize('n,K,A,D', SHAPES)
def test_row_grad_float_stands_inside_the_yardstick(drv, n, K, A, D):
    net = sharp_net(D, A, seed=100 + n)
    batch, weights = make_batch(n, K, A, D, seed=n + K)
    want, want_losses = twin_grad(net, *as_torch(batch, weights, torch.float64))
    ref32, ref32_losses = twin_grad(copy_net(net, torch.float32), *as_torch(batch, weights, torch.float32))
    got, losses, bad = driver_grad(drv, net, batch, weights, 'grad32')
    assert bad == 0
    assert_within_yardstick(net, got, ref32, want, 'row_grad<float> %r' % ((n, K, A, D), ))
    assert_losses_within_yardstick(losses, ref32_losses, want_losses, 'row_grad<float> %r' % ((n, K, A, D), ))


def test_an_action_out_of_range_is_flagged_and_indexes_nothing(drv):
    net = sharp_net(4, 2, seed=3)
    batch, _ = make_batch(3, 2, 2, 4, seed=5)
    for wrong in (-1, 2, 2 ** 40):
        bad_batch = tuple(a.copy() for a in batch)
        bad_batch[1][1, 1] = wrong
        g, _, bad = driver_grad(drv, net, bad_batch, None, 'grad64')   # (the sanitized build reads no weight row outside dyn1)
        assert bad == 1 and np.isfinite(g).all()


def clipped(g, max_norm=5.0):
    norm = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    return g * min(1.0, max_norm / (norm + 1e-6))


def test_the_tolerance_catches_every_wrong_term():
    """Each perturbed twin lands more than 100 tolerances from the true gradient, the tolerance being the yardstick of these inputs.
    Measured here: the 1 / K dropped 6e6 tolerances away, the halving and the arg-min route 1e4 .. 1e5, the clip after the weight
    decay 277 -- the narrowest, a term of size weight_decay * |p|: it is 99 with weights at twice torch's initialisation and
    clears 100 from three times on, which is what this test and the GPU tests of the update use."""
    n, K, A, D = 9, 5, 2, 4
    net = sharp_net(D, A, seed=11, gain=3.0)
    batch, weights = make_batch(n, K, A, D, seed=12, target_scale=8.0)   # (large targets: the clip is active below)
    tb, tw = as_torch(batch, weights, torch.float64)
    true, _ = twin_grad(net, tb, tw)
    ref32, _ = twin_grad(copy_net(net, torch.float32), *as_torch(batch, weights, torch.float32))
    tol = YARDSTICK * np.abs(ref32 - true).max()
    for perturb in ('no_1_over_K', 'no_half', 'argmin_cut'):
        wrong, _ = twin_grad(net, tb, tw, perturb)
        away = np.abs(wrong - true).max()
        print('%s: %.3e away, tolerance %.3e' % (perturb, away, tol))
        assert away > 100.0 * tol, perturb
    # the clip applied after the weight decay: what Adam is fed, against clip(g) + wd p
    wd = 1e-4
    p = flat(net.parameters())
    assert np.sqrt((true ** 2).sum()) > 5.0
    fed, fed_wrong = clipped(true) + wd * p, clipped(true + wd * p)
    tol_fed = YARDSTICK * np.abs(clipped(ref32.astype(np.float64)) - clipped(true)).max()
    print('clip after weight decay: %.3e away, tolerance %.3e' % (np.abs(fed - fed_wrong).max(), tol_fed))
    assert np.abs(fed - fed_wrong).max() > 100.0 * tol_fed


@pytest.mark.parametrize('weight_decay', [0.0, 1e-4])
@pytest.mark.parametrize('grad_scale', [0.01, 30.0])
def test_clip_and_adam_element_against_torch(drv, weight_decay, grad_scale):
    """Five steps of clip_grad_norm_(5.0) + Adam(foreach=False) on one float32 vector; ``grad_scale``: the clip inactive / active.
    Bound: every step rounds p once (|p| 2^-24 each way for either evaluation) and forms an update of size <= lr m / sqrt(v) ~ lr
    through six float32 operations (6 x 2^-24 relative each way); m and v are three roundings a step each."""
    N, steps, lr = 257, 5, 3e-3
    rng = np.random.RandomState(7)
    p0 = rng.standard_normal(N).astype(np.float32)
    grads = (rng.standard_normal((steps, N)) * grad_scale).astype(np.float32)
    hyper = np.array([lr, weight_decay, 0.9, 0.999, 1e-8, 5.0], dtype=np.float64)
    p, m, v, coefs = drv.run('adam', [steps], [hyper, p0, grads], [np.float32] * 4)
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([param], lr=lr, weight_decay=weight_decay, foreach=False, fused=False, capturable=False)
    for s in range(steps):
        param.grad = torch.from_numpy(grads[s].copy())
        norm = torch.nn.utils.clip_grad_norm_([param], 5.0)
        want_coef = min(1.0, 5.0 / (float(norm) + 1e-6))
        assert (want_coef < 1.0) == (grad_scale > 1.0)
        assert abs(float(coefs[s]) - want_coef) <= 4 * 2.0 ** -24 * want_coef + 2.0 ** -24 * N ** 0.5 * want_coef   # (the norm: a sum of N squares)
        opt.step()
    st = opt.state[param]
    u = 2.0 ** -24
    assert np.abs(p - param.detach().numpy()).max() <= steps * (2 * u * np.abs(p0).max() + 2 * 12 * u * 10 * lr)
    assert np.abs(m - st['exp_avg'].numpy()).max() <= steps * 2 * 4 * u * np.abs(m).max() + u * N ** 0.5 * np.abs(m).max()
    assert np.abs(v - st['exp_avg_sq'].numpy()).max() <= steps * 2 * 4 * u * np.abs(v).max() + 2 * u * N ** 0.5 * np.abs(v).max()
    assert int(st['step']) == steps


@pytest.mark.parametrize('kwargs,names', [(dict(hidden=32), 'hidden'), (dict(hidden=128), 'hidden'), (dict(n_actions=9), 'n_actions'),
                                          (dict(unroll_steps=17), 'unroll_steps'), (dict(obs_dim=17), 'obs_dim'), (dict(obs_dim=0), 'obs_dim')])
def test_the_constructor_refuses_what_the_kernel_is_not_built_for(kwargs, names):
    """A ValueError that names the limit, before anything is allocated (no GPU is needed to be refused)."""
    with pytest.raises(ValueError, match=names):
        MuZeroAgent(fused_learner=True, **kwargs)


def test_learn_async_is_the_fused_routes():
    agent = MuZeroAgent(device='cpu')
    assert agent.fused is None and not agent.fused_learner
    with pytest.raises(RuntimeError, match='fused_learner=True'):
        agent.learn_async(None)


def test_the_trainers_flag_defaults_to_off():
    spec = importlib.util.spec_from_file_location('train_muzero', os.path.join(REPO, 'tools', 'train_muzero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args([]).fused_learner is False
    assert ap.parse_args(['--fused-learner']).fused_learner is True
    import inspect
    assert inspect.signature(mod.MuZeroPipeline.__init__).parameters['fused_learner'].default is False
    assert inspect.signature(MuZeroAgent.__init__).parameters['fused_learner'].default is False
