"""rz_mz_learn.h with a support on the CPU: ``mzl_row_grad<T>(..., S)`` (plain and under the sanitizers, tests/host_driver.py) against
torch float64 autograd of ``agent.support_losses`` -- the PyTorch route's own expressions on ``net.double()``.  <double> to 1e-11;
<float> inside the yardstick of tests/test_mz_learner_host.py (4 times the torch-f32 route's own error against the same twin)."""
import numpy as np
import pytest
import torch

import host_driver
from rlzero_amd.muzero import support as sup
from rlzero_amd.muzero.agent import support_losses
from rlzero_amd.muzero.network import MuZeroNet
from test_mz_learner_host import YARDSTICK, as_torch, assert_losses_within_yardstick, assert_within_yardstick, flat, make_batch, tensor_slices

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rz_mz_learn.h"
namespace rl = rzmzl;
template <typename T> static std::vector<T> load(const char *p) {
    FILE *f = fopen(p, "rb"); if (!f) exit(2);
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)n / sizeof(T)); if (n && fread(v.data(), 1, (size_t)n, f) != (size_t)n) exit(2); fclose(f); return v;
}
template <typename T> static void store(const char *p, const std::vector<T> &v) { FILE *f = fopen(p, "wb"); if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2); fclose(f); }
// D A K n S params obs actions.i64 tv tr tp mask weights -> grad [P], losses [4] (means)
template <typename T> static int grad(char **a) {
    const int D = atoi(a[0]), A = atoi(a[1]), K = atoi(a[2]), n = atoi(a[3]), S = atoi(a[4]);
    int off[RZ_MZL_TENSORS + 1];
    rl::tensor_offsets(D, A, off, S);
    const auto params = load<T>(a[5]), obs = load<T>(a[6]), tv = load<T>(a[8]), tr = load<T>(a[9]), tp = load<T>(a[10]), mask = load<T>(a[11]), w = load<T>(a[12]);
    const auto actions = load<int64_t>(a[7]);
    if ((int)params.size() != off[RZ_MZL_TENSORS]) return 4;
    std::vector<std::vector<T>> tensors;   // (each tensor and each row in an allocation of its own size: an overread is the sanitizer's to report)
    const T *ptrs[RZ_MZL_TENSORS];
    for (int t = 0; t < RZ_MZL_TENSORS; ++t) tensors.emplace_back(params.begin() + off[t], params.begin() + off[t + 1]);
    for (int t = 0; t < RZ_MZL_TENSORS; ++t) ptrs[t] = tensors[t].data();
    std::vector<T> g(params.size(), (T)0), losses(4, (T)0);
    int bad = 0;
    for (int b = 0; b < n; ++b) {
        const std::vector<T> o(obs.begin() + b * D, obs.begin() + (b + 1) * D), v(tv.begin() + b * (K + 1), tv.begin() + (b + 1) * (K + 1)),
            r(tr.begin() + b * (K + 1), tr.begin() + (b + 1) * (K + 1)), p(tp.begin() + b * (K + 1) * A, tp.begin() + (b + 1) * (K + 1) * A),
            m(mask.begin() + b * (K + 1), mask.begin() + (b + 1) * (K + 1));
        const std::vector<long long> ac(actions.begin() + b * K, actions.begin() + (b + 1) * K);
        rl::mzl_row_grad<T>(D, A, K, ptrs, o.data(), ac.data(), v.data(), r.data(), p.data(), m.data(), w[b], n, g.data(), losses.data(), &bad, S);
    }
    for (int i = 0; i < 4; ++i) losses[i] /= (T)n;
    store(a[13], g); store(a[14], losses);
    return bad;
}
int main(int argc, char **argv) {
    if (argc != 17) return 4;
    return argv[1][4] == '6' ? grad<double>(argv + 2) : grad<float>(argv + 2);
}
'''
drv = host_driver.fixture('mz_learn_support', DRIVER)
SHAPES = [(1, 1, 1, 1, 1), (5, 5, 2, 4, 20), (3, 16, 8, 16, 31)]   # (n, K, A, D, S)


def support_net(D, A, S, seed, gain=2.0, dtype=torch.float64):
    """test_mz_learner_host.sharp_net with categorical heads: weights at ``gain`` times torch's initialisation, wide biases."""
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = MuZeroNet(D, A, 64, value_transform=True, support=S).to(dtype)
    with torch.no_grad():
        for name, p in net.named_parameters():
            p.mul_(gain) if name.endswith('weight') else p.copy_(torch.randn(p.shape, generator=gen, dtype=dtype) * 0.3)
    return net


def support_batch(n, K, A, D, S, seed):
    """make_batch with targets across the support, among them exact integers, exactly +-S, values beyond +-S and a value one float32
    ulp below an integer (the first entries of the value and, mirrored, of the reward targets)."""
    batch, weights = make_batch(n, K, A, D, seed, target_scale=S / 2.0)
    f = np.float32
    mix = np.array([S, -S, S + 2.5, -S - 0.25, 0.0, 1 - S, np.nextafter(f(S - 1), f(0)), np.nextafter(f(0), f(-1))], dtype=f)
    for t, m in ((batch[2], mix), (batch[3], -mix[::-1])):
        flat_t = t.reshape(-1)
        flat_t[:min(len(m), flat_t.size)] = m[:flat_t.size]
    return batch, weights


def twin(net, batch, weights, dtype=torch.float64, device='cpu', losses=support_losses):
    """-> (flat gradient, the four loss means) of ``losses`` under autograd on a copy of ``net`` in ``dtype``."""
    copy = MuZeroNet(net.obs_dim, net.n_actions, 64, value_transform=True, support=net.support).to(device, dtype)
    copy.load_state_dict({k: v.to(device, dtype) for k, v in net.state_dict().items()})
    tb, tw = as_torch(batch, weights, dtype, device)
    loss, lv, lr_, lp = losses(copy, *tb, tw)
    return flat(torch.autograd.grad(loss, list(copy.parameters()))), np.array([float(x.detach().mean()) for x in (loss, lv, lr_, lp)])


def driver_grad(drv, net, batch, weights, kind):
    dt = np.float64 if kind == 'grad64' else np.float32
    (obs, actions, tv, tr, tp, mask), (n, K) = batch, batch[1].shape
    w = np.ones(n, dtype=dt) if weights is None else weights.astype(dt)
    return drv.run(kind, [net.obs_dim, net.n_actions, K, n, net.support],
                   [flat(net.parameters()).astype(dt), obs.astype(dt), actions, tv.astype(dt), tr.astype(dt), tp.astype(dt), mask.astype(dt), w], [dt, dt])


@pytest.mark.parametrize('n,K,A,D,S', SHAPES)
@pytest.mark.parametrize('weighted', [False, True])
def test_row_grad_double_equals_the_twin(drv, n, K, A, D, S, weighted):
    net = support_net(D, A, S, seed=100 + n)
    batch, weights = support_batch(n, K, A, D, S, seed=n + K)
    weights = weights if weighted else None
    want, want_losses = twin(net, batch, weights)
    got, losses = driver_grad(drv, net, batch, weights, 'grad64')
    for name, sl in tensor_slices(net):
        scale = np.abs(want[sl]).max()
        assert scale > 0.0 or (A == 1 and name.startswith('pol')), name   # (one action: the policy loss is constant)
        assert np.abs(got[sl] - want[sl]).max() <= 1e-11 * scale, name
    assert np.abs(losses - want_losses).max() <= 1e-11 * np.abs(want_losses).max()


@pytest.mark.parametrize('n,K,A,D,S', SHAPES)
def test_row_grad_float_stands_inside_the_yardstick(drv, n, K, A, D, S):
    net = support_net(D, A, S, seed=100 + n)
    batch, weights = support_batch(n, K, A, D, S, seed=n + K)
    want, want_losses = twin(net, batch, weights)
    ref32, ref32_losses = twin(net, batch, weights, torch.float32)
    got, losses = driver_grad(drv, net, batch, weights, 'grad32')
    assert_within_yardstick(net, got, ref32, want, 'row_grad<float> %r' % ((n, K, A, D, S), ))
    assert_losses_within_yardstick(losses, ref32_losses, want_losses, 'row_grad<float> %r' % ((n, K, A, D, S), ))


def test_the_tolerance_catches_a_dropped_quarter_and_a_misplaced_bin(monkeypatch):
    """The twin without the 0.25 on the value loss, and with w_hi on the bin below lo instead of the one above, each lands more than
    100 tolerances from the true gradient (measured: 2.6e6 and 6.5e5), the tolerance being the yardstick of these inputs."""
    n, K, A, D, S = 5, 5, 2, 4, 20
    net = support_net(D, A, S, seed=11)
    batch, weights = support_batch(n, K, A, D, S, seed=12)
    true, _ = twin(net, batch, weights)
    tol = YARDSTICK * np.abs(twin(net, batch, weights, torch.float32)[0] - true).max()

    def no_quarter(*args):
        loss, lv, lr_, lp = support_losses(*args)
        return ((lv + lr_ + lp) * args[-1]).mean(), lv, lr_, lp
    away = [np.abs(twin(net, batch, weights, losses=no_quarter)[0] - true).max()]

    def bin_below(y, S):   # two_hot_torch with w_hi on bin lo - 1
        y = y.detach().clamp(-float(S), float(S))
        idx, w_hi = torch.floor(y).long() + S, y - torch.floor(y)
        out = torch.zeros(y.shape + (2 * S + 1, ), dtype=y.dtype).scatter_(-1, idx.unsqueeze(-1), (1.0 - w_hi).unsqueeze(-1))
        return out.scatter_add_(-1, (idx - 1).clamp_min(0).unsqueeze(-1), w_hi.unsqueeze(-1))
    monkeypatch.setattr(sup, 'two_hot_torch', bin_below)
    away.append(np.abs(twin(net, batch, weights)[0] - true).max())
    print('away %r, tolerance %.3e' % (away, tol))
    assert min(away) > 100.0 * tol
