"""csrc/rz_mz_support.h on the CPU (plain and under the sanitizers: tests/host_driver.py) against the twin rlzero_amd/muzero/support.py
bit for bit; the packed head rows of csrc/rz_mz_pack.h; the model's option; ``MuZeroAgent.learn``'s cross-entropy under float64 autograd."""
import numpy as np
import pytest
import torch

import host_driver
from rlzero_amd.muzero import support as sup
from rlzero_amd.muzero.agent import MuZeroAgent
from rlzero_amd.muzero.network import MuZeroNet
from test_mz_learner_host import YARDSTICK, make_batch

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rz_mz_pack.h"
#include "rz_mz_support.h"
template <typename T> static std::vector<T> rd(const char *p) {
    FILE *f = fopen(p, "rb"); if (!f) exit(2);
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)n / sizeof(T)); if (n && fread(v.data(), 1, (size_t)n, f) != (size_t)n) exit(2); fclose(f); return v;
}
template <typename T> static void wr(const char *p, const std::vector<T> &v) { FILE *f = fopen(p, "wb"); if (!f) exit(2); fwrite(v.data(), sizeof(T), v.size(), f); fclose(f); }
int main(int argc, char **argv) {
    const int S = argc > 3 ? atoi(argv[2]) : 0, B = 2 * S + 1;
    if (!strcmp(argv[1], "two_hot")) {          // y f64 [n] -> lo i32 [n], (w_lo, w_hi) f64 [n][2], dense f64 [n][B]
        const auto y = rd<double>(argv[3]);
        std::vector<int> lo(y.size()); std::vector<double> w(2 * y.size()), d(y.size() * B);
        for (size_t i = 0; i < y.size(); ++i) { rzmzs::two_hot(y[i], S, &lo[i], &w[2 * i], &w[2 * i + 1]); rzmzs::dense(y[i], S, &d[i * B]); }
        wr(argv[4], lo); wr(argv[5], w); wr(argv[6], d);
    } else if (!strcmp(argv[1], "expect")) {    // logits f64 [n][B] -> f64 [n] (a row in its own allocation: an overread is a report)
        const auto x = rd<double>(argv[3]);
        std::vector<double> e(x.size() / B);
        for (size_t i = 0; i < e.size(); ++i) { std::vector<double> row(x.begin() + i * B, x.begin() + (i + 1) * B); e[i] = rzmzs::expectation(row.data(), S); }
        wr(argv[4], e);
    } else if (!strcmp(argv[1], "pack")) {      // val.w [B][64], val.b [B] -> the packed head: w [64][64], b [64]
        const auto w = rd<float>(argv[3]), b = rd<float>(argv[4]);
        const int A = 2;
        std::vector<float> z((64 + A) * 64, 0.25f);
        const float *p[14] = {z.data(), z.data(), z.data(), z.data(), z.data(), z.data(), w.data(), b.data(), z.data(), z.data(), z.data(), z.data(), w.data(), b.data()};
        const rzmp::Model m = rzmp::pack_model(p, A, S);
        std::vector<float> pw(m.host.begin() + m.off[12], m.host.begin() + m.off[12] + 64 * 64), pb(m.host.begin() + m.off[13], m.host.begin() + m.off[13] + 64);
        wr(argv[5], pw); wr(argv[6], pb);
    } else return 2;
    return 0;
}
'''
drv = host_driver.fixture('mz_support', DRIVER)


@pytest.mark.parametrize('S', (1, 20, 31))
def test_two_hot_equals_the_twin_bit_for_bit(drv, S):
    up, dn = np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)   # -S, S, beyond both ends, integers, -0.0, either side of an integer
    y = np.array([-S, S, -S - 0.5, S + 3.0, -1e300, 1e300, 0.0, -0.0, 1.0, -1.0, S - 1.0, up, dn, -up, -dn, np.nextafter(float(S), 0.0),
                  np.nextafter(-float(S), 0.0), 0.5, -0.25, S - 0.125, 1e-300], dtype=np.float64)
    lo, w, dense = drv.run('two_hot', [S], [y], [np.int32, np.float64, np.float64])
    t_lo, t_wlo, t_whi = sup.two_hot(y, S)
    assert np.array_equal(lo, t_lo) and np.array_equal(w.reshape(-1, 2).view(np.uint64), np.stack((t_wlo, t_whi), axis=1).view(np.uint64))
    assert np.array_equal(dense.view(np.uint64), sup.two_hot_dense(y, S).reshape(-1).view(np.uint64))
    assert lo.max() == 2 * S and (w[1::2][lo == 2 * S] == 0.0).all()   # at the end all weight on the last bin, none past it
    # expectation(two_hot(y)) gives y back inside the support: logits = log of the two weights, -800 elsewhere (a term of exactly 0)
    inside = y[np.abs(y) <= S]
    with np.errstate(divide='ignore'):
        logits = np.maximum(np.log(sup.two_hot_dense(inside, S)), -800.0)
    back, = drv.run('expect', [S], [logits], [np.float64])
    assert np.abs(back - inside).max() <= 1e-12


@pytest.mark.parametrize('S', (1, 20, 31))
def test_expectation_equals_the_twin_bit_for_bit(drv, S):
    B, rng = 2 * S + 1, np.random.RandomState(S)
    rows = [rng.standard_normal(B) * g for g in (0.1, 1.0, 20.0)] + [np.zeros(B), np.full(B, -3.5)]
    rows += [rng.uniform(0.0, 1.0, B) + 51.0 * (np.arange(B) == peak) for peak in (0, S, B - 1)]   # saturated: one logit 50 above the rest
    x = np.array(rows, dtype=np.float32)
    got, = drv.run('expect', [S], [x.astype(np.float64)], [np.float64])   # (float32 logits, widened as the kernel widens them)
    assert np.array_equal(got.view(np.uint64), sup.support_expectation(x, S).view(np.uint64))
    assert got[3] == 0.0 and got[4] == 0.0                       # all-equal logits: the support is symmetric
    assert np.abs(got[5:] - (np.array([0, S, B - 1]) - S)).max() <= 1e-15 * S + 2 * S * np.exp(-49.0) * B


@pytest.mark.parametrize('S', (1, 20, 31))
def test_packed_heads_padding_rows_give_a_term_of_exactly_zero(drv, S):
    B, rng = 2 * S + 1, np.random.RandomState(100 + S)
    w, b, act = (rng.standard_normal(s).astype(np.float32) for s in ((B, 64), (B, ), (64, )))
    pw, pb = drv.run('pack', [S], [w, b], [np.float32, np.float32])
    pw = pw.reshape(64, 64)                                       # k-major [k][bin]
    assert np.array_equal(pw[:, :B], w.T) and (pw[:, B:] == 0.0).all() and np.array_equal(pb[:B], b)
    logit = act @ pw + pb                                         # the 64 lanes' logits: a padding lane's term is exactly 0
    assert (np.exp(logit - logit.max())[B:] == 0.0).all() and (np.exp(logit - logit.max())[:B] > 0.0).all()


def test_the_models_option_its_refusals_and_the_checkpoint(tmp_path):
    assert [tuple(p.shape) for p in MuZeroNet().state_dict().values()][-1] == (1, )          # the default: today's module
    net = MuZeroNet(6, 3, 64, value_transform=True, support=20)
    nxt, reward, logits, value = net.recurrent_inference(net.representation(torch.randn(5, 6)), torch.tensor([0, 1, 2, 0, 1]))
    assert net.rew2.weight.shape == net.val.weight.shape == (41, 64) and reward.shape == value.shape == (5, )
    assert np.abs(value.detach().numpy() - sup.support_expectation(net.prediction_logits(nxt)[1].detach().numpy(), 20)).max() <= 4 * 2.0 ** -23 * 20
    with pytest.raises(ValueError, match='value_transform'):
        MuZeroNet(support=20)
    for bad in (0, 32, -1, 2.5):
        with pytest.raises(ValueError, match='support'):
            MuZeroNet(value_transform=True, support=bad)
    with pytest.raises(ValueError, match='fused_learner'):
        MuZeroAgent(device='cpu', fused_learner=True, value_transform=True, support=5)
    MuZeroAgent(device='cpu', value_transform=True, support=5).save_model(str(tmp_path / 'ck.pt'))
    MuZeroAgent(device='cpu', value_transform=True, support=5).load_model(str(tmp_path / 'ck.pt'))
    for other in (dict(support=6), dict()):
        with pytest.raises(ValueError, match='support'):
            MuZeroAgent(device='cpu', value_transform=True, **other).load_model(str(tmp_path / 'ck.pt'))


@pytest.mark.parametrize('S,scale', [(1, 3.0), (20, 8.0)])
def test_learn_is_the_cross_entropy_under_float64_autograd(S, scale):
    """``learn`` (float32; plain SGD of rate 1 in Adam's place, so the step is the clipped gradient) against the same agent in float64.
    The bound is the number format's: every entry goes through 64-term dot products in K + 1 unrolled steps, so YARDSTICK * 64 * (K + 1)
    roundings of 2^-23 of the largest entry.  The definition itself, once, from the twin: a K = 0 batch's value loss."""
    batch, weights = make_batch(9, 3, 3, 6, seed=S, target_scale=scale)   # K = 3
    agents = [MuZeroAgent(6, 3, device='cpu', value_transform=True, support=S) for _ in range(2)]
    agents[1].net.double().load_state_dict({k: v.double() for k, v in agents[0].net.state_dict().items()})
    head = agents[1].net.prediction_logits(agents[1].net.representation(torch.from_numpy(batch[0]).double()))[1].detach()
    lv0 = -(sup.two_hot_dense(batch[2][:, 0], S) * torch.log_softmax(head, dim=1).numpy()).sum(axis=1)
    assert np.array_equal(sup.two_hot_torch(torch.from_numpy(batch[2]).double(), S).numpy(), sup.two_hot_dense(batch[2], S))
    probe = MuZeroAgent(6, 3, device='cpu', value_transform=True, support=S)   # K = 0: the value loss is step 0's alone
    probe.net.double().load_state_dict(agents[1].net.state_dict())
    got0 = probe.learn(tuple(a[:, :1].astype(np.float64) if i > 1 else a[:, :0] if i == 1 else a.astype(np.float64) for i, a in enumerate(batch)))
    assert abs(got0[1] - lv0.mean()) <= 1e-12 * lv0.mean() and got0[2] == 0.0
    out, steps = [], []
    for agent, dtype in zip(agents, (np.float32, np.float64)):
        agent.optimizer = torch.optim.SGD(agent.net.parameters(), lr=1.0)
        before = torch.cat([p.detach().reshape(-1) for p in agent.net.parameters()]).double().numpy()
        out.append(np.array(agent.learn(tuple(a if a.dtype == np.int64 else a.astype(dtype) for a in batch), weights.astype(dtype))))
        steps.append(before - torch.cat([p.detach().reshape(-1) for p in agent.net.parameters()]).double().numpy())
    bound = YARDSTICK * 64 * (3 + 1) * 2.0 ** -23
    assert np.abs(out[0] - out[1]).max() <= bound * np.abs(out[1]).max()
    assert np.abs(steps[0] - steps[1]).max() <= bound * np.abs(steps[1]).max() and np.abs(steps[1]).max() > 1e-3
