"""MuZero's invertible value transform (rlzero_amd/csrc/rz_mz_value.h) on the CPU, against its Python twin (tests/mz_value_twin.py).

A driver with its own main is compiled against the header with ROCm's clang++ (by tests/host_driver.py) with
-ffp-contract=off, plain and with -fsanitize=address,undefined (a stand-alone program: no Python process is involved), fed binary
inputs and compared BIT FOR BIT: ``value_h`` / ``value_h_inv`` with the twin, ``unroll_row<true>`` (rz_mz_target.h: the targets of
k_mzr_gather<true>) with ``ReplayBuffer(value_transform=True).sample``.  The torch functions of rlzero_amd/muzero/network.py and the
host buffer are held to the twin the same way.

The round trip: |h^-1(h(x)) - x| <= 1e-11 max(1, |x|).  The bound is the issue's; a CPU check of 200 000 draws with these expressions
gave a worst case of 2.4e-13, so it has about 40 x of room.  Where the 2e-13 comes from: s^2 = 1 + 4 eps (|y| + 1 + eps) is
(1 + 2 eps)^2 at y = 0, so u = (s - 1) / (2 eps) carries ulp(s) / (2 eps) = 1.1e-13 of absolute error and u^2 - 1 twice that -- h^-1
of a value near 0 is exact to 2e-13, not to an ulp.  The monotonicity check therefore uses a geometric grid (ratio 1.014 from 1e-6:
neighbours 1.4e-8 apart at the least), not neighbours that a random draw may put 1e-13 apart.

What the GPU test's bound catches (tests/test_mz_value_transform_gpu.py holds the kernel's inverted reward and value to YARDSTICK = 4
errors of the torch float32 route): the last test forms that tolerance on the CPU for the test nets at both head gains and shows how
many tolerances away three wrong inverses land."""
import os
import struct

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import host_driver
import mz_net_twin
import mz_value_twin as vt
from rlzero_amd.muzero.network import MuZeroNet, inverse_value_transform, value_transform
from rlzero_amd.muzero.selfplay import Episode, ReplayBuffer
from test_mz_learner_host import YARDSTICK, copy_net
from test_mz_search_net_host import host_case, rolled_net

EPS = 0.001
U = 2.0 ** -23
REACH = (0.9, 20.0)   # what rew2 / val are scaled to reach on either side of 0: |y| within about 1, and up to about 20 (h(500) = 21.9)

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rz_mz_target.h"
#include "rz_mz_value.h"

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

// values x.f64 [n] -> h.f64 [n], h_inv.f64 [n], h32.f32 [n] = (float)h((double)(float)x), h_inv32.f32 [n]
static int values(char **a) {
    const std::vector<double> x = load<double>(a[0]);
    std::vector<double> h(x.size()), hi(x.size());
    std::vector<float> h32(x.size()), hi32(x.size());
    for (size_t i = 0; i < x.size(); ++i) {
        h[i] = rzmzv::value_h(x[i]);
        hi[i] = rzmzv::value_h_inv(x[i]);
        const float f = (float)x[i];
        h32[i] = (float)rzmzv::value_h((double)f);
        hi32[i] = (float)rzmzv::value_h_inv((double)f);
    }
    store(a[1], h);
    store(a[2], hi);
    store(a[3], h32);
    store(a[4], hi32);
    return 0;
}

// rows VT K td T disc.f64 [td + 1] lengths.i32 [E] reward.f64 [E][T] value.f64 [E][T] action.i32 [E][T] draws.i64 [n][K + 2]
//   -> tv.f32 tr.f32 mask.f32 [n][K + 1], actions.i64 [n][K]
template <bool VT>
static int rows(char **a) {
    const int K = atoi(a[0]), td = atoi(a[1]), T = atoi(a[2]);
    const std::vector<double> disc = load<double>(a[3]);
    const std::vector<int32_t> lengths = load<int32_t>(a[4]);
    const std::vector<double> reward = load<double>(a[5]), value = load<double>(a[6]);
    const std::vector<int32_t> action = load<int32_t>(a[7]);
    const std::vector<int64_t> draws = load<int64_t>(a[8]);
    const size_t E = lengths.size(), n = draws.size() / (K + 2);
    if ((int)disc.size() != td + 1 || reward.size() != E * T || value.size() != E * T || action.size() != E * T) return 4;
    std::vector<float> tv(n * (K + 1)), tr(n * (K + 1)), mask(n * (K + 1));
    std::vector<int64_t> actions(n * K);
    for (size_t b = 0; b < n; ++b) {
        const int64_t *dr = draws.data() + b * (K + 2);
        const size_t e = (size_t)dr[0];
        if (e >= E || lengths[e] < 0 || lengths[e] > T || dr[1] < 0 || dr[1] >= lengths[e]) return 5;
        const int len = lengths[e];
        // (heap arrays of exactly the episode's length: a read past the end is the sanitizer's to report)
        const std::vector<double> rw(reward.begin() + e * T, reward.begin() + e * T + len), rv(value.begin() + e * T, value.begin() + e * T + len);
        const std::vector<int32_t> ac(action.begin() + e * T, action.begin() + e * T + len);
        for (int k = 0; k <= K; ++k) {
            const rzmzt::Row r = rzmzt::unroll_row<VT>(rw.data(), rv.data(), ac.data(), len, (int)dr[1], k, td, disc.data(), k > 0 ? dr[2 + k - 1] : 0);
            const size_t o = b * (K + 1) + k;
            tv[o] = r.value, tr[o] = r.reward, mask[o] = r.mask;
            if (k > 0) actions[b * K + k - 1] = r.action;
        }
    }
    store(a[9], tv);
    store(a[10], tr);
    store(a[11], mask);
    store(a[12], actions);
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "values" && argc == 7) return values(argv + 2);
    if (what == "rows1" && argc == 15) return rows<true>(argv + 2);
    if (what == "rows0" && argc == 15) return rows<false>(argv + 2);
    return 4;
}
'''


drv = host_driver.fixture('mz_value', DRIVER)


# ----------------------------------------------------------------------------------------------- the values
def sample_values():
    """4000 random values with |x| log-uniform over 1e-6 .. 1e6 (both signs) and the crafted ones."""
    rng = np.random.RandomState(43)
    x = 10.0 ** rng.uniform(-6.0, 6.0, size=4000) * np.where(rng.uniform(size=4000) < 0.5, -1.0, 1.0)
    denormal = struct.unpack('<d', struct.pack('<Q', 0x0000000000000123))[0]
    crafted = [0.0, -0.0, 1.0, -1.0, EPS, -EPS, 21.883, -21.883, 1e300, denormal, -denormal]
    return np.concatenate((x, np.array(crafted, dtype=np.float64)))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_the_twin_knows_the_papers_numbers():
    assert vt.EPS == EPS and abs(vt.value_h(500.0) - 21.883) < 1e-3 and vt.value_h(0.0) == 0.0
    assert abs(vt.value_h_inv(vt.value_h(500.0)) - 500.0) < 1e-9
    assert struct.pack('<d', vt.value_h(-0.0)) == struct.pack('<d', -0.0)


def test_the_header_equals_the_twin_bit_for_bit(drv):
    x = sample_values()
    h, hi, h32, hi32 = drv.run('values', [], [x], [np.float64, np.float64, np.float32, np.float32])
    assert (bits(h) == bits(vt.h_array(x))).all()
    assert (bits(hi) == bits(vt.h_inv_array(x))).all()
    with np.errstate(over='ignore'):
        x32 = x.astype(np.float32)   # (1e300 -> inf: h(inf) = inf on both sides)
    assert (bits(h32) == bits(vt.h_f32(x32))).all()
    assert (bits(hi32) == bits(vt.h_inv_f32(x32))).all()


def test_the_torch_functions_equal_the_twin_bit_for_bit():
    x = sample_values()
    t64 = torch.from_numpy(x)
    got_h, got_hi = value_transform(t64), inverse_value_transform(t64)
    assert got_h.dtype == torch.float64 and got_hi.dtype == torch.float64
    assert (bits(got_h.numpy()) == bits(vt.h_array(x))).all()
    assert (bits(got_hi.numpy()) == bits(vt.h_inv_array(x))).all()
    x32 = x[np.abs(x) < 1e30].astype(np.float32)
    t32 = torch.from_numpy(x32)
    got_h, got_hi = value_transform(t32), inverse_value_transform(t32)
    assert got_h.dtype == torch.float32 and got_hi.dtype == torch.float32 and got_h.shape == t32.shape
    assert (bits(got_h.numpy()) == bits(vt.h_f32(x32))).all()
    assert (bits(got_hi.numpy()) == bits(vt.h_inv_f32(x32))).all()


def test_round_trip_oddness_and_monotonicity(drv):
    x = sample_values()
    x = x[np.abs(x) < 1e299]   # (h(1e300) is fine, and so is its inverse; the bound below is relative, checked apart)
    h, hi = vt.h_array(x), vt.h_inv_array(x)
    back = vt.h_inv_array(h)
    rel = np.abs(back - x) / np.maximum(1.0, np.abs(x))
    print('round trip h^-1(h(x)): worst |error| / max(1, |x|) = %.3e' % rel.max())
    assert rel.max() <= 1e-11
    assert abs(vt.value_h_inv(vt.value_h(1e300)) - 1e300) <= 1e-11 * 1e300
    forth = vt.h_array(hi)   # (and the other way round, for |y| where h^-1(y) stays finite)
    assert (np.abs(forth - x) / np.maximum(1.0, np.abs(x))).max() <= 1e-11
    # odd, bit for bit: copysign carries the sign, everything else sees |x|
    assert (bits(vt.h_array(-x)) == bits(-h)).all() and (bits(vt.h_inv_array(-x)) == bits(-hi)).all()
    # strictly increasing on a sorted sample: a geometric grid (the module text says why), its mirror image and 0
    grid = 1e-6 * 1.014 ** np.arange(2000)
    assert grid[-1] > 1e5
    s = np.concatenate((-grid[::-1], [0.0], grid))
    assert (np.diff(s) > 0).all()
    for f in (vt.h_array, vt.h_inv_array):
        assert (np.diff(f(s)) > 0).all(), f.__name__
    got_h, got_hi, _, _ = drv.run('values', [], [s], [np.float64, np.float64, np.float32, np.float32])
    assert (np.diff(got_h) > 0).all() and (np.diff(got_hi) > 0).all()


# ----------------------------------------------------------------------------------------------- the host buffer and unroll_row<true>
D, A, K, TD, DISCOUNT, T = 6, 3, 5, 10, 0.997, 20


def episodes(seed):
    """Episodes of lengths 1 .. K + TD + 3 with negative rewards (Acrobot's sign) and root values of both signs."""
    rng = np.random.RandomState(seed)
    out = []
    for n in range(1, K + TD + 4):
        out.append(Episode.from_arrays(rng.standard_normal((n, D)).astype(np.float32), rng.randint(A, size=n).astype(np.int64),
                                       -rng.uniform(0.25, 1.75, size=n), rng.dirichlet(np.ones(A), size=n).astype(np.float32),
                                       rng.standard_normal(n) * 40.0 - 60.0))
    return out


def buffers(seed=5):
    eps = episodes(11)
    on = ReplayBuffer(capacity=100, unroll_steps=K, td_steps=TD, discount=DISCOUNT, seed=seed, value_transform=True)
    off = ReplayBuffer(capacity=100, unroll_steps=K, td_steps=TD, discount=DISCOUNT, seed=seed)
    for ep in eps:
        on.add(ep)
        off.add(ep)
    return eps, on, off


def fp64_targets(buf, eps, idx, pos):
    """The fp64 value and reward targets of the entries (idx, pos) as the buffer WITHOUT the flag forms them before its cast,
    and which of them lie inside the episode."""
    n = len(idx)
    tv, tr = np.zeros((n, K + 1)), np.zeros((n, K + 1))
    in_v, in_r = np.zeros((n, K + 1), dtype=bool), np.zeros((n, K + 1), dtype=bool)
    for b in range(n):
        ep = eps[idx[b]]
        for k in range(K + 1):
            i = pos[b] + k
            if i < len(ep):
                tv[b, k], in_v[b, k] = buf._value_target(ep, i), True
            if k > 0 and i - 1 < len(ep):
                tr[b, k], in_r[b, k] = ep.rewards[i - 1], True
    return tv, tr, in_v, in_r


def test_the_host_buffer_transforms_only_value_and_reward_targets():
    n = 400
    eps, on, off = buffers()
    assert on.value_transform and not off.value_transform and not ReplayBuffer().value_transform
    got = on.sample(n, A)
    plain = off.sample(n, A)
    rng = np.random.RandomState(5)   # the buffers' own draw sequence: the episodes, then the positions
    idx = rng.randint(len(eps), size=n)
    pos = [rng.randint(len(eps[i])) for i in idx]
    tv64, tr64, in_v, in_r = fp64_targets(off, eps, idx, pos)
    assert (bits(plain[2]) == bits(tv64.astype(np.float32))).all() and (bits(plain[3]) == bits(tr64.astype(np.float32))).all()
    assert (bits(got[2]) == bits(np.where(in_v, vt.h_array(tv64), 0.0).astype(np.float32))).all()
    assert (bits(got[3]) == bits(np.where(in_r, vt.h_array(tr64), 0.0).astype(np.float32))).all()
    assert in_v.any() and not in_v.all() and in_r[:, 1:].any() and not in_r[:, 1:].all()   # rows on both sides of an episode's end
    assert (got[2][in_v] != plain[2][in_v]).all() and (got[2][~in_v] == 0.0).all() and (got[3][~in_r] == 0.0).all()
    for i in (0, 1, 4, 5):   # observations, actions, policies and the mask are untouched
        assert got[i].dtype == plain[i].dtype and got[i].tobytes() == plain[i].tobytes()


def test_unroll_row_with_the_transform_equals_the_host_buffer(drv):
    """rz_mz_target.h: unroll_row<true>, what k_mzr_gather<true> writes, on EVERY (episode, position)."""
    eps, on, off = buffers()
    E = len(eps)
    lengths = np.array([len(ep) for ep in eps], dtype=np.int32)
    reward, value, action = np.zeros((E, T)), np.zeros((E, T)), np.zeros((E, T), dtype=np.int32)
    for e, ep in enumerate(eps):
        reward[e, :len(ep)], value[e, :len(ep)], action[e, :len(ep)] = ep.rewards, ep.root_values, ep.actions
    idx = np.repeat(np.arange(E), lengths)
    pos = np.concatenate([np.arange(m) for m in lengths])
    filler = np.random.RandomState(3).randint(A, size=(len(idx), K))
    draws = np.concatenate((idx[:, None], pos[:, None], filler), axis=1).astype(np.int64)
    disc = np.array([DISCOUNT ** i for i in range(TD + 1)], dtype=np.float64)
    tv64, tr64, in_v, in_r = fp64_targets(off, eps, idx, pos)
    outs = [np.float32, np.float32, np.float32, np.int64]
    tv1, tr1, mask1, act1 = drv.run('rows1', [K, TD, T], [disc, lengths, reward, value, action, draws], outs)
    tv0, tr0, mask0, act0 = drv.run('rows0', [K, TD, T], [disc, lengths, reward, value, action, draws], outs)
    assert (bits(tv0) == bits(tv64.astype(np.float32).reshape(-1))).all() and (bits(tr0) == bits(tr64.astype(np.float32).reshape(-1))).all()
    assert (bits(tv1) == bits(np.where(in_v, vt.h_array(tv64), 0.0).astype(np.float32).reshape(-1))).all()
    assert (bits(tr1) == bits(np.where(in_r, vt.h_array(tr64), 0.0).astype(np.float32).reshape(-1))).all()
    assert mask1.tobytes() == mask0.tobytes() and act1.tobytes() == act0.tobytes()
    assert (mask1.reshape(-1, K + 1) == in_v).all()


# ----------------------------------------------------------------------------------------------- the flag's owner, without a GPU
def test_the_flag_and_its_refusals_on_the_host(tmp_path):
    from rlzero_amd.muzero.agent import MuZeroAgent, check_value_transform
    assert not MuZeroNet().value_transform and MuZeroNet(value_transform=True).value_transform
    a_on = MuZeroAgent(device='cpu', value_transform=True)
    a_off = MuZeroAgent(device='cpu')
    assert a_on.net.value_transform and not a_off.net.value_transform
    b_on, b_off = ReplayBuffer(value_transform=True), ReplayBuffer()
    check_value_transform(a_on.net, b_on)
    check_value_transform(a_off.net, b_off)
    for agent, buf in ((a_on, b_off), (a_off, b_on)):
        with pytest.raises(ValueError) as info:
            agent.learn(None, buffer=buf)   # (refused before the batch is looked at)
        assert 'net has value_transform=%s' % agent.net.value_transform in str(info.value)
        assert 'ReplayBuffer' in str(info.value) and 'value_transform=%s' % buf.value_transform in str(info.value)
    p_on, p_off = str(tmp_path / 'on.model'), str(tmp_path / 'off.model')
    a_on.save_model(p_on)
    a_off.save_model(p_off)
    assert torch.load(p_on)['value_transform'] is True and 'value_transform' not in torch.load(p_off)
    a_on.load_model(p_on)
    a_off.load_model(p_off)
    for agent, path, saved in ((a_on, p_off, False), (a_off, p_on, True)):
        before = [p.clone() for p in agent.net.parameters()]
        with pytest.raises(ValueError) as info:
            agent.load_model(path)
        assert 'saved with value_transform=%s' % saved in str(info.value) and 'net has value_transform=%s' % (not saved) in str(info.value)
        assert all(torch.equal(a, b) for a, b in zip(before, agent.net.parameters()))


def test_the_trainers_flags_default_to_off():
    import importlib.util
    spec = importlib.util.spec_from_file_location('train_muzero_vt', os.path.join(REPO, 'tools', 'train_muzero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.build_parser().parse_args([])
    assert args.value_transform is False and args.eval_every == 0 and args.eval_envs is None
    args = mod.build_parser().parse_args(['--value-transform', '--eval-every', '10', '--eval-envs', '32'])
    assert args.value_transform is True and args.eval_every == 10 and args.eval_envs == 32


def test_the_abi_names_the_two_entries():
    from rlzero_amd import _hip
    assert {'rz_mz_set_value_transform', 'rz_mz_replay_set_value_transform'} <= set(_hip.exported_symbols())
    assert _hip.ABI_VERSION >= 43


# ----------------------------------------------------------------------------------------------- what the GPU bound catches
def inverse_without_eps(y):
    a = np.abs(y)
    return np.copysign((a + 1.0) ** 2 - 1.0, y)


def inverse_with_eps_dropped_in_the_root(y):
    a = np.abs(y)
    s = np.sqrt(1.0 + 4.0 * EPS * (a + 1.0))
    u = (s - 1.0) / (2.0 * EPS)
    return np.copysign(u * u - 1.0, y)


WRONG = (('an inverse without eps', inverse_without_eps), ('eps dropped inside the root', inverse_with_eps_dropped_in_the_root),
         ('h where h^-1 belongs', vt.h_array))
CAUGHT_BY = 10.0   # tolerances: every wrong inverse lands at least this many of them away, at both reaches (the figures: the test's docstring)


def scaled_heads(A, reach):
    """A copy of the float64 test net of ``A`` actions whose rew2 and val are an affine map of the original's: the test net's heads
    span a narrow band on one side of 0 (its value lies in -1.5 .. -1.0 at A = 3), so each head y becomes g (y - c), with c the middle
    and g = reach / half the width of the band the TWIN gives on the host chain of tests/test_mz_search_net_host.py -- outputs of both
    signs that reach about ``reach`` on either side.  (Other parent states, the kernel's own for instance, give a similar band.)"""
    net64, _, _, _, want = host_case(A, 0)
    net = copy_net(net64, torch.float64)
    with torch.no_grad():
        for layer, y in ((net.rew2, want.reward), (net.val, want.value)):
            c, half = 0.5 * (float(y.max()) + float(y.min())), 0.5 * (float(y.max()) - float(y.min()))
            g = reach / half
            layer.weight.mul_(g)
            layer.bias.copy_((layer.bias - c) * g)
    return net.eval()


@pytest.mark.parametrize('gain', REACH)
def test_the_gpu_bound_catches_a_wrong_inverse(gain):
    """The GPU test's tolerance, formed here with torch float32 on the CPU: YARDSTICK errors of ``recurrent_inference`` followed by
    ``inverse_value_transform`` against the twin's float64 outputs through the twin's h^-1, floored at 2^-23 max |h^-1|.

    The figures (reward / value; the tolerance grows with the head's gain, whose float32 error h^-1 multiplies by 2 (|y| + 1)):
      reach 0.9 (raw within 2.6), tolerance 9.1e-06 / 2.5e-05:  without eps off by 9.9e-03 = 1079 / 397 tolerances,
          eps dropped inside the root 3.8e-03 = 413 / 152,  h where h^-1 belongs 2.2 = 242 770 / 89 271
      reach 20 (raw within 422), tolerance 1.6e-03 / 3.2e-03:  without eps off by 17.6 = 11 122 / 5 488 tolerances,
          eps dropped inside the root 4.0e-02 = 25 / 12,  h where h^-1 belongs 419 = 265 219 / 130 876
    The weakest case -- eps missing only inside the root, seen through a value head of gain 90 -- is still 12 tolerances away."""
    _, _, states, actions, _ = host_case(3, 0)
    net = scaled_heads(3, gain)
    sd = mz_net_twin.state_dict64(net)
    want = mz_net_twin.recurrent(sd, states.astype(np.float64), actions)
    net32 = copy_net(net, torch.float32)
    with torch.no_grad():
        _, r32, _, v32 = net32.recurrent_inference(torch.from_numpy(states), torch.from_numpy(actions))
        r32, v32 = inverse_value_transform(r32).double().numpy(), inverse_value_transform(v32).double().numpy()
    for name, y, got32 in (('reward', want.reward, r32), ('value', want.value, v32)):
        raw = vt.h_inv_array(y)
        assert (y > 0).any() and (y < 0).any(), 'both signs'
        assert 0.99 * gain <= np.abs(y).max() <= 1.01 * gain
        yard = max(float(np.abs(got32 - raw).max()), U * float(np.abs(raw).max()))
        tol = YARDSTICK * yard
        print('reach %g %s: head outputs within %.2f (raw %.1f), tolerance %.3e' % (gain, name, np.abs(y).max(), np.abs(raw).max(), tol))
        for what, wrong in WRONG:
            off = float(np.abs(wrong(y) - raw).max())
            print('    %s: off by %.3e = %.0f tolerances' % (what, off, off / tol))
            assert off >= CAUGHT_BY * tol, (what, name, gain, off, tol)
