"""What rz_mz_load_model and rz_mz_load_representation compute before they upload (rlzero_amd/csrc/rz_mz_pack.h), on the CPU.

A driver with its own main is compiled against the header with ROCm's clang++ and the flags that matter to host arithmetic in the
library's build (-ffp-contract=off).  It reads a blob of the 14 (or 4) tensors in torch layout [out][in] and writes the packed vector
with its offsets; each buffer is then restated in numpy FROM ITS COMMENT in the header -- as a transpose or reshape of the torch tensor
-- and compared bit for bit, the padding floats and the zero rows of rep1 included.  The scalar pieces (pow2_for, wmax_of, the bound on
relu(dyn1), s1) run on edge inputs of their own through the same driver.

What the edge inputs show (the header's comments say the same; nothing here changes what is uploaded):
  * a largest weight below 2^-114 -- every float32 subnormal among them -- has no float32 power of two that brings it to 2^13:
    pow2_for returns inf (ldexp overflows), and f16_ok stays true because the weights are finite;
  * where 60000 / bound is exactly a power of two (bound 3750: s1 16), bound * s1 equals 60000: the bound holds with <=, not <;
  * a nan never reaches the bound or a scale (fmax drops it) and a -inf weight does not either: only the scan of the 14 tensors makes
    f16_ok false for them.  Finite float32 weights cannot make the bound infinite (64 x 3.4e38 is finite in fp64): +inf does."""
import math

import numpy as np
import pytest

import host_driver
from test_net_pack import run_both, same_bits

f32, f64 = np.float32, np.float64
H = 64
NAMES = ('dyn1.w', 'dyn1.b', 'dyn2.w', 'dyn2.b', 'rew1.w', 'rew1.b', 'rew2.w', 'rew2.b', 'pre1.w', 'pre1.b', 'pol.w', 'pol.b', 'val.w', 'val.b')

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <string>
#include "rz_mz_pack.h"

template <typename T> static std::vector<T> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)n / sizeof(T));
    if (n && fread(v.data(), 1, (size_t)n, f) != (size_t)n) exit(2);
    fclose(f);
    return v;
}
template <typename T> static void dump(const std::string &path, const T *p, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, sizeof(T), n, f) != n) { perror(path.c_str()); exit(2); }
    fclose(f);
}

int main(int argc, char **argv) {
    using namespace rzmp;
    static_assert(kMzH == 64 && kMzMaxA == 8 && kMzObs == 8, "the sizes the test is written for");
    const std::string cmd = argv[1];
    if (cmd == "model") {   // model A blob outdir -> host.bin, meta.bin (doubles: f16_ok, off_scales, off[14], bound)
        const int A = atoi(argv[2]);
        const std::vector<float> blob = slurp<float>(argv[3]);
        const std::string dir = argv[4];
        const size_t KX = (size_t)kMzH + A, sizes[14] = {KX * 64, 64, 64 * 64, 64, 64 * 64, 64, 64, 1, 64 * 64, 64, (size_t)A * 64, (size_t)A, 64, 1};
        const float *p[14];
        size_t at = 0;
        for (int i = 0; i < 14; ++i) { p[i] = blob.data() + at; at += sizes[i]; }
        if (at != blob.size()) return 3;
        const Model m = pack_model(p, A);
        dump(dir + "/host.bin", m.host.data(), m.host.size());
        double meta[17] = {m.f16_ok ? 1.0 : 0.0, (double)m.off_scales};
        for (int i = 0; i < 14; ++i) meta[2 + i] = (double)m.off[i];
        meta[16] = relu_dyn1_bound(p[0], p[1], A);
        dump(dir + "/meta.bin", meta, 17);
    } else if (cmd == "rep") {   // rep obs_dim blob outdir -> host.bin, meta.bin (doubles: off[4])
        const int D = atoi(argv[2]);
        const std::vector<float> blob = slurp<float>(argv[3]);
        const std::string dir = argv[4];
        if (blob.size() != (size_t)64 * D + 64 + 64 * 64 + 64) return 3;
        const float *p[4] = {blob.data(), blob.data() + 64 * D, blob.data() + 64 * D + 64, blob.data() + 64 * D + 64 + 64 * 64};
        const Representation r = pack_representation(p, D);
        dump(dir + "/host.bin", r.host.data(), r.host.size());
        const double meta[4] = {(double)r.off[0], (double)r.off[1], (double)r.off[2], (double)r.off[3]};
        dump(dir + "/meta.bin", meta, 4);
    } else if (cmd == "pow2") {   // floats -> pow2_for of each
        const std::vector<float> x = slurp<float>(argv[2]);
        std::vector<float> y(x.size());
        for (size_t i = 0; i < x.size(); ++i) y[i] = pow2_for(x[i]);
        dump(argv[3], y.data(), y.size());
    } else if (cmd == "s1") {   // doubles -> s1_for of each
        const std::vector<double> x = slurp<double>(argv[2]);
        std::vector<float> y(x.size());
        for (size_t i = 0; i < x.size(); ++i) y[i] = s1_for(x[i]);
        dump(argv[3], y.data(), y.size());
    } else {
        return 4;
    }
    return 0;
}
'''


driver = host_driver.fixture('mz_pack', DRIVER)


@pytest.fixture(scope='module')
def drv(driver):
    def run(cmd, *args, data, out_dtype=None):
        """Runs `cmd args <file of data> <out>` -> the output file as `out_dtype`, or (host float32, meta float64) of an output directory."""
        got = run_both(driver, [cmd, *args, *driver.write([data])], out_dtype, {'host': f32, 'meta': f64})
        return got if out_dtype is not None else (got['host'], got['meta'])
    return run


def model_weights(A, seed):
    """The 14 tensors in torch layout [out][in], random, of a size a trained net's have."""
    rs = np.random.RandomState(seed)
    shapes = [(H, H + A), (H, ), (H, H), (H, ), (H, H), (H, ), (1, H), (1, ), (H, H), (H, ), (A, H), (A, ), (1, H), (1, )]
    return [(rs.uniform(-1, 1, s) * 2.0 ** rs.randint(-6, 1)).astype(f32) for s in shapes]


def packed_model(drv, w):
    A = w[10].shape[0]
    host, meta = drv('model', A, data=np.concatenate([t.reshape(-1) for t in w]))
    return host, {'f16_ok': meta[0] == 1.0, 'off_scales': int(meta[1]), 'off': [int(v) for v in meta[2:16]], 'bound': meta[16],
                  'scales': host[int(meta[1]):int(meta[1]) + 8]}


# ---- independent restatements, from the comments of the header

def pad4(a):
    a = np.asarray(a, dtype=f32).reshape(-1)
    return np.concatenate([a, np.zeros(-a.size % 4, dtype=f32)])


def pow2_for(wmax):
    """The power of two that brings wmax into [2^13, 2^14), as a float32 (inf where float32 has none); 1 for 0, inf, nan."""
    wmax = float(wmax)
    if not (wmax > 0.0 and math.isfinite(wmax)):
        return f32(1.0)
    with np.errstate(over='ignore'):
        return np.ldexp(f32(1.0), 14 - math.frexp(wmax)[1]).astype(f32)


def wmax_of(w):
    """The largest |w| over the first 64 input columns; a nan does not count (fmax)."""
    return np.fmax.reduce(np.abs(w[:, :H]).reshape(-1), initial=f32(0.0))


def relu_dyn1_bound(w, b):
    """|bias| + the positive state weights (added in column order) + the largest action weight (at least 0), per unit in float64; the
    maximum over the units.  fmax everywhere: a nan term counts as absent."""
    w, b = w.astype(f64), b.astype(f64)
    with np.errstate(invalid='ignore'):
        acc = np.cumsum(np.concatenate([np.abs(b)[:, None], np.fmax(0.0, w[:, :H])], axis=1), axis=1)[:, -1]   # (cumsum adds in order)
        amax = np.fmax.reduce(w[:, H:], axis=1, initial=0.0)
        return np.fmax.reduce(acc + amax, initial=0.0)


def s1_for(bound):
    """16 while bound * 16 < 60000, else 2^(e - 1) with 60000 / bound = f 2^e, f in [0.5, 1); a bound that is not finite and positive
    counts as 1e30 there."""
    if bound * 16.0 < 60000.0:
        return 16.0
    return 2.0 ** (math.frexp(60000.0 / (bound if math.isfinite(bound) and bound > 0.0 else 1e30))[1] - 1)


def model_layout(w):
    """Every tensor padded to 4 floats, in order; dyn1.w, dyn2.w, rew1.w, pre1.w k-major (the transpose of torch's [out][in]), the rest
    as they are; then the 8 floats of the scales."""
    with np.errstate(invalid='ignore'):
        scales = [pow2_for(wmax_of(w[i])) for i in (0, 2, 4, 8)] + [f32(s1_for(float(relu_dyn1_bound(w[0], w[1])))), 0, 0, 0]
    return np.concatenate([pad4(t.T if i in (0, 2, 4, 8) else t) for i, t in enumerate(w)] + [np.array(scales, dtype=f32)])


# ---- the layouts, every element

@pytest.mark.parametrize('A', [1, 2, 3, 8])
def test_model_layout(drv, A):
    """The whole upload of rz_mz_load_model bit for bit: the four k-major matrices, the ten copies, the padding, the scales; the
    offsets are the running sum of the sizes rounded up to 4."""
    w = model_weights(A, 20 + A)
    host, m = packed_model(drv, w)
    sizes = [t.size for t in w]
    want_off = np.concatenate([[0], np.cumsum([(s + 3) // 4 * 4 for s in sizes])])
    assert m['off'] == want_off[:14].tolist() and m['off_scales'] == want_off[14] and host.size == want_off[14] + 8
    same_bits(host, model_layout(w))
    k_major = host[m['off'][0]:m['off'][0] + sizes[0]].reshape(H + A, H)         # dyn1: [k][unit], the action rows last
    same_bits(k_major[:H], w[0][:, :H].T)
    same_bits(k_major[H:], w[0][:, H:].T)
    same_bits(host[m['off'][10]:m['off'][10] + sizes[10]].reshape(A, H), w[10])  # pol.w stays [A][H]
    for i, s in enumerate(sizes):                                                # the padding floats are zero bits
        assert not host[m['off'][i] + s:m['off'][i] + (s + 3) // 4 * 4].view(np.uint32).any(), NAMES[i]
    assert not host[-3:].view(np.uint32).any()
    assert m['f16_ok'] and m['bound'] == relu_dyn1_bound(w[0], w[1])
    scaled = np.array([np.abs(w[i][:, :H]).max() for i in (0, 2, 4, 8)]) * m['scales'][:4]
    assert ((scaled >= 2.0 ** 13) & (scaled < 2.0 ** 14)).all() and m['scales'][4] == 16.0


@pytest.mark.parametrize('obs_dim', [1, 4, 6, 8])
def test_representation_layout(drv, obs_dim):
    """rep1.w k-major as [8][64] with zero rows at obs_dim and above, rep1.b, rep2.w k-major, rep2.b, no padding between them."""
    rs = np.random.RandomState(40 + obs_dim)
    w = [rs.uniform(-1, 1, s).astype(f32) for s in ((H, obs_dim), (H, ), (H, H), (H, ))]
    host, off = drv('rep', obs_dim, data=np.concatenate([t.reshape(-1) for t in w]))
    assert off.tolist() == [0, 8 * H, 8 * H + H, 8 * H + H + H * H] and host.size == 8 * H + H + H * H + H
    rep1 = np.zeros((8, H), dtype=f32)
    rep1[:obs_dim] = w[0].T
    same_bits(host, np.concatenate([rep1.reshape(-1), w[1], w[2].T.reshape(-1), w[3]]))
    assert not host[obs_dim * H:8 * H].view(np.uint32).any()


# ---- the scales

def test_weight_scales(drv):
    """A layer of zeros: 1.  A largest weight that is a power of two, and one ulp below it: the scaled maximum lies in [2^13, 2^14).
    A subnormal largest weight: inf (see the module's docstring).  dyn1's scale sees only its 64 state columns."""
    one_below = np.nextafter(f32(0.25), f32(0.0))

    def with_top(w, idx, top):
        w[idx] = (w[idx] * f32(0.1)).astype(f32)
        w[idx][17, 5] = -top

    w = model_weights(3, 7)
    w[2][:] = 0.0                          # dyn2: all zeros
    with_top(w, 4, f32(0.25))              # rew1: exactly a power of two
    with_top(w, 8, one_below)              # pre1: one ulp below it
    plain = packed_model(drv, w)[1]['scales'].copy()
    assert plain[1] == 1.0 and plain[2] == 2.0 ** 15 and plain[3] == 2.0 ** 16
    for top, scale in ((f32(0.25), plain[2]), (one_below, plain[3])):
        assert 2.0 ** 13 <= float(top) * float(scale) < 2.0 ** 14
    w[0][9, H + 1] = 1e30                  # a huge ACTION weight of dyn1: not one of the 64 columns the f16 pipe multiplies
    host, m = packed_model(drv, w)
    same_bits(m['scales'][:4], plain[:4])
    same_bits(host, model_layout(w))
    w[0][9, 3] = 1e30                      # ... the same weight on a state column is seen
    assert packed_model(drv, w)[1]['scales'][0] == pow2_for(1e30) == 2.0 ** (14 - 100)
    w = model_weights(2, 8)
    w[8][:] = 0.0
    w[8][3, 3] = 1e-40                     # pre1: a subnormal largest weight
    host, m = packed_model(drv, w)
    assert np.isinf(m['scales'][3]) and m['f16_ok']
    same_bits(host, model_layout(w))


def test_pow2_for(drv):
    """pow2_for itself against the restatement: powers of two and their neighbours, the ends of the float32 range, 0, inf, nan, a negative."""
    up, down = (lambda x: np.nextafter(f32(x), f32(np.inf))), (lambda x: np.nextafter(f32(x), f32(0.0)))
    xs = [1.0, up(1.0), down(1.0), 0.5, 0.25, down(0.25), 8192.0, 16384.0, down(16384.0), 3.0e38, 2.0 ** -113, 2.0 ** -114, up(2.0 ** -114), 2.0 ** -126,
          1e-40, 2.0 ** -149, 0.0, np.inf, np.nan, -1.0]
    got = drv('pow2', data=np.array(xs, dtype=f32), out_dtype=f32)
    same_bits(got, np.array([pow2_for(f32(x)) for x in xs], dtype=f32))
    assert got[:9].tolist() == [2.0 ** 13, 2.0 ** 13, 2.0 ** 14, 2.0 ** 14, 2.0 ** 15, 2.0 ** 16, 1.0, 0.5, 1.0]
    assert got[9] == 2.0 ** -114 and got[10] == 2.0 ** 126 and got[11] == 2.0 ** 127 and got[12] == 2.0 ** 127 and np.isinf(got[13:16]).all() and (got[16:] == 1.0).all()
    ok = np.arange(len(xs)) < 13
    scaled = np.array(xs, dtype=f64)[ok] * got[ok].astype(f64)
    assert ((scaled >= 2.0 ** 13) & (scaled < 2.0 ** 14)).all()


# ---- the bound on relu(dyn1) and s1

def bound_case(A, unit, bias, state=(), action=()):
    """Weights of zeros but for one unit of dyn1: its bias, some state weights (column, value), some action weights (action, value)."""
    w = [np.zeros_like(t) for t in model_weights(A, 0)]
    w[1][unit] = bias
    for k, v in state:
        w[0][unit, k] = v
    for a, v in action:
        w[0][unit, H + a] = v
    return w


@pytest.mark.parametrize('side', ['below', 'at', 'above'])
@pytest.mark.parametrize('form', ['bias', 'sum'])
def test_s1_around_the_threshold(drv, side, form):
    """bound * 16 just below 60000: s1 = 16; just above: 8; each time a power of two <= 16 with bound * s1 < 60000.  At 60000 exactly
    (bound 3750) s1 is 16 and bound * s1 = 60000, the one case of equality."""
    top = {'below': np.nextafter(f32(3750.0), f32(0.0)), 'at': f32(3750.0), 'above': np.nextafter(f32(3750.0), f32(np.inf))}[side]
    if form == 'bias':
        w = bound_case(2, 5, -top)                       # |bias| alone
        want = float(top)
    else:                                                # |bias| + positive state weights + the largest action weight; the negatives do not count
        w = bound_case(3, 60, f32(-250.0), state=[(0, f32(1500.0)), (7, f32(-4000.0)), (63, f32(1000.0))], action=[(0, f32(-9.0)), (1, top - f32(2750.0)), (2, f32(3.0))])
        want = 250.0 + 1500.0 + 1000.0 + float(top - f32(2750.0))
        assert f32(want) == top
    host, m = packed_model(drv, w)
    assert m['bound'] == want == relu_dyn1_bound(w[0], w[1]) and m['f16_ok']
    s1 = float(m['scales'][4])
    assert s1 == s1_for(want) == {'below': 16.0, 'at': 16.0, 'above': 8.0}[side]
    assert math.frexp(s1)[0] == 0.5 and s1 <= 16.0
    assert want * s1 < 60000.0 if side != 'at' else want * s1 == 60000.0
    same_bits(host, model_layout(w))


def test_bound_and_s1_of_random_weights(drv):
    """The bound of random weights large enough to pass 60000 / 16, against the float64 restatement; s1_for on bounds of every size."""
    for seed, gain in ((1, 1.0), (2, 300.0), (3, 1e6), (4, 1e30)):
        w = model_weights(3, seed)
        w[0] = (w[0] * f32(gain)).astype(f32)
        host, m = packed_model(drv, w)
        want = float(relu_dyn1_bound(w[0], w[1]))
        assert m['bound'] == want and m['f16_ok']
        s1 = float(m['scales'][4])
        assert s1 == s1_for(want) and math.frexp(s1)[0] == 0.5 and s1 <= 16.0 and want * s1 < 60000.0
        same_bits(host, model_layout(w))
    bounds = [0.0, 1.0, float(np.nextafter(3750.0, 0.0)), 3750.0, float(np.nextafter(3750.0, np.inf)), 7500.0, 60000.0, 480000.0, 1e29, np.inf, np.nan, -1.0]
    got = drv('s1', data=np.array(bounds, dtype=f64), out_dtype=f32)
    assert got.tolist() == [s1_for(b) for b in bounds]
    assert 2.0 ** -81 <= 60000.0 / 1e29 < 2.0 ** -80 and 2.0 ** -84 <= 60000.0 / 1e30 < 2.0 ** -83   # (inf and nan count as 1e30)
    assert got.tolist() == [16.0, 16.0, 16.0, 16.0, 8.0, 8.0, 1.0, 0.125, 2.0 ** -81, 2.0 ** -84, 2.0 ** -84, 16.0]


# ---- f16_ok

@pytest.mark.parametrize('tensor', range(14), ids=NAMES)
def test_one_nan_anywhere_forbids_whole_moves(drv, tensor):
    """One nan in any of the 14 tensors: f16_ok is false -- by the scan alone: the nan reaches neither the bound nor a scale."""
    w = model_weights(3, 30)
    flat = w[tensor].reshape(-1)
    flat[flat.size // 2] = np.nan
    host, m = packed_model(drv, w)
    assert not m['f16_ok']
    assert math.isfinite(m['bound']) and np.isfinite(m['scales']).all()
    same_bits(host, model_layout(w))


def test_an_inf_or_an_infinite_bound_forbids_whole_moves(drv):
    """-inf on a state column: the bound stays finite (a negative weight does not count), the scan says no.  +inf there, or an
    infinite bias: the bound itself is infinite.  Finite weights, however large: f16_ok is true."""
    for where, value, bound_finite in (((0, (4, 4)), -np.inf, True), ((0, (4, 4)), np.inf, False), ((1, (9, )), -np.inf, False), ((12, (0, 3)), np.inf, True)):
        w = model_weights(2, 31)
        w[where[0]][where[1]] = value
        host, m = packed_model(drv, w)
        assert not m['f16_ok'] and math.isfinite(m['bound']) == bound_finite
        assert m['bound'] == relu_dyn1_bound(w[0], w[1])
        same_bits(host, model_layout(w))
    w = model_weights(2, 31)
    w[0][:, :H] = np.finfo(f32).max                    # the largest bound finite float32 weights can give
    _, m = packed_model(drv, w)
    assert m['f16_ok'] and math.isfinite(m['bound']) and m['bound'] > 64 * 3.4e38
