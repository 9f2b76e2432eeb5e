"""What rz_net_load computes before it uploads (rlzero_amd/csrc/rz_pack.h), on the CPU.

A driver with its own main is compiled against the header with ROCm's clang++ (the host compiler that knows _Float16) and the
flags that matter to host arithmetic in the library's build (-ffp-contract=off).  It reads a blob of the 16 tensors of a
PolicyValueNet and writes every prepared buffer; each layout is then restated in numpy FROM ITS COMMENT in the header -- as a
reshape / transpose of the weight tensor that puts "lane h*32 + r of tile t, step s" where the comment says -- and compared bit
for bit, padding included.  The scalar pieces (weight scale, hi + lo split, e4m3, activation bounds and scales) are run on edge
inputs of their own through the same driver."""
import filecmp
import math
import os

import numpy as np
import pytest

import host_driver

f32, f64, f16, u8, u16, u32 = np.float32, np.float64, np.float16, np.uint8, np.uint16, np.uint32

# (rows, cols, policy outputs): the smallest; n_actions != cells; 9 x 9; not square; padding in A; none
BOARDS = [(3, 3, 9), (6, 7, 7), (9, 9, 81), (11, 16, 176), (15, 15, 225), (16, 16, 256)]
VF_GROUPS = {(3, 3, 9): 16, (6, 7, 7): 32, (9, 9, 81): 64, (11, 16, 176): 128, (15, 15, 225): 128, (16, 16, 256): 128}
NPAD = {(3, 3, 9): 32, (6, 7, 7): 32, (9, 9, 81): 96, (11, 16, 176): 192, (15, 15, 225): 256, (16, 16, 256): 256}
SEEDS = (11, 12)
BUFFERS = ('w1', 'w2', 'w3', 'u2f', 'u3f', 's2', 's3', 's1', 't2', 't3', 't3f', 'fs_act', 'fs_val', 's_inv', 'wh', 'whp', 'bh',
           'fc_act_w', 'fc_act_b', 'fc_val1_w', 'w1t')

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <string>
#include "rz_pack.h"

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
#define DUMP(name) dump(dir + "/" #name ".bin", P.name.data(), P.name.size())

int main(int argc, char **argv) {
    const std::string cmd = argv[1];
    if (cmd == "prep") {   // prep S A Npad groups_act groups_val blob outdir
        const rzp::Shape D{atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])};
        const std::vector<float> blob = slurp<float>(argv[7]);
        const std::string dir = argv[8];
        const size_t S = (size_t)D.S, A = (size_t)D.A;
        const size_t sizes[16] = {32 * 4 * 9, 32, 64 * 32 * 9, 64, 128 * 64 * 9, 128, 4 * 128, 4, A * 4 * S, A, 2 * 128, 2, 64 * 2 * S, 64, 64, 1};
        const float *p[16];
        size_t at = 0;
        for (int i = 0; i < 16; ++i) { p[i] = blob.data() + at; at += sizes[i]; }
        if (at != blob.size()) return 3;
        const rzp::Prepared P = rzp::prepare(p, D);
        DUMP(w1); DUMP(w2); DUMP(w3); DUMP(u2f); DUMP(u3f); DUMP(s2); DUMP(s3); DUMP(s1); DUMP(t2); DUMP(t3); DUMP(t3f);
        DUMP(fs_act); DUMP(fs_val); DUMP(s_inv); DUMP(wh); DUMP(whp); DUMP(bh); DUMP(fc_act_w); DUMP(fc_act_b); DUMP(fc_val1_w); DUMP(w1t);
        float meta[10] = {(float)P.vf_groups, P.split_ok ? 1.0f : 0.0f};
        for (int i = 0; i < 8; ++i) meta[2 + i] = P.range_info[i];
        dump(dir + "/meta.bin", meta, 10);
    } else if (cmd == "e4m3") {   // floats -> bytes
        const std::vector<float> x = slurp<float>(argv[2]);
        std::vector<unsigned char> y(x.size());
        for (size_t i = 0; i < x.size(); ++i) y[i] = rzp::to_e4m3(x[i]);
        dump(argv[3], y.data(), y.size());
    } else if (cmd == "scale") {   // scale n: rows of n floats -> a scale per row
        const size_t n = (size_t)atol(argv[2]);
        const std::vector<float> x = slurp<float>(argv[3]);
        std::vector<float> y(x.size() / n);
        for (size_t i = 0; i < y.size(); ++i) y[i] = rzp::weight_scale(x.data() + i * n, n);
        dump(argv[4], y.data(), y.size());
    } else if (cmd == "split") {   // floats -> (hi, lo) f16 pairs
        const std::vector<float> x = slurp<float>(argv[2]);
        std::vector<_Float16> y(2 * x.size());
        for (size_t i = 0; i < x.size(); ++i) rzp::split_f16(x[i], &y[2 * i], &y[2 * i + 1]);
        dump(argv[3], y.data(), y.size());
    } else if (cmd == "act") {   // doubles -> act_scale floats
        const std::vector<double> x = slurp<double>(argv[2]);
        std::vector<float> y(x.size());
        for (size_t i = 0; i < x.size(); ++i) y[i] = rzp::act_scale(x[i]);
        dump(argv[3], y.data(), y.size());
    } else if (cmd == "bound") {   // bound cout cin taps weights+bias [input bounds | -] -> top, out[cout] as doubles
        const int cout = atoi(argv[2]), cin = atoi(argv[3]), taps = atoi(argv[4]);
        const std::vector<float> wb = slurp<float>(argv[5]);
        std::vector<double> in;
        if (std::string(argv[6]) != "-") in = slurp<double>(argv[6]);
        std::vector<double> y(1 + (size_t)cout);
        y[0] = rzp::layer_bound(wb.data(), wb.data() + (size_t)cout * cin * taps, cout, cin, taps, in.empty() ? nullptr : in.data(), y.data() + 1);
        dump(argv[7], y.data(), y.size());
    } else {
        return 4;
    }
    return 0;
}
'''


def run_both(driver, argv, out_dtype, files):
    """`argv <out>` through both builds of `driver` -> the plain build's output file as `out_dtype`, or (None) {name: array} of the
    `files` = {name: dtype} in its output directory.  Every file is held equal between the builds, byte for byte."""
    outs = driver.fresh(1)
    if out_dtype is None:
        for (path, ) in outs:
            os.mkdir(path)
    (plain, ), (san, ) = driver.both(argv, outs)
    if out_dtype is not None:
        assert filecmp.cmp(plain, san, shallow=False)
        return np.fromfile(plain, dtype=out_dtype)
    assert filecmp.cmpfiles(plain, san, [name + '.bin' for name in files], shallow=False)[1:] == ([], [])   # (none differs, none is missing)
    return {name: np.fromfile(os.path.join(plain, name + '.bin'), dtype=dt) for name, dt in files.items()}


driver = host_driver.fixture('pack', DRIVER)


@pytest.fixture(scope='module')
def drv(driver):
    def run(cmd, *args, inputs=(), out_dtype=None):
        """Runs `cmd`; each of `inputs` (arrays; None: '-') becomes a file argument behind `args`, the output file comes last."""
        argv = [cmd, *args, *['-' if a is None else driver.write([a])[0] for a in inputs]]
        return run_both(driver, argv, out_dtype, {name: f32 for name in BUFFERS + ('meta', )})
    return run


def shape_of(board):
    """rz_net_create's geometry: S, A, Npad, groups_act, groups_val."""
    rows, cols, A = board
    S = rows * cols
    return S, A, (A + 31) // 32 * 32, (4 * S + 15) // 16, (2 * S + 15) // 16


def net_weights(board, seed):
    """The 16 tensors of PolicyValueNet(board).state_dict() as float32 arrays, in its order."""
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(seed)
    return [v.detach().numpy().astype(f32).copy() for v in PolicyValueNet(*board).state_dict().values()]


_cache = {}


def prepared(drv, board, seed, edit=None):
    """(weights, buffers) of a net; `edit(weights)` changes them first (not cached)."""
    key = (board, seed)
    if edit is None and key in _cache:
        return _cache[key]
    w = net_weights(board, seed)
    if edit is not None:
        edit(w)
    got = drv('prep', *shape_of(board), inputs=[np.concatenate([t.reshape(-1) for t in w])])
    if edit is None:
        _cache[key] = (w, got)
    return w, got


CASES = [(b, s) for b in BOARDS for s in SEEDS]
case_id = lambda c: '%dx%d-%d' % (c[0][0], c[0][1], c[1]) if isinstance(c, tuple) and isinstance(c[0], tuple) else None


# ---- independent restatements

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: u16, 4: u32, 8: np.uint64, 1: u8}[a.dtype.itemsize]).reshape(-1)


def same_bits(got, want):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, '%d of %d elements differ, the first at %d' % (bad.size, got.size, bad[0])


def weight_scale(w):
    """oracle.fp8_cross_ref.weight_scale, as the float the library holds (a denormal largest weight: 2^140 and more -> inf)."""
    import torch
    from oracle.fp8_cross_ref import weight_scale as ref
    with np.errstate(over='ignore'):
        return f32(ref(torch.from_numpy(np.ascontiguousarray(w))))


def pieces(v):
    """[hi | lo] of float32 values: hi = float16(v), lo = float16(v - float32(hi))."""
    v = np.asarray(v, dtype=f32)
    with np.errstate(invalid='ignore', over='ignore'):
        hi = v.astype(f16)
        lo = (v - hi.astype(f32)).astype(f16)
    return np.stack([hi, lo])


def conv_layout(w):
    """pack_conv: [tile][cin_step][tg][lane = kq*16 + m][e] = W[16 tile + m][4 step + kq][tap 4 tg + e], taps 9 .. 11 zero."""
    cout, cin = w.shape[:2]
    p = np.zeros((cout, cin, 12), dtype=f32)
    p[:, :, :9] = w.reshape(cout, cin, 9)
    p = p.reshape(cout // 16, 16, cin // 4, 4, 3, 4)      # tile, m, step, kq, tg, e
    return p.transpose(0, 2, 4, 3, 1, 5)                  # tile, step, tg, kq, m, e


def wino_layout(w):
    """pack_wino_f4: U = G g G^T in float64 (each product summed left to right), rounded once; [tile][pass][cin_step][j][lane = kq*16 + m][e]
    = component k = 4 j + e of pass p of U[16 tile + m][4 step + kq], component k = U[rows[p][k // 6]][k % 6], rows = (1, 2), (3, 4), (0, 5)."""
    G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]])
    cout, cin = w.shape[:2]
    g = w.astype(f64)                                      # [cout][cin][3][3]
    tmp = sum(G[None, None, :, k, None] * g[:, :, None, k, :] for k in range(3))       # [cout][cin][6][3] = G g
    U = sum(tmp[:, :, :, None, k] * G[None, None, None, :, k] for k in range(3))       # [cout][cin][6][6] = (G g) G^T
    comp = np.stack([U[:, :, rows, :].reshape(cout, cin, 12) for rows in ((1, 2), (3, 4), (0, 5))], axis=2).astype(f32)   # [cout][cin][pass][k]
    comp = comp.reshape(cout // 16, 16, cin // 4, 4, 3, 3, 4)   # tile, m, step, kq, pass, j, e
    return comp.transpose(0, 4, 2, 5, 3, 1, 6)                  # tile, pass, step, j, kq, m, e


def split_layout(w, scale):
    """pack_split: [tile of 32][step = tap * chunks + chunk of 16][piece][lane = h*32 + r][j] = piece of W[32 tile + r][16 chunk + 8 h + j][tap] * scale."""
    cout, cin = w.shape[:2]
    p = pieces(w.reshape(cout, cin, 9) * f32(scale))
    p = p.reshape(2, cout // 32, 32, cin // 16, 2, 8, 9)   # piece, tile, r, chunk, h, j, tap
    return p.transpose(1, 6, 3, 0, 4, 2, 5)                # tile, tap, chunk, piece, h, r, j


def split_unpack(buf, cout, cin):
    """The hi pieces of a pack_split buffer, back as [cout][cin][tap]."""
    p = buf.view(f16).reshape(cout // 32, 9, cin // 16, 2, 2, 32, 8)
    return p[:, :, :, 0].transpose(0, 4, 2, 3, 5, 1).reshape(cout, cin, 9)   # tile, r, chunk, h, j, tap


def rows_layout(w, scale):
    """pack_rows: [tile of 16][step = tap * chunks + chunk of 32][piece][lane = g*16 + r][j] = piece of W[16 tile + r][32 chunk + 8 g + j][tap] * scale."""
    cout, cin = w.shape[:2]
    p = pieces(w.reshape(cout, cin, 9) * f32(scale))
    p = p.reshape(2, cout // 16, 16, cin // 32, 4, 8, 9)   # piece, tile, r, chunk, g, j, tap
    return p.transpose(1, 6, 3, 0, 4, 2, 5)                # tile, tap, chunk, piece, g, r, j


def rows_unpack(buf, cout, cin):
    p = buf.view(f16).reshape(cout // 16, 9, cin // 32, 2, 4, 16, 8)
    return p[:, :, :, 0].transpose(0, 4, 2, 3, 5, 1).reshape(cout, cin, 9)   # tile, r, chunk, g, j, tap


def e4m3_values():
    """The value of every e4m3fn byte (1.4.3, bias 7; 0x7f / 0xff: nan)."""
    b = np.arange(256)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    v[(b & 0x7f) == 0x7f] = np.nan
    return np.where(b >> 7 == 1, -v, v)


def check_e4m3(x, got):
    """`got`: the bytes of float32 `x`.  A nan is 0x7f; everything else carries the sign of x and decodes to the oracle's e4m3(x)."""
    import torch
    from oracle.fp8_cross_ref import e4m3
    x = np.asarray(x, dtype=f32).reshape(-1)
    got = np.asarray(got, dtype=u8).reshape(-1)
    assert got.shape == x.shape
    nan = np.isnan(x)
    assert (got[nan] == 0x7f).all()
    x, got = x[~nan], got[~nan]
    want = e4m3(torch.from_numpy(x.astype(f64))).numpy()
    assert np.array_equal(e4m3_values()[got], want)
    assert np.array_equal(got >> 7 == 1, np.signbit(x))


def rows_f8_parts(w, scale):
    """pack_rows_f8 -> (part 0 as f16 [tile][tap][half c][lane = g*16 + r][j] = hi of W[16 tile + r][32 c + 8 g + j][tap] * scale,
    the float32 inputs of part 1's bytes [tile][tap][half][lane = g*16 + r][j]: channel 16 g + j, half 0 lo * 32, half 1 hi / 64)."""
    cout, cin = w.shape[:2]
    p = pieces(w.reshape(cout, cin, 9) * f32(scale))
    hi = p[0].reshape(cout // 16, 16, 2, 4, 8, 9).transpose(0, 5, 2, 3, 1, 4)       # tile, r, c, g, j, tap -> tile, tap, c, g, r, j
    q = p.astype(f32).reshape(2, cout // 16, 16, 4, 16, 9)                          # piece, tile, r, g, j, tap
    x = np.stack([q[1] * f32(32.0), q[0] * f32(1.0 / 64.0)])                        # half, tile, r, g, j, tap
    return hi, x.transpose(1, 5, 0, 3, 2, 4)                                        # tile, tap, half, g, r, j


def split1_layout(w, scale):
    """pack_split1: [ky][piece][lane = h*32 + r][j] = piece of conv1's W[r][plane][ky][kx] * scale at k = 8 h + j = 4 kx + plane, kx = 3: zero."""
    p = np.zeros((32, 4, 3, 4), dtype=f32)                 # r, plane, ky, kx
    p[..., :3] = w * f32(scale)
    k = p.transpose(2, 0, 3, 1).reshape(3, 32, 2, 8)       # ky, r, (kx, plane) = (h, j)
    return pieces(k).transpose(1, 0, 3, 2, 4)              # ky, piece, h, r, j


def fc_layout(w, scale, tiles, steps):
    """pack_split_fc: [tile of 32 outputs][K-step][piece][lane = h*32 + c][j] = piece of W[32 tile + c][16 step + 8 h + j] * scale, zero beyond
    the outputs and inputs there are, and one more K-step of zeros behind the last tile."""
    n_out, k_in = w.shape
    p = np.zeros((32 * tiles, 16 * steps), dtype=f32)
    p[:n_out, :k_in] = w * f32(scale)
    p = pieces(p).reshape(2, tiles, 32, steps, 2, 8)       # piece, tile, c, step, h, j
    p = p.transpose(1, 3, 0, 4, 2, 5).reshape(-1)          # tile, step, piece, h, c, j
    return np.concatenate([p, np.zeros(2 * 64 * 8, dtype=f16)])


def layer_bound(w, bias, inp):
    """A ReLU output is at most its bias (if positive) plus the positive weights times the bounds of their inputs (None: 1), summed in
    float64 in the order (input channel, tap); a nan weight makes the bound infinite.  -> (the layer's largest bound, every channel's)."""
    cout, cin = w.shape[:2]
    w64 = w.astype(f64).reshape(cout, cin, -1)
    with np.errstate(invalid='ignore', over='ignore'):
        terms = np.where(w64 > 0, w64 * (1.0 if inp is None else inp[None, :, None]), 0.0)
        terms[np.isnan(w64)] = np.inf
        first = np.where(bias > 0, bias, 0).astype(f64)
        out = np.cumsum(np.concatenate([first[:, None], terms.reshape(cout, -1)], axis=1), axis=1)[:, -1]   # (cumsum adds in order)
    return (out.max() if (out >= 0).all() else np.inf), out


def act_scale(bound):
    """The largest power of two <= 16 that keeps bound * scale below 60000 (16 for a bound of 0)."""
    if not bound * 16.0 >= 60000.0:
        return 16.0
    return 2.0 ** (math.frexp(60000.0 / bound)[1] - 1)


# ---- the layouts, every element

@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_trunk_layouts(drv, case):
    """The three convolutions in all their layouts: f32 fragments (taps 9 .. 11 zero), Winograd, split f16 for both trunks and conv1's
    (kx = 3 zero); and one weight's hi piece is the same wherever it is packed."""
    w, got = prepared(drv, *case)
    c1, c2, c3 = w[0], w[2], w[4]
    for name, t in (('w1', c1), ('w2', c2), ('w3', c3)):
        same_bits(got[name], conv_layout(t))
        assert not got[name].reshape(-1, 3, 64, 4)[:, 2, :, 1:].any()      # taps 9, 10, 11
    same_bits(got['u2f'], wino_layout(c2))
    same_bits(got['u3f'], wino_layout(c3))
    s1, s2, s3 = weight_scale(c1), weight_scale(c2), weight_scale(c3)
    same_bits(got['s2'].view(f16), split_layout(c2, s2))
    same_bits(got['s3'].view(f16), split_layout(c3, s3))
    same_bits(got['t2'].view(f16), rows_layout(c2, s2))
    same_bits(got['t3'].view(f16), rows_layout(c3, s3))
    same_bits(got['s1'].view(f16), split1_layout(c1, s1))
    k = got['s1'].view(f16).reshape(3, 2, 2, 32, 8)                        # ky, piece, h, r, j
    assert not bits(k[:, :, 1, :, 4:]).any()                               # kx = 3: k = 12 .. 15 = (h 1, j 4 .. 7)
    hi3 = pieces(c3.reshape(128, 64, 9) * s3)[0]
    same_bits(split_unpack(got['s3'], 128, 64), hi3)
    same_bits(rows_unpack(got['t3'], 128, 64), hi3)
    part0 = got['t3f'].view(f16).reshape(8, 9, 2, 2, 4, 16, 8)[:, :, 0]    # tile, tap, part 0, half c, g, r, j
    same_bits(part0.transpose(0, 4, 2, 3, 5, 1).reshape(128, 64, 9), hi3)  # tile, r, c, g, j, tap


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_fp8_layout(drv, case):
    """pack_rows_f8, all four 1024-byte parts of every (tile, tap): the hi fragments of the two chunks, e4m3(lo 2^5), e4m3(hi 2^-6)."""
    w, got = prepared(drv, *case)
    hi, x = rows_f8_parts(w[4], weight_scale(w[4]))
    raw = got['t3f'].view(u8).reshape(8, 9, 2, 2048)
    same_bits(raw[:, :, 0].copy().view(f16), hi)
    check_e4m3(x, raw[:, :, 1].reshape(8, 9, 2, 4, 16, 16))


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_head_layouts(drv, case):
    """The FC layers' f16 fragments (zero rows >= n_out, zero k >= k_in, the extra zero K-step), the padded f32 copies, the 1 x 1 head
    convolutions, the value head's first layer by groups of four inputs."""
    board, _ = case
    w, got = prepared(drv, *case)
    S, A, npad, ga, gv = shape_of(board)
    assert npad == NPAD[board]
    same_bits(got['fs_act'].view(f16), fc_layout(w[8], weight_scale(w[8]), npad // 32, ga))
    same_bits(got['fs_val'].view(f16), fc_layout(w[12], weight_scale(w[12]), 2, gv))
    act = got['fs_act'].view(f16)[:-1024].reshape(npad // 32, ga, 2, 2, 32, 8)           # tile, step, piece, h, c, j
    rows_beyond = act.transpose(0, 4, 1, 2, 3, 5).reshape(npad, -1)[A:]
    k_beyond = act.transpose(1, 3, 5, 0, 2, 4).reshape(16 * ga, -1)[4 * S:]
    assert not bits(rows_beyond).any() and not bits(k_beyond).any() and not bits(got['fs_act'].view(f16)[-1024:]).any()
    fa = np.zeros((npad, 16 * ga), dtype=f32)
    fa[:A, :4 * S] = w[8]
    fb = np.zeros(npad, dtype=f32)
    fb[:A] = w[9]
    fv = np.zeros((64, 16 * gv), dtype=f32)
    fv[:, :2 * S] = w[12]
    same_bits(got['fc_act_w'], fa)
    same_bits(got['fc_act_b'], fb)
    same_bits(got['fc_val1_w'], fv)
    wh = np.concatenate([w[6].reshape(4, 128), w[10].reshape(2, 128)])
    same_bits(got['wh'], wh)
    same_bits(got['whp'], wh.T)
    same_bits(got['bh'], np.concatenate([w[7], w[11]]))
    groups = int(got['meta'][0])
    assert groups == VF_GROUPS[board] and groups in (16, 32, 64, 128) and 4 * groups >= 2 * S and (groups == 16 or 2 * groups < 2 * S)
    t = np.zeros((64, 4 * groups), dtype=f32)
    t[:, :2 * S] = w[12]
    same_bits(got['w1t'], t.reshape(64, groups, 4).transpose(1, 0, 2))                   # [group][hidden unit][4]


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_bounds_and_scales(drv, case):
    """range_info and s_inv of a net: the bounds in float64, the activation scales, the eight factors in float32."""
    w, got = prepared(drv, *case)
    t1, b1 = layer_bound(w[0], w[1], None)
    t2, b2 = layer_bound(w[2], w[3], b1)
    _, b3 = layer_bound(w[4], w[5], b2)
    tf = max(layer_bound(w[6], w[7], b3)[0], layer_bound(w[10], w[11], b3)[0])
    a1, a2, a3 = (f32(act_scale(t)) for t in (t1, t2, tf))
    assert got['meta'][1] == 1.0
    same_bits(got['meta'][2:], np.array([t1, t2, tf, a1, a2, a3, 1.0, 0.0], dtype=f32))
    sw1, sw2, sw3, sfa, sfv = (weight_scale(w[i]) for i in (0, 2, 4, 8, 12))
    one, obs = f32(1.0), f32(16.0)
    same_bits(got['s_inv'], np.array([a2 / (a1 * sw2), one / (a2 * sw3), a1 / (obs * sw1), one / (a3 * sfa), one / (a3 * sfv), a1, a2, a3], dtype=f32))


# ---- the scalar pieces on edge inputs

def test_layer_bound(drv):
    """layer_bound itself, every channel's bound: without input bounds (conv1), with them (conv2), 1 x 1 (the heads), a nan weight."""
    w = net_weights((9, 9, 81), 5)
    _, b1 = layer_bound(w[0], w[1], None)
    _, b2 = layer_bound(w[2], w[3], b1)
    _, b3 = layer_bound(w[4], w[5], b2)
    bad = w[2].copy()
    bad[7, 3, 1, 1] = np.nan
    for wt, bias, inp in ((w[0], w[1], None), (w[2], w[3], b1), (w[4], w[5], b2), (w[6], w[7], b3), (w[10], w[11], b3), (bad, w[3], b1)):
        cout, cin = wt.shape[:2]
        got = drv('bound', cout, cin, wt[0, 0].size, inputs=[np.concatenate([wt.reshape(-1), bias]), inp], out_dtype=f64)
        top, out = layer_bound(wt, bias, inp)
        same_bits(got, np.concatenate([[top], out]))
    assert np.isinf(got[0]) and np.isinf(got[1 + 7]) and np.isfinite(np.delete(got, [0, 1 + 7])).all()


def test_act_scale(drv):
    """16 for a bound of 0 and while bound * 16 stays below 60000 (3750: 60000 / 3750 = 16 exactly), 8 just above; 2^-k where the
    bound is 60000 * 2^k; just above such a bound the next power down."""
    up = lambda x: np.nextafter(x, np.inf)
    bounds = [0.0, 1.0, np.nextafter(3750.0, 0.0), 3750.0, up(3750.0), 7500.0, up(7500.0), 60000.0, 480000.0, up(480000.0), 60000.0 * 2.0 ** 20, 1e29]
    want = [16.0, 16.0, 16.0, 16.0, 8.0, 8.0, 4.0, 1.0, 0.125, 0.0625, 2.0 ** -20, 2.0 ** -81]
    assert 2.0 ** -81 <= 60000.0 / 1e29 < 2.0 ** -80
    got = drv('act', inputs=[np.array(bounds, dtype=f64)], out_dtype=f32)
    assert got.tolist() == want
    assert [act_scale(b) for b in bounds] == want


def test_weight_scale(drv):
    """The oracle's weight_scale: the largest weight exactly a power of two, just below one, a denormal (no float32 power of two brings
    it to 2^13: inf, as the oracle's 2^(14 - e) is in float32), tensors of zeros, of inf, of nan (scale 1)."""
    rs = np.random.RandomState(0)
    rows = rs.uniform(-1, 1, (24, 64)).astype(f32) * (2.0 ** rs.randint(-30, 30, (24, 1))).astype(f32)
    edge = []
    for top in (1.0, 0.5, 2.0 ** -20, 8192.0, 16384.0, np.nextafter(f32(1.0), f32(0.0)), np.nextafter(f32(1.0), f32(2.0)), 1e-40, 2.0 ** -149, 2.0 ** -126):
        r = rs.uniform(-0.4, 0.4, 64).astype(f32) * f32(top)
        r[rs.randint(64)] = -top if len(edge) % 2 else top
        edge.append(r)
    rows = np.concatenate([rows, np.array(edge, dtype=f32), np.zeros((1, 64), f32), np.full((1, 64), np.inf, f32), np.full((1, 64), np.nan, f32)])
    rows[-2, 5] = -np.inf
    got = drv('scale', 64, inputs=[rows], out_dtype=f32)
    same_bits(got, np.array([weight_scale(r) for r in rows], dtype=f32))
    assert got[24] == 2.0 ** 13 and got[25] == 2.0 ** 14 and got[28] == 0.5 and got[29] == 2.0 ** 14 and got[30] == 2.0 ** 13
    assert np.isinf(got[31:34]).all() and (got[-3:] == 1.0).all()
    scaled = np.abs(rows[:31]).max(axis=1) * got[:31]
    assert ((scaled >= 2.0 ** 13) & (scaled < 2.0 ** 14)).all()


def test_split_f16(drv):
    """hi = float16(v), lo = float16(v - float32(hi)): scaled weights (|v| < 2^14), ties of the f16 rounding, f16 subnormals, zeros."""
    rs = np.random.RandomState(1)
    v = np.concatenate([
        rs.uniform(-16384, 16384, 4096), rs.uniform(-1, 1, 4096), rs.uniform(-1, 1, 1024) * 2.0 ** -16, [0.0, -0.0, 16383.996, 1.0 + 2.0 ** -11,
        1.0 + 3 * 2.0 ** -11, 2048.5, 2049.5, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 65504.0, 1e-30]]).astype(f32)
    got = drv('split', inputs=[v], out_dtype=u16).reshape(-1, 2)
    same_bits(got.T, pieces(v))


def test_e4m3(drv):
    """Every f16 bit pattern as a float, times 1, 32 and 1 / 64 (what pack_rows_f8 feeds it and more), against the oracle; then the
    cases by name."""
    h = np.arange(65536, dtype=u16).view(f16).astype(f32)
    with np.errstate(invalid='ignore'):
        x = np.concatenate([h, h * f32(32.0), h * f32(1.0 / 64.0)])
    check_e4m3(x, drv('e4m3', inputs=[x], out_dtype=u8))
    tiny = 2.0 ** -10
    named = [(np.nan, 0x7f), (-np.nan, 0x7f), (448.0, 0x7e), (-448.0, 0xfe), (1e9, 0x7e), (np.inf, 0x7e), (-np.inf, 0xfe), (464.0, 0x7e), (447.0, 0x7e),
             (432.0, 0x7e), (431.9, 0x7d), (0.0, 0x00), (-0.0, 0x80), (1.0, 0x38), (1.0625, 0x38), (1.1875, 0x3a), (-1.0625, 0xb8), (1.0626, 0x39),
             (tiny, 0x00), (-tiny, 0x80), (float(np.nextafter(f32(tiny), f32(1))), 0x01), (2 * tiny, 0x01), (3 * tiny, 0x02), (5 * tiny, 0x02),
             (14 * tiny, 0x07), (15 * tiny, 0x08), (16 * tiny, 0x08), (2.0 ** -6, 0x08), (1.9375, 0x40), (240.0, 0x77), (248.0, 0x78)]
    xs = np.array([v for v, _ in named], dtype=f32)
    got = drv('e4m3', inputs=[xs], out_dtype=u8)
    assert got.tolist() == [b for _, b in named]
    check_e4m3(xs, got)


@pytest.mark.parametrize('bad', [np.inf, np.nan], ids=['inf', 'nan'])
@pytest.mark.parametrize('layer', [0, 2, 4, 6, 10], ids=['conv1', 'conv2', 'conv3', 'act_conv1', 'val_conv1'])
def test_no_finite_bound(drv, layer, bad):
    """An inf or a nan weight in any convolution: no finite activation bound, split_ok false, the activation scales at their default.
    (conv3's own bound is not one of the three: the weight sits on a channel the policy head reads with a positive weight.)"""
    board = (3, 3, 9)
    base = net_weights(board, SEEDS[0])
    channel = int(np.argmax(base[6].reshape(4, 128)[0]))
    assert base[6].reshape(4, 128)[0, channel] > 0

    def edit(w):
        w[layer].reshape(w[layer].shape[0], -1)[channel if layer == 4 else 1, 2] = bad
    _, got = prepared(drv, board, SEEDS[0], edit)
    assert got['meta'][1] == 0.0 and got['meta'][8] == 0.0
    assert got['meta'][5:8].tolist() == [16.0, 16.0, 16.0] and got['s_inv'][5:].tolist() == [16.0, 16.0, 16.0]
    assert not np.isfinite(got['meta'][2:5]).all()
    _, ok = prepared(drv, board, SEEDS[0])
    assert ok['meta'][1] == 1.0 and np.isfinite(ok['meta'][2:5]).all()
