// rz_pack.h -- what rz_net_load computes on the host before anything is uploaded: the weights of PolicyValueNet in the fragment
// layouts of rz_net.hip's kernels, the power-of-two scales of the split-f16 route, the e4m3 bytes of the FP8 route, the activation
// bounds that decide whether the f16 pipe may be used at all.  Pure CPU arithmetic, no HIP: plain C++17 for a compiler that knows
// _Float16 (clang), included by rz_net.hip and by the driver of tests/test_net_pack.py, which restates every layout in numpy.
// Buffers the kernels read as 16-byte vectors are returned as std::vector<float> (four floats per vector): rz_net_load copies bytes.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

namespace rzp {

constexpr float kObsScale = 16.0f;  // observation planes (0 / 1) are stored times 16
constexpr float kMaxActScale = 16.0f, kF16Room = 60000.0f;  // activation scales: powers of two <= 16 that keep bound * scale < 60000

// weight [cout][cin][3][3] -> [tile][cin_step][3][lane][4]: lane = kq*16 + m holds
// W[16*tile + m][4*step + kq][tap = 4*tg + e] (taps 9..11 are zero padding)
inline std::vector<float> pack_conv(const float *w, int cout, int cin) {
    const int tiles = cout / 16, steps = cin / 4;
    std::vector<float> out((size_t)tiles * steps * 3 * 64 * 4, 0.0f);
    for (int t = 0; t < tiles; ++t)
        for (int s = 0; s < steps; ++s)
            for (int tg = 0; tg < 3; ++tg)
                for (int lane = 0; lane < 64; ++lane) {
                    const int m = lane & 15, kq = lane >> 4;
                    float *v = &out[((((size_t)t * steps + s) * 3 + tg) * 64 + lane) * 4];
                    for (int e = 0; e < 4; ++e) {
                        const int tap = 4 * tg + e;
                        if (tap < 9) v[e] = w[((size_t)(16 * t + m) * cin + (4 * s + kq)) * 9 + tap];
                    }
                }
    return out;
}

// U = G g G^T for F(4x4,3x3) (G: 6x3), packed [tile][pass][cin_step][3][64 lanes] x 4: lane = kq*16 + m
// holds components k = 4*j + e (j = 0..2) of pass p for U[16*tile + m][4*step + kq], component k =
// (transform row i' = rows[p][k / 6], column j' = k % 6).  fp64, rounded once.
inline std::vector<float> pack_wino_f4(const float *w, int cout, int cin) {
    static const double G[6][3] = {{1.0 / 4, 0, 0},          {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                   {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6},  {0, 0, 1}};
    static const int rows[3][2] = {{1, 2}, {3, 4}, {0, 5}};
    const int tiles = cout / 16, steps = cin / 4;
    std::vector<float> out((size_t)tiles * 3 * steps * 3 * 64 * 4);
    for (int t = 0; t < tiles; ++t)
        for (int s = 0; s < steps; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                const int m = lane & 15, kq = lane >> 4;
                const float *g = w + ((size_t)(16 * t + m) * cin + (4 * s + kq)) * 9;
                double tmp[6][3], U[6][6];
                for (int i = 0; i < 6; ++i)
                    for (int c = 0; c < 3; ++c)
                        tmp[i][c] = G[i][0] * g[0 * 3 + c] + G[i][1] * g[1 * 3 + c] + G[i][2] * g[2 * 3 + c];
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j) U[i][j] = tmp[i][0] * G[j][0] + tmp[i][1] * G[j][1] + tmp[i][2] * G[j][2];
                for (int p = 0; p < 3; ++p)
                    for (int j = 0; j < 3; ++j) {
                        float *v = &out[(((((size_t)t * 3 + p) * steps + s) * 3 + j) * 64 + lane) * 4];
                        for (int e = 0; e < 4; ++e) {
                            const int k = 4 * j + e;
                            v[e] = (float)U[rows[p][k / 6]][k % 6];
                        }
                    }
            }
    return out;
}

// The weight scale of the split-f16 route: the power of two that brings the largest |w| of the tensor into [2^13, 2^14)
// (1 for a tensor of zeros, or one that holds an inf or a nan)
inline float weight_scale(const float *w, size_t n) {
    float wmax = 0.0f;
    for (size_t i = 0; i < n; ++i) wmax = std::fmax(wmax, std::fabs(w[i]));
    int e = 0;
    if (wmax > 0.0f && std::isfinite(wmax)) {
        (void)std::frexp(wmax, &e);  // wmax = f * 2^e, f in [0.5, 1)
        e = 14 - e;                  // wmax * 2^e in [2^13, 2^14)
    }
    return std::ldexp(1.0f, e);
}

// v = hi + lo up to f16 rounding of lo: the two pieces every f32 operand of the f16 matrix pipe is carried as
inline void split_f16(float v, _Float16 *hi, _Float16 *lo) {
    *hi = (_Float16)v;
    *lo = (_Float16)(v - (float)*hi);
}

// w [cout][cin][3][3] * scale as hi + lo f16 pieces in the A fragments of an f16 MFMA whose tile has R = 32 or 16 rows (output
// channels) and whose K-step therefore holds 64 / R groups of 8 input channels: packed [tile of R cout][step = tap * chunks + chunk]
// [piece][lane] x 8 f16, lane = g*R + r holds W[R*tile + r][(512 / R)*chunk + 8*g + j][tap], j = 0..7.
inline std::vector<float> pack_frags(const float *w, int cout, int cin, float scale, int R) {
    const int tiles = cout / R, chunk = 512 / R, chunks = cin / chunk, steps = 9 * chunks;
    std::vector<float> out((size_t)tiles * steps * 2 * 64 * 4);
    _Float16 *o = reinterpret_cast<_Float16 *>(out.data());
    for (int t = 0; t < tiles; ++t)
        for (int tap = 0; tap < 9; ++tap)
            for (int c = 0; c < chunks; ++c)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int r = lane % R, g = lane / R, s = tap * chunks + c;
                        const size_t at = ((((size_t)t * steps + s) * 2 + 0) * 64 + lane) * 8 + j;   // (the lo piece: 64 lanes x 8 further)
                        split_f16(w[((size_t)(R * t + r) * cin + (chunk * c + 8 * g + j)) * 9 + tap] * scale, &o[at], &o[at + 512]);
                    }
    return out;
}

// Split f16 weights (k_trunk_split): w * scale = hi + lo with scale = weight_scale of the layer.
// Packed [tile of 32 cout][step = tap * chunks + chunk][piece][lane]
// x 8 f16: lane = h*32 + r holds W[32*tile + r][16*chunk + 8*h + j][tap], j = 0..7 (the A fragment of
// v_mfma_f32_32x32x16_f16).
inline std::vector<float> pack_split(const float *w, int cout, int cin, float *scale_out) {
    *scale_out = weight_scale(w, (size_t)cout * cin * 9);
    return pack_frags(w, cout, cin, *scale_out, 32);
}

// The same weights for k_trunk_rows (scale as pack_split: the two kernels share the rescaling factors).  Packed
// [tile of 16 cout][step = tap * chunks + chunk of 32 cin][piece][lane] x 8 f16: lane = g*16 + r holds
// W[16*tile + r][32*chunk + 8*g + j][tap], j = 0..7 (the A fragment of v_mfma_f32_16x16x32_f16).
inline std::vector<float> pack_rows(const float *w, int cout, int cin, float scale) { return pack_frags(w, cout, cin, scale, 16); }

// OCP e4m3fn (1.4.3, bias 7, no infinities, largest finite 448) of x, round to nearest even, saturating
inline unsigned char to_e4m3(float x) {
    const unsigned char sign = std::signbit(x) ? 0x80 : 0;
    double a = std::fabs((double)x);
    if (!(a == a)) return 0x7f;
    if (a >= 448.0) return sign | 0x7e;
    if (a < std::ldexp(1.0, -10)) return sign;   // below half the smallest subnormal (2^-9): zero
    int e = 0;
    (void)std::frexp(a, &e);   // a = f 2^e, f in [0.5, 1)
    int ex = e - 1;            // a = 1.m x 2^ex
    if (ex < -6) ex = -6;      // subnormals share the exponent of the smallest normal
    const double step = std::ldexp(1.0, ex - 3);
    double qv = std::nearbyint(a / step);   // (the default rounding mode: to nearest even)
    int m = (int)qv;   // 0 .. 16 in units of step
    if (ex == -6 && m < 8) return sign | (unsigned char)m;   // subnormal
    if (m == 16) { m = 8; ++ex; }
    if (ex > 8 || (ex == 8 && m - 8 > 6)) return sign | 0x7e;
    return sign | (unsigned char)(((ex + 7) << 3) | (m - 8));
}

// conv3 for the FP8 cross terms of k_trunk_rows (rt::slot_r, F8).  v = w * scale as in pack_rows (|v| < 2^14), hi = f16(v),
// lo = f16(v - hi).  Packed [tile of 16 cout][tap][part][half][lane] x 16 bytes with lane = g*16 + r:
//   part 0, half c: the hi f16 pieces of W[16 tile + r][32 c + 8 g + j][tap], j = 0..7 (pack_rows' hi fragment of chunk c);
//   part 1: the lane's 32 bytes of the K = 128 block of the scaled MFMA, input channels 16 g + j, j = 0..15:
//           half 0 = e4m3(lo * 2^5) (meets the activations' e5m2 value), half 1 = e4m3(hi * 2^-6) (meets e5m2((value - hi) 2^11));
//           with the block's scale 2^-5 both products come out in the units of hi x hi.  |lo| <= 4 and |hi| <= 2^14: 128 and 256 of 448.
inline std::vector<float> pack_rows_f8(const float *w, int cout, int cin, float scale) {
    const int tiles = cout / 16;
    std::vector<float> out((size_t)tiles * 9 * 2 * 2 * 64 * 4);
    unsigned char *o = reinterpret_cast<unsigned char *>(out.data());
    for (int t = 0; t < tiles; ++t)
        for (int tap = 0; tap < 9; ++tap)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 15, g = lane >> 4;
                auto piece = [&](int ci, _Float16 *hi, _Float16 *lo) {
                    split_f16(w[((size_t)(16 * t + r) * cin + ci) * 9 + tap] * scale, hi, lo);
                };
                const size_t base = ((size_t)t * 9 + tap) * 4 * 1024 + (size_t)lane * 16;
                for (int c = 0; c < 2; ++c)
                    for (int j = 0; j < 8; ++j) {
                        _Float16 hi, lo;
                        piece(32 * c + 8 * g + j, &hi, &lo);
                        memcpy(o + base + c * 1024 + j * 2, &hi, 2);
                    }
                for (int j = 0; j < 16; ++j) {
                    _Float16 hi, lo;
                    piece(16 * g + j, &hi, &lo);
                    o[base + 2048 + j] = to_e4m3((float)lo * 32.0f);
                    o[base + 3072 + j] = to_e4m3((float)hi * (1.0f / 64.0f));
                }
            }
    return out;
}

// conv1 (32 x 4 x 3 x 3) for k_trunk_split: K-step = kernel row ky, k = 4 * kx + plane for kx = 0..3 (kx = 3: zero
// padding); lane = h*32 + r holds k = 8*h .. 8*h + 7 of output channel r.  [ky][hi | lo][lane] x 8 f16.
inline std::vector<float> pack_split1(const float *w, float *scale_out) {
    const float scale = *scale_out = weight_scale(w, 32 * 4 * 9);
    std::vector<float> out((size_t)3 * 2 * 64 * 4);
    _Float16 *o = reinterpret_cast<_Float16 *>(out.data());
    for (int ky = 0; ky < 3; ++ky)
        for (int lane = 0; lane < 64; ++lane) {
            const int r = lane & 31, h = lane >> 5;
            for (int j = 0; j < 8; ++j) {
                const int kx = 2 * h + (j >> 2), c = j & 3;
                const float v = kx < 3 ? w[((r * 4 + c) * 3 + ky) * 3 + kx] * scale : 0.0f;
                split_f16(v, &o[(((size_t)ky * 2 + 0) * 64 + lane) * 8 + j], &o[(((size_t)ky * 2 + 1) * 64 + lane) * 8 + j]);
            }
        }
    return out;
}

// FC weights for k_heads_split: w [n_out][k_in] row-major * scale = hi + lo (scale as in pack_split), packed
// [32-output tile][K-step][hi | lo][lane] x 8 f16: lane = h*32 + c holds W[32*tile + c][16*step + 8*h + j], the B
// fragment of v_mfma_f32_32x32x16_f16; zero beyond n_out / k_in.
inline std::vector<float> pack_split_fc(const float *w, int n_out, int k_in, int tiles, int steps, float *scale_out) {
    const float scale = *scale_out = weight_scale(w, (size_t)n_out * k_in);
    std::vector<float> out(((size_t)tiles * steps + 1) * 2 * 64 * 4, 0.0f);  // + one all-zero K-step
    _Float16 *o = reinterpret_cast<_Float16 *>(out.data());
    for (int t = 0; t < tiles; ++t)
        for (int st = 0; st < steps; ++st)
            for (int lane = 0; lane < 64; ++lane) {
                const int c = lane & 31, h = lane >> 5, row = 32 * t + c;
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * st + 8 * h + j;
                    const float v = (row < n_out && k < k_in) ? w[(size_t)row * k_in + k] * scale : 0.0f;
                    split_f16(v, &o[((((size_t)t * steps + st) * 2 + 0) * 64 + lane) * 8 + j],
                              &o[((((size_t)t * steps + st) * 2 + 1) * 64 + lane) * 8 + j]);
                }
            }
    return out;
}

// Activation bounds for observation planes in [0, 1] (the MCTS leaves: 0 / 1): a ReLU output is at most its
// bias plus the positive weights times the bounds of their inputs (`in`; NULL: 1 each).  -> the largest bound of the layer,
// infinite when a weight or bias is inf / nan; out[c]: the bound of output channel c.
inline double layer_bound(const float *w, const float *bias, int cout, int cin, int taps, const double *in, double *out) {
    double top = 0.0;
    for (int c = 0; c < cout; ++c) {
        double acc = bias[c] > 0.0f ? (double)bias[c] : 0.0;
        for (int i = 0; i < cin; ++i)
            for (int t = 0; t < taps; ++t) {
                const double wv = w[((size_t)c * cin + i) * taps + t];
                if (wv > 0.0) acc += wv * (in ? in[i] : 1.0);
                else if (!(wv <= 0.0)) acc = INFINITY;  // nan
            }
        out[c] = acc;
        top = std::fmax(top, acc);
        if (!(acc >= 0.0)) top = INFINITY;
    }
    return top;
}

// Each layer's f16 pieces are stored times the largest power of two <= 16 that keeps bound * scale below 60000, so NO
// activation of such an input can leave the f16 range (the pieces of a value of size z carry an absolute error of
// max(2^-22 z, 2^-25): a bound 1000x above the real activations still leaves the error below f32 rounding).
inline float act_scale(double bound) {
    if (!(bound * kMaxActScale >= kF16Room)) return kMaxActScale;  // also bound == 0
    int e = 0;
    (void)std::frexp(kF16Room / bound, &e);   // kF16Room / bound = f * 2^e, f in [0.5, 1)
    return std::ldexp(1.0f, e - 1);            // the largest power of two <= kF16Room / bound
}

// the NetDev fields the preparation reads (rz_net_create): S cells, A policy outputs (Npad: padded to 32), groups_*: K / 16 of the FC layers
struct Shape { int S, A, Npad, groups_act, groups_val; };

// Everything rz_net_load uploads that is not a plain copy of a parameter tensor (the fields of NetDev of these names), and what it keeps.
struct Prepared {
    std::vector<float> w1, w2, w3, u2f, u3f, s2, s3, s1, t2, t3, t3f, fs_act, fs_val;   // the packers' outputs
    std::vector<float> s_inv;                          // [8]: NetDev::s_inv
    std::vector<float> wh, whp, bh;                    // the 1 x 1 head convolutions: [6][128] (act_conv1's 4 rows, then val_conv1's 2), [128][6], [6]
    std::vector<float> fc_act_w, fc_act_b, fc_val1_w;  // act_fc1 zero padded to [Npad][16 * groups_act], [Npad]; val_fc1.weight to [64][16 * groups_val]
    std::vector<float> w1t;                            // val_fc1.weight as [vf_groups][64][4], zero padded (rz_value_head)
    int vf_groups = 0;                                 // K / 4 of the value head's first layer: 16, 32, 64 or 128
    bool split_ok = true;                              // finite activation bounds: the split-f16 trunk cannot overflow
    float range_info[8] = {0};                         // rz_net_range_info: the bounds t1, t2, tf, the scales a1, a2, a3, split_ok, 0
};

// p: the 16 tensors in the order of PolicyValueNet.state_dict(): conv1.w,b conv2.w,b conv3.w,b act_conv1.w,b
// act_fc1.w,b val_conv1.w,b val_fc1.w,b val_fc2.w,b
inline Prepared prepare(const float *const *p, const Shape &D) {
    Prepared P;
    const int S = D.S;
    P.w1 = pack_conv(p[0], 32, 4);
    P.w2 = pack_conv(p[2], 64, 32);
    P.w3 = pack_conv(p[4], 128, 64);
    P.u2f = pack_wino_f4(p[2], 64, 32);
    P.u3f = pack_wino_f4(p[4], 128, 64);
    float sw1 = 1.0f, sw2 = 1.0f, sw3 = 1.0f, sfa = 1.0f, sfv = 1.0f;
    P.s2 = pack_split(p[2], 64, 32, &sw2);
    P.s3 = pack_split(p[4], 128, 64, &sw3);
    P.t2 = pack_rows(p[2], 64, 32, sw2);
    P.t3 = pack_rows(p[4], 128, 64, sw3);
    P.t3f = pack_rows_f8(p[4], 128, 64, sw3);
    P.s1 = pack_split1(p[0], &sw1);
    P.fs_act = pack_split_fc(p[8], D.A, 4 * S, D.Npad / 32, D.groups_act, &sfa);
    P.fs_val = pack_split_fc(p[12], 64, 2 * S, 2, D.groups_val, &sfv);
    {   // Without finite bounds (inf / nan weights) the net runs on the exact-f32 direct trunk instead.
        double b1v[32], b2v[64], b3v[128], bfv[6];
        const double t1 = layer_bound(p[0], p[1], 32, 4, 9, nullptr, b1v);
        const double t2 = layer_bound(p[2], p[3], 64, 32, 9, b1v, b2v);
        (void)layer_bound(p[4], p[5], 128, 64, 9, b2v, b3v);
        double tf = layer_bound(p[6], p[7], 4, 128, 1, b3v, bfv);
        tf = std::fmax(tf, layer_bound(p[10], p[11], 2, 128, 1, b3v, bfv + 4));
        P.split_ok = std::isfinite(t1) && std::isfinite(t2) && std::isfinite(tf) && t1 < 1e30 && t2 < 1e30 && tf < 1e30;
        const float a1 = P.split_ok ? act_scale(t1) : kMaxActScale, a2 = P.split_ok ? act_scale(t2) : kMaxActScale,
                    a3 = P.split_ok ? act_scale(tf) : kMaxActScale;
        const float info[8] = {(float)t1, (float)t2, (float)tf, a1, a2, a3, P.split_ok ? 1.0f : 0.0f, 0.0f};
        memcpy(P.range_info, info, sizeof(info));
        P.s_inv = {a2 / (a1 * sw2), 1.0f / (a2 * sw3), a1 / (kObsScale * sw1), 1.0f / (a3 * sfa), 1.0f / (a3 * sfv), a1, a2, a3};
    }
    P.wh.resize(6 * 128);
    P.bh.resize(6);
    memcpy(P.wh.data(), p[6], 4 * 128 * sizeof(float));
    memcpy(P.wh.data() + 4 * 128, p[10], 2 * 128 * sizeof(float));
    memcpy(P.bh.data(), p[7], 4 * sizeof(float));
    memcpy(P.bh.data() + 4, p[11], 2 * sizeof(float));
    P.whp.resize(128 * 6);
    for (int c = 0; c < 128; ++c)
        for (int o = 0; o < 6; ++o) P.whp[c * 6 + o] = P.wh[o * 128 + c];
    {
        const size_t ld = (size_t)16 * D.groups_act;
        P.fc_act_w.assign((size_t)D.Npad * ld, 0.0f);
        P.fc_act_b.assign((size_t)D.Npad, 0.0f);
        for (int j = 0; j < D.A; ++j) {
            P.fc_act_b[j] = p[9][j];
            memcpy(&P.fc_act_w[(size_t)j * ld], p[8] + (size_t)j * 4 * S, (size_t)4 * S * sizeof(float));
        }
    }
    {
        const size_t ld = (size_t)16 * D.groups_val;
        P.fc_val1_w.assign((size_t)64 * ld, 0.0f);
        for (int j = 0; j < 64; ++j) memcpy(&P.fc_val1_w[(size_t)j * ld], p[12] + (size_t)j * 2 * S, (size_t)2 * S * sizeof(float));
    }
    {   // the value head's first layer for the tree step of the deferred route: [group of 4 inputs][hidden unit][4]
        // four waves x two halves x PER groups of 4 inputs, PER = 2, 4, 8 or 16 (k_tree_step_def): 64 .. 512 inputs
        const int need = (2 * S + 3) / 4;
        P.vf_groups = need <= 16 ? 16 : need <= 32 ? 32 : need <= 64 ? 64 : 128;
        P.w1t.assign((size_t)P.vf_groups * 64 * 4, 0.0f);
        for (int j = 0; j < 64; ++j)
            for (int k = 0; k < 2 * S; ++k) P.w1t[((size_t)(k / 4) * 64 + j) * 4 + k % 4] = p[12][(size_t)j * 2 * S + k];
    }
    return P;
}

}  // namespace rzp
