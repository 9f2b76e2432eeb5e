// rz_mz_pack.h -- what rz_mz_load_model and rz_mz_load_representation compute on the host between their argument checks and their upload:
// the weights of the MuZero network (rlzero_amd/muzero/network.py, hidden size 64) in the layouts k_mz_search reads (rz_muzero_search.h),
// the power-of-two scales of the f16 layers of whole moves, the bound on relu(dyn1) that gives their activation scale, and the verdict
// whether whole moves may run at all.  Pure CPU arithmetic, no HIP: plain C++17, included by rz_muzero.hip (through the headers that
// need the sizes below) and by the driver of tests/test_mz_pack.py, which restates every layout, scale and bound in numpy.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

namespace rzmp {

// the sizes the fused search is built for: floats of a hidden state, the most actions, the most observation features (rep1's rows)
constexpr int kMzH = 64, kMzMaxA = 8, kMzObs = 8;

// The power of two that brings a layer's largest weight `wmax` into [2^13, 2^14) (1 for a layer of zeros, or a wmax that is inf or nan;
// inf for a wmax below 2^-114, subnormals among them: float32 has no such power and ldexp overflows)
inline float pow2_for(float wmax) {
    int ex = 0;
    if (wmax > 0.0f && std::isfinite(wmax)) {
        (void)std::frexp(wmax, &ex);
        ex = 14 - ex;   // wmax * 2^ex in [2^13, 2^14)
    }
    return std::ldexp(1.0f, ex);
}

// The largest |w| of a 64-unit layer w [64][n_in] (torch layout [out][in]) over its first 64 input columns: the columns the f16 matrix
// pipe multiplies (dyn1's one-hot action columns, 64 .. n_in - 1, stay f32 and do not count)
inline float wmax_of(const float *w, int n_in) {
    float m = 0.0f;
    for (int o = 0; o < kMzH; ++o)
        for (int k = 0; k < kMzH; ++k) m = std::fmax(m, std::fabs(w[(size_t)o * n_in + k]));
    return m;
}

// relu(dyn1 [state in [0, 1], one-hot action]) <= |bias| + the positive state weights + the largest action weight (0 if none is
// positive), per unit in that order in fp64; the maximum over the 64 units.  w [64][64 + A], b [64]
inline double relu_dyn1_bound(const float *w, const float *b, int A) {
    const int KX = kMzH + A;
    double bound = 0.0;
    for (int o = 0; o < kMzH; ++o) {
        double acc = std::fabs((double)b[o]), amax = 0.0;
        for (int k = 0; k < kMzH; ++k) acc += std::fmax(0.0, (double)w[(size_t)o * KX + k]);
        for (int a = 0; a < A; ++a) amax = std::fmax(amax, (double)w[(size_t)o * KX + kMzH + a]);
        bound = std::fmax(bound, acc + amax);
    }
    return bound;
}

// The scale of relu(dyn1)'s f16 pieces: 16 while bound * 16 stays below 60000, else 2^(e - 1) where 60000 / bound = f 2^e, f in [0.5, 1):
// the largest power of two with bound * s1 <= 60000 (equal only where 60000 / bound is itself a power of two; f16 holds 65504).  A bound
// that is nan, inf or not positive counts as 1e30 there
inline float s1_for(double bound) {
    float s1 = 16.0f;
    if (!(bound * 16.0 < 60000.0)) {
        int ex = 0;
        (void)std::frexp(60000.0 / (std::isfinite(bound) && bound > 0.0 ? bound : 1e30), &ex);
        s1 = std::ldexp(1.0f, ex - 1);
    }
    return s1;
}

// rz_mz_load_model's upload.  The 14 tensors p[i] in torch layout [out][in], in this order:
//   dyn1.w [H][H+A], dyn1.b, dyn2.w [H][H], dyn2.b, rew1.w [H][H], rew1.b, rew2.w [1][H], rew2.b, pre1.w [H][H], pre1.b,
//   pol.w [A][H], pol.b [A], val.w [1][H], val.b                                                                   (H = 64)
// Tensor i lies at off[i] of `host`, padded with zeros to a multiple of 4 floats.  The big matrices dyn1.w, dyn2.w, rew1.w, pre1.w
// go k-major, w[k][unit] = torch w[unit][k] (dyn1.w: [H+A][H], its action rows last); every other tensor is copied as it is (pol.w
// stays [A][H]).  Behind them, at off_scales, 8 floats: [0..3] pow2_for(wmax_of) of dyn1, dyn2, rew1, pre1 (MzModel::f16_scales),
// [4] s1_for(relu_dyn1_bound), [5..7] zero.
struct Model {
    std::vector<float> host;
    size_t off[14], off_scales;
    // the f16 pieces of whole MOVES cannot overflow when the weights are finite: hidden states are min-max scaled to [0, 1]
    // (stored x 16), relu(dyn1) is stored x s1 with bound x s1 < 60000, every weight x its power of two lies below 2^14.  Weights
    // WITHOUT finite values give no such bound: the whole-moves route then refuses to run (rz_mz_play_env) instead of
    // filling the trees with inf -- the move-by-move routes (f32-input MFMA, PyTorch-ROCm) remain.
    bool f16_ok;   // every value of the 14 tensors and the bound are finite
};

inline Model pack_model(const float *const *p, int A) {
    const int KX = kMzH + A;
    const size_t sizes[14] = {(size_t)KX * kMzH, kMzH, (size_t)kMzH * kMzH, kMzH, (size_t)kMzH * kMzH, kMzH, kMzH, 1,
                              (size_t)kMzH * kMzH, kMzH, (size_t)A * kMzH, (size_t)A, kMzH, 1};
    Model m;
    size_t total = 0;
    for (int i = 0; i < 14; ++i) {
        m.off[i] = total;
        total += (sizes[i] + 3) / 4 * 4;
    }
    m.off_scales = total;
    total += 8;
    m.host.assign(total, 0.0f);
    auto transpose = [&](int idx, int n_out, int n_in) {
        for (int o = 0; o < n_out; ++o)
            for (int k = 0; k < n_in; ++k) m.host[m.off[idx] + (size_t)k * n_out + o] = p[idx][(size_t)o * n_in + k];
    };
    transpose(0, kMzH, KX);
    transpose(2, kMzH, kMzH);
    transpose(4, kMzH, kMzH);
    transpose(8, kMzH, kMzH);
    for (int i : {1, 3, 5, 6, 7, 9, 10, 11, 12, 13})
        for (size_t q = 0; q < sizes[i]; ++q) m.host[m.off[i] + q] = p[i][q];
    // the f16 layers of whole MOVES (MzModel::f16_scales)
    m.host[m.off_scales + 0] = pow2_for(wmax_of(p[0], KX));
    m.host[m.off_scales + 1] = pow2_for(wmax_of(p[2], kMzH));
    m.host[m.off_scales + 2] = pow2_for(wmax_of(p[4], kMzH));
    m.host[m.off_scales + 3] = pow2_for(wmax_of(p[8], kMzH));
    const double bound = relu_dyn1_bound(p[0], p[1], A);
    m.host[m.off_scales + 4] = s1_for(bound);
    bool finite = std::isfinite(bound);
    for (int i = 0; i < 14 && finite; ++i)
        for (size_t q = 0; q < sizes[i]; ++q)
            if (!std::isfinite(p[i][q])) {
                finite = false;
                break;
            }
    m.f16_ok = finite;
    return m;
}

// rz_mz_load_representation's upload, from rep1.w [H][obs_dim], rep1.b, rep2.w [H][H], rep2.b (torch layout [out][in]):
// off[0] rep1.w k-major as [kMzObs][H], w[k][unit] = torch w[unit][k], rows obs_dim .. kMzObs - 1 zero (the search multiplies all eight
// rows; observations past obs_dim are zero as well); off[1] rep1.b; off[2] rep2.w k-major [H][H]; off[3] rep2.b.  No padding: every
// piece is a multiple of 4 floats.
struct Representation {
    std::vector<float> host;
    size_t off[4];
};

inline Representation pack_representation(const float *const *p, int obs_dim) {
    Representation r = {{}, {0, (size_t)kMzObs * kMzH, (size_t)kMzObs * kMzH + kMzH, (size_t)kMzObs * kMzH + kMzH + (size_t)kMzH * kMzH}};
    r.host.assign(r.off[3] + kMzH, 0.0f);
    for (int o = 0; o < kMzH; ++o) {
        for (int k = 0; k < obs_dim; ++k) r.host[r.off[0] + (size_t)k * kMzH + o] = p[0][(size_t)o * obs_dim + k];
        for (int k = 0; k < kMzH; ++k) r.host[r.off[2] + (size_t)k * kMzH + o] = p[2][(size_t)o * kMzH + k];
        r.host[r.off[1] + o] = p[1][o];
        r.host[r.off[3] + o] = p[3][o];
    }
    return r;
}

}  // namespace rzmp
