// rz_mz_support.h -- MuZero's categorical value and reward heads (arXiv:1911.08265v2 appendix F): ONE copy of the rule for the search
// (rz_muzero_search.h: the CAT instantiations of k_mz_search read a head's logits through chunk_max / chunk_sums / combine4 below), for
// the packing of the wider heads (rz_mz_pack.h) and for the CPU, which tests it bit for bit against the Python twin
// rlzero_amd/muzero/support.py (tests/test_mz_support_host.py).  Plain C++, no HIP include, as rz_mz_value.h and rz_mz_gumbel.h.
//
// A support of half-width S, 1 <= S <= 31, has B = 2 S + 1 bins at the integers -S .. S: B <= 63, one bin per lane of a wave.  A head
// is a softmax over the bins; the number it stands for is the expectation sum_i p_i (i - S), in the transformed space of rz_mz_value.h
// (the search takes it through rzmzv::value_h_inv; the learner's targets are two_hot(h(target))).
//
// The ONE summation order of `expectation`.  The bins are padded to kLanes = 64 terms; a padding term (bin >= B) is exactly 0 in both sums
// and takes no part in the maximum.  The 64 terms fall into 4 chunks of 16 consecutive bins, chunk c = bins 16 c .. 16 c + 15:
//   m     = the largest logit
//   e_i   = exp(x_i - m)                                               (fp64, the widened float32 logit)
//   den_c = ((0 + e_16c) + e_16c+1) + ... + e_16c+15                   (left to right)
//   num_c = ((0 + e_16c (16c - S)) + e_16c+1 (16c + 1 - S)) + ...      (one product, one sum per bin, left to right)
//   den   = (den_0 + den_1) + (den_2 + den_3),  num likewise           (combine4)
//   expectation = num / den
// fp64 throughout, one rounding per operation (-ffp-contract=off).  In the kernel four lanes serve a game, lane c its chunk c; combine4 is
// two lane exchanges (c ^ 1, then c ^ 2), which gives every lane (s_c + s_c^1) + (s_c^2 + s_c^3): the same bits as above, since IEEE
// addition commutes.  (exp is the platform's: glibc's on the host, which CPython's math.exp calls too, the device library's in the kernel;
// the two may differ in the last bit of a term, the order of the sums does not.)
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define RZS_FN __host__ __device__ inline __attribute__((always_inline))   // (no HIP header here: __forceinline__ is the runtime's macro)
#else
#define RZS_FN inline
#endif

#pragma clang fp contract(off)

namespace rzmzs {

constexpr int kMinS = 1, kMaxS = 31, kLanes = 64, kChunk = 16, kChunks = 4;

RZS_FN constexpr bool support_ok(int S) { return S >= kMinS && S <= kMaxS; }
RZS_FN constexpr int bins(int S) { return 2 * S + 1; }

// the two-hot encoding of y: clamped to [-S, S], lo = floor(y), w_hi = y - lo on bin lo + 1, w_lo = 1 - w_hi on bin lo (bins count from
// 0 at -S).  At y == S the lower bin is the last one and carries all the weight: *lo_bin + 1 is then past the end and w_hi is 0 -- a
// caller adds w_hi only where it is positive (dense does).  A nan clamps to -S.
RZS_FN void two_hot(double y, int S, int *lo_bin, double *w_lo, double *w_hi) {
    const double s = (double)S;
    y = y > -s ? y : -s;   // (also takes nan)
    y = y < s ? y : s;
    const double lo = __builtin_floor(y);
    *w_hi = y - lo;
    *w_lo = 1.0 - *w_hi;
    *lo_bin = (int)lo + S;
}

// two_hot as a dense row of B weights
RZS_FN void dense(double y, int S, double *row) {
    int lo;
    double w_lo, w_hi;
    two_hot(y, S, &lo, &w_lo, &w_hi);
    for (int i = 0; i < bins(S); ++i) row[i] = 0.0;
    row[lo] = w_lo;
    if (w_hi > 0.0) row[lo + 1] = w_hi;
}

// the largest of chunk c's logits (x: the chunk's 16 logits; bins >= B do not count); -inf for a chunk of padding alone
template <typename T>
RZS_FN double chunk_max(const T *x, int c, int S) {
    double m = -__builtin_inf();
#pragma unroll 1
    for (int j = 0; j < kChunk; ++j) {
        const double v = kChunk * c + j < bins(S) ? (double)x[j] : -__builtin_inf();
        m = v > m ? v : m;
    }
    return m;
}

// den_c and num_c of chunk c (x: the chunk's 16 logits, m: the largest logit of the head)
template <typename T>
RZS_FN void chunk_sums(const T *x, int c, int S, double m, double *den, double *num) {
    double d = 0.0, u = 0.0;
#pragma unroll 1   // (one exp at a time: in the search kernel sixteen in flight spill registers)
    for (int j = 0; j < kChunk; ++j) {
        const int i = kChunk * c + j;
        const double e = i < bins(S) ? ::exp((double)x[j] - m) : 0.0;
        d = d + e;
        u = u + e * (double)(i - S);
    }
    *den = d;
    *num = u;
}

RZS_FN double combine4(double s0, double s1, double s2, double s3) { return (s0 + s1) + (s2 + s3); }

// the expectation of a head from its logits x[kLanes] (entries >= B are not read as values)
template <typename T>
RZS_FN double expectation(const T *x, int S) {
    double m = -__builtin_inf(), den[kChunks], num[kChunks];
    for (int c = 0; c < kChunks; ++c) {
        const double mc = chunk_max(x + kChunk * c, c, S);
        m = mc > m ? mc : m;
    }
    for (int c = 0; c < kChunks; ++c) chunk_sums(x + kChunk * c, c, S, m, &den[c], &num[c]);
    return combine4(num[0], num[1], num[2], num[3]) / combine4(den[0], den[1], den[2], den[3]);
}

// the bias of a padding row of a packed head (rz_mz_pack.h): with zero weights its logit is -inf whatever the (finite) activations,
// its term exp(-inf - m) is exactly 0 and it never is the maximum
RZS_FN float pad_bias() { return -__builtin_inff(); }

}  // namespace rzmzs
