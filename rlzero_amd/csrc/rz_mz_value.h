// rz_mz_value.h -- MuZero's invertible value transform (arXiv:1911.08265v2 appendix F; R2D2's h): ONE copy of the rule for the search
// (rz_muzero_search.h: k_mz_search<..., VT> applies value_h_inv to the network's reward and value before the backup) and for the learner's
// targets (rz_mz_target.h: unroll_row<VT> applies value_h to the n-step return and the stored reward).  Plain C++, no HIP include,
// so that the CPU can test it against the Python twin tests/mz_value_twin.py bit for bit (tests/test_mz_value_transform_host.py).
//   h(x)    = sign(x) (sqrt(|x| + 1) - 1) + eps x
//   h^-1(y) = sign(y) (((sqrt(1 + 4 eps (|y| + 1 + eps)) - 1) / (2 eps))^2 - 1)
// eps = 0.001, a constant.  fp64 throughout, one rounding per operation in the order written below (-ffp-contract=off; IEEE sqrt on
// host and device): a caller that holds float32 widens before the call and rounds once after it.  Both are odd; h^-1(h(x)) = x within
// 1e-11 max(1, |x|) (the cancellation in sqrt(..) - 1 near zero leaves about 2e-13).
#pragma once

#if defined(__HIPCC__)
#define RZV_FN __host__ __device__ __forceinline__
#else
#define RZV_FN inline
#endif

namespace rzmzv {

constexpr double kEps = 0.001;

RZV_FN double value_h(double x) {
    return __builtin_copysign(__builtin_sqrt(__builtin_fabs(x) + 1.0) - 1.0, x) + kEps * x;
}

RZV_FN double value_h_inv(double y) {
    const double a = __builtin_fabs(y);
    const double s = __builtin_sqrt(1.0 + 4.0 * kEps * (a + 1.0 + kEps));
    const double u = (s - 1.0) / (2.0 * kEps);
    return __builtin_copysign(u * u - 1.0, y);
}

}  // namespace rzmzv
