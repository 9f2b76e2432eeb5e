// rz_forced.h -- forced playouts and policy target pruning (Wu 2019, "Accelerating Self-Play Learning in Go", section 3.2) for the
// root of a PUCT search: everything about them that is neither a kernel launch nor a memory access.  Plain C++, no HIP include, so
// that the CPU can test it against tests/forced_twin.py (tests/test_forced_host.py); the kernels call these functions
// (rz_tree.h: scan_children at the root; rz_engine_play.h: k_root_pruned).  All fp64, each operation rounded once: the including
// translation units are compiled with -ffp-contract=off, and the pragma below says so again.
//
// Notation: N the visit count of the root RECORD (the N whose square root the PUCT term uses -- under tree reuse whatever the record
// holds, not the sum of the children); n, w, p a child's visit count, value sum and stored float32 prior (the noised one where noise
// is on); c = c_puct; k > 0 the forced-playout constant (the paper's 2).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RZF_FN __host__ __device__ __forceinline__
#else
#define RZF_FN inline
#endif

#pragma clang fp contract(off)

namespace rzf {

// node.py:105-117 with Q = 0 at N = 0: q + c * (p * sqrt(parent N) / (n + 1)), evaluated in this order (rz_tree.h's puct IS this)
RZF_FN double puct(double w, int n, float prior, double sqrt_parent, double c) {
    const double q = n > 0 ? w / (double)n : 0.0;
    const double u = ((double)prior * sqrt_parent) / (double)(n + 1);
    const double cu = c * u;
    return q + cu;
}

// (k p) N, the square of the forced-playout floor (k p N)^1/2; no square root is taken anywhere
RZF_FN double floor_sq(float p, int32_t N, double k) { return (k * (double)p) * (double)N; }

// A root child the search has touched and that has fewer visits than its floor: it is selected whatever its score (+infinity in
// the root's scan; several forced children resolve by the scan's first-maximum rule).
RZF_FN bool forced(int32_t n, float p, int32_t N, double k) {
    const double nd = (double)n;
    return n > 0 && nd * nd < floor_sq(p, N, k);
}

// min(f, n) for f the largest integer with f f <= t: the most playouts pruning may take from a child of n > 0 visits.  t >= n n
// answers n without a root; below that f < n < 2^31, so f f is exact and the two loops repair the last place of sqrt's rounding.
RZF_FN int32_t forced_most(double t, int32_t n) {
    const double nd = (double)n;
    if (!(t < nd * nd)) return n;
    if (!(t >= 1.0)) return 0;
    int64_t f = (int64_t)__builtin_sqrt(t);
    while (f > 0 && (double)f * (double)f > t) f -= 1;
    while ((double)(f + 1) * (double)(f + 1) <= t) f += 1;
    return (int32_t)(f < (int64_t)n ? f : (int64_t)n);
}

// The pruned count of one child that is NOT the best one (the best child -- the first with the largest n -- keeps its n; s_best is
// its puct).  q = w / n is held constant; at most f times, while m > 0, a playout is taken away when the child's PUCT at count m - 1
// stays below s_best.  A child left with a single playout is dropped, whether or not anything was subtracted.
RZF_FN int32_t pruned_child(int32_t n, double w, float p, int32_t N, double sqrt_parent, double k, double c, double s_best) {
    if (n <= 0) return 0;
    const int32_t most = forced_most(floor_sq(p, N, k), n);
    const double q = w / (double)n;
    const double ps = (double)p * sqrt_parent;
    int32_t m = n;
    for (int32_t i = 0; i < most && m > 0; ++i) {
        const double u = ps / (double)m;
        const double cu = c * u;
        if (q + cu < s_best) m -= 1;
        else break;
    }
    return m == 1 ? 0 : m;
}

// first child with the largest n (K >= 1)
RZF_FN int best_child(const int32_t *n, int K) {
    int b = 0;
    for (int r = 1; r < K; ++r)
        if (n[r] > n[b]) b = r;
    return b;
}

// The whole root at once (the CPU's use and the statement the kernel is held to; k_root_pruned places a child per lane through
// pruned_child): out[r] for the K children in rank order.  A root without a visited child comes back as it is (all zero).
RZF_FN void pruned_counts(const int32_t *n, const double *w, const float *p, int K, int32_t N, double sqrt_parent, double k, double c,
                          int32_t *out) {
    if (K <= 0) return;
    const int b = best_child(n, K);
    const double s_best = puct(w[b], n[b], p[b], sqrt_parent, c);
    for (int r = 0; r < K; ++r) out[r] = r == b ? (n[r] > 0 ? n[r] : 0) : pruned_child(n[r], w[r], p[r], N, sqrt_parent, k, c, s_best);
}

}  // namespace rzf
