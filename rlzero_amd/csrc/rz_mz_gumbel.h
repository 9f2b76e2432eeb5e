// rz_mz_gumbel.h -- the rules of Gumbel MuZero's search (Danihelka et al., "Policy improvement by planning with Gumbel", ICLR 2022),
// ONE copy for the kernel (rz_muzero_search.h: the GUMBEL instantiations of k_mz_search) and for the CPU (tests/test_mz_gumbel_host.py
// against rlzero_amd/muzero/gumbel.py).  Plain C++, no HIP type; fp64, one rounding per operation in the order written (fp contract off).
//
//   considered visits   cv[s], s = 0 .. n - 1: Sequential Halving over m = min(max_considered, A) actions as ONE table.  ceil(log2 m)
//                       phases; a phase visits every still-considered action max(1, n / (phases * considered)) times, round-robin, then
//                       considered = max(2, considered / 2); the sequence goes on until n entries stand (m = 1: 0, 1, 2, ...).  cv[s] is the
//                       visit count an action must HAVE to be eligible at simulation s, so the root keeps no set: the top-m restriction
//                       (the first m simulations take the m best of g + logit, each once) and the halving fall out of `N(a) == cv[s]`.
//   logit(a)            log(prior(a)) of the stored fp64 prior (softmax and arg-max are shift-invariant); prior 0 -> -inf, never chosen.
//   q(a)                reward(a) + discount * value(a), for N(a) > 0.
//   v_mix               (v_hat + (sumN / SP) * SPQ) / (1 + sumN), SP = sum of prior(b), SPQ = sum of prior(b) q(b) over visited b,
//                       sumN = sum of N(b); v_hat, the node's raw network value, alone when nothing is visited (or SP == 0).
//   cq(a)               normalize(N(a) > 0 ? q(a) : v_mix, lo, hi) with the tree's MinMax bounds (MinMaxStats.normalize).
//   s(a)                logit(a) + ((c_visit + max_b N(b)) * c_scale) * cq(a)
//   pi'(a)              exp(s(a) - max_b s(b)) / sum_b exp(s(b) - max_b s(b))
//   root, simulation s  arg-max over N(a) == cv[s] of g(a) + s(a)              (g: the move's Gumbel draws, float32 widened)
//   below the root      arg-max of pi'(a) - N(a) / (1 + sumN)
//   result              among N(a) == max_b N(b), the arg-max of g(a) + s(a); the target is pi' of the root as float32
// An arg-max is over the pairs (score, action): the larger action wins a tie, as in mz_descend; an action that is not a candidate scores
// -inf, and when every action scores -inf the largest action is taken.
//
// SUMMATION ORDER.  The kernel spreads a node's (at most 8) children over four lanes, lane q holding actions 2q and 2q + 1, and adds
// across lanes as mz_rowsum does (lane q ^ 1, then lane q ^ 2).  Every sum over actions of a term t(a) -- t = 0 for an action past A or
// outside the sum -- is therefore
//       ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7))
// (sum8 below; fp64 addition commutes, so all four lanes hold the same bits).  Maxima and arg-maxima do not depend on an order.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RZG_FN __host__ __device__ __forceinline__
#else
#define RZG_FN inline
#endif

#pragma clang fp contract(off)

namespace rzmzg {

constexpr int kMaxA = 8;   // the fused search's limit

RZG_FN int ceil_log2(int m) {
    int p = 0;
    while ((1 << p) < m) ++p;
    return p;
}

// cv[0 .. n): the considered-visits table of m actions and n simulations
RZG_FN void considered_visits(int m, int n, int32_t *cv) {
    if (m <= 1) {
        for (int s = 0; s < n; ++s) cv[s] = s;
        return;
    }
    const int phases = ceil_log2(m);
    int s = 0, considered = m, base = 0;   // base: the visits every considered action has when a phase begins
    while (s < n) {
        const int per = n / (phases * considered) > 1 ? n / (phases * considered) : 1;
        for (int v = 0; v < per && s < n; ++v)
            for (int k = 0; k < considered && s < n; ++k) cv[s++] = base + v;
        base += per;
        considered = considered / 2 > 2 ? considered / 2 : 2;
    }
}

RZG_FN double normalize(double v, double lo, double hi) { return hi > lo ? (v - lo) / (hi - lo) : v; }   // MinMaxStats.normalize

// a lane's two terms, then the four lanes' partial sums: the one order of every sum over actions
RZG_FN double sum2(double t0, double t1) { return t0 + t1; }
RZG_FN double sum4(double p0, double p1, double p2, double p3) { return (p0 + p1) + (p2 + p3); }
RZG_FN double sum8(const double *t) { return sum4(sum2(t[0], t[1]), sum2(t[2], t[3]), sum2(t[4], t[5]), sum2(t[6], t[7])); }

RZG_FN double v_mix(double v_hat, int sum_n, double sp, double spq) {
    return sum_n > 0 && sp > 0.0 ? (v_hat + ((double)sum_n / sp) * spq) / (1.0 + (double)sum_n) : v_hat;
}
RZG_FN double completed(int n, double q, double vmix, double lo, double hi) { return normalize(n > 0 ? q : vmix, lo, hi); }
RZG_FN double sigma_scale(double c_visit, double c_scale, int max_n) { return (c_visit + (double)max_n) * c_scale; }
RZG_FN double logit_score(double logit, double scale, double cq) { return logit + scale * cq; }   // s(a)
RZG_FN double root_score(float g, double s) { return (double)g + s; }
RZG_FN double below_score(double pi, int n, int sum_n) { return pi - (double)n / (1.0 + (double)sum_n); }
// (score, action) beats (best, best_action)
RZG_FN bool better(double score, int action, double best, int best_action) { return score > best || (score == best && action > best_action); }

// ---- the scalar reference: a node's children in action order, every sum through sum8
struct Node {
    int A, N[kMaxA];
    double prior[kMaxA], logit[kMaxA], q[kMaxA];   // q: reward + discount * value, read where N > 0
    double v_hat, lo, hi;
};
struct Eval {
    int sum_n, max_n;
    double vmix, cq[kMaxA], s[kMaxA], pi[kMaxA];   // (entries past A: 0, -inf, 0)
};

RZG_FN void evaluate(const Node &nd, double c_visit, double c_scale, Eval &ev) {
    double tp[kMaxA], tpq[kMaxA], te[kMaxA];
    ev.sum_n = 0;
    ev.max_n = 0;
    for (int a = 0; a < kMaxA; ++a) {
        const bool seen = a < nd.A && nd.N[a] > 0;
        tp[a] = seen ? nd.prior[a] : 0.0;
        tpq[a] = seen ? nd.prior[a] * nd.q[a] : 0.0;
        if (a < nd.A) {
            ev.sum_n += nd.N[a];
            ev.max_n = nd.N[a] > ev.max_n ? nd.N[a] : ev.max_n;
        }
    }
    ev.vmix = v_mix(nd.v_hat, ev.sum_n, sum8(tp), sum8(tpq));
    const double scale = sigma_scale(c_visit, c_scale, ev.max_n);
    double mx = -INFINITY;
    for (int a = 0; a < kMaxA; ++a) {
        ev.cq[a] = a < nd.A ? completed(nd.N[a], nd.q[a], ev.vmix, nd.lo, nd.hi) : 0.0;
        ev.s[a] = a < nd.A ? logit_score(nd.logit[a], scale, ev.cq[a]) : -INFINITY;
        mx = ev.s[a] > mx ? ev.s[a] : mx;
    }
    for (int a = 0; a < kMaxA; ++a) te[a] = a < nd.A ? std::exp(ev.s[a] - mx) : 0.0;
    const double den = sum8(te);
    for (int a = 0; a < kMaxA; ++a) ev.pi[a] = te[a] / den;
}

// the root's action at a simulation whose considered-visits entry is `cv_s`
RZG_FN int root_action(const Node &nd, const Eval &ev, const float *g, int cv_s) {
    double best = -INFINITY;
    int act = -1;
    for (int a = 0; a < nd.A; ++a) {
        const double sc = nd.N[a] == cv_s ? root_score(g[a], ev.s[a]) : -INFINITY;
        if (better(sc, a, best, act)) {
            best = sc;
            act = a;
        }
    }
    return act;
}

RZG_FN int below_action(const Node &nd, const Eval &ev) {
    double best = -INFINITY;
    int act = -1;
    for (int a = 0; a < nd.A; ++a) {
        const double sc = below_score(ev.pi[a], nd.N[a], ev.sum_n);
        if (better(sc, a, best, act)) {
            best = sc;
            act = a;
        }
    }
    return act;
}

// the move of a finished search
RZG_FN int final_action(const Node &nd, const Eval &ev, const float *g) { return root_action(nd, ev, g, ev.max_n); }

}  // namespace rzmzg
