"""csrc/rz_mz_gumbel.h -- the rules the GUMBEL instantiations of k_mz_search compile -- as a stand-alone driver (plain and with
-fsanitize=address,undefined: tests/host_driver.py) against rlzero_amd/muzero/gumbel.py: the considered-visits table for every (m, n)
with m in 1..8 and n in 1..64, and v_mix, the completed values, s, pi' and the three decisions on 300 random nodes plus crafted ones.
Integers and decisions are equal; doubles agree within 1e-12 (exp and log of the C library and of CPython / numpy may differ in the
last place, every other operation is ordered identically)."""
import numpy as np

import host_driver
from rlzero_amd.muzero import gumbel as G

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rz_mz_gumbel.h"
template <typename T> std::vector<T> rd(const char *p) {
    FILE *f = fopen(p, "rb"); if (!f) exit(2);
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<T> v(n / sizeof(T)); if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(3); fclose(f); return v;
}
template <typename T> void wr(const char *p, const std::vector<T> &v) { FILE *f = fopen(p, "wb"); fwrite(v.data(), sizeof(T), v.size(), f); fclose(f); }
int main(int argc, char **argv) {
    if (!strcmp(argv[1], "schedule")) {   // schedule <out>: cv of every (m, n), m = 1..8, n = 1..64, one after the other
        std::vector<int32_t> all;
        for (int m = 1; m <= 8; ++m) for (int n = 1; n <= 64; ++n) { std::vector<int32_t> cv(n); rzmzg::considered_visits(m, n, cv.data()); all.insert(all.end(), cv.begin(), cv.end()); }
        wr(argv[2], all);
        return 0;
    }
    // nodes K <ints [K][10]: A, N[8], cv_s> <doubles [K][21]: prior[8], q[8], v_hat, lo, hi, c_visit, c_scale> <floats g [K][8]> <out ints [K][5]> <out doubles [K][25]>
    const int K = atoi(argv[2]);
    const auto I = rd<int32_t>(argv[3]); const auto D = rd<double>(argv[4]); const auto F = rd<float>(argv[5]);
    std::vector<int32_t> oi(K * 5); std::vector<double> od(K * 25);
    for (int k = 0; k < K; ++k) {
        rzmzg::Node nd; rzmzg::Eval ev;
        nd.A = I[k * 10];
        for (int a = 0; a < 8; ++a) { nd.N[a] = I[k * 10 + 1 + a]; nd.prior[a] = D[k * 21 + a]; nd.logit[a] = std::log(nd.prior[a]); nd.q[a] = D[k * 21 + 8 + a]; }
        nd.v_hat = D[k * 21 + 16]; nd.lo = D[k * 21 + 17]; nd.hi = D[k * 21 + 18];
        rzmzg::evaluate(nd, D[k * 21 + 19], D[k * 21 + 20], ev);
        oi[k * 5] = rzmzg::root_action(nd, ev, &F[k * 8], I[k * 10 + 9]); oi[k * 5 + 1] = rzmzg::below_action(nd, ev);
        oi[k * 5 + 2] = rzmzg::final_action(nd, ev, &F[k * 8]); oi[k * 5 + 3] = ev.sum_n; oi[k * 5 + 4] = ev.max_n;
        od[k * 25] = ev.vmix;
        for (int a = 0; a < 8; ++a) { od[k * 25 + 1 + a] = ev.cq[a]; od[k * 25 + 9 + a] = ev.s[a]; od[k * 25 + 17 + a] = ev.pi[a]; }
    }
    wr(argv[6], oi); wr(argv[7], od);
    return 0;
}
'''
drv = host_driver.fixture('mz_gumbel', DRIVER)


def test_the_considered_visits_of_every_m_and_n(drv):
    got = np.fromfile(drv.same(['schedule'], 1)[0], dtype=np.int32)
    want = np.concatenate([G.considered_visits(m, n) for m in range(1, 9) for n in range(1, 65)])
    assert np.array_equal(got, want)
    assert G.considered_visits(1, 5).tolist() == [0, 1, 2, 3, 4]
    assert G.considered_visits(4, 16).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]   # 2 phases: 4 x 2, then 2 x 4
    assert G.considered_visits(3, 2).tolist() == [0, 0]   # a budget below m


def node(A, N, prior, q, v_hat=0.3, lo=-1.0, hi=2.0, cv_s=0, g=None, c_visit=50.0, c_scale=1.0):
    pad = lambda x, fill: list(x) + [fill] * (8 - len(x))   # noqa: E731
    return ([A] + pad(N, 0) + [cv_s], pad(prior, 0.0) + pad(q, 0.0) + [v_hat, lo, hi, c_visit, c_scale], pad(g if g is not None else [0.0] * A, 0.0))


def nodes():
    rng = np.random.default_rng(7)
    out = [node(4, [0, 0, 0, 0], [0.1, 0.2, 0.3, 0.4], [0, 0, 0, 0], g=[0.5, -0.2, 0.1, 0.0]),            # nothing visited
           node(3, [2, 1, 4], [0.5, 0.3, 0.2], [0.4, -0.3, 1.1], cv_s=1, g=[0.1, 0.2, 0.3]),               # everything visited
           node(3, [1, 0, 0], [0.6, 0.0, 0.4], [0.2, 0.0, 0.0], g=[0.0, 9.0, 0.0]),                        # one zero prior
           node(5, [1, 0, 2, 0, 0], [0.2] * 5, [0.5, 0, 0.5, 0, 0], lo=0.5, hi=0.5, g=[0.3, 0.1, 0.2, 0.1, 0.0]),   # lo == hi
           node(4, [1, 0, 0, 1], [0.25] * 4, [0.7, 0, 0, 0.7], cv_s=0, g=[0.0, 0.5, 0.5, 0.0])]            # an exact tie: 2 beats 1
    for _ in range(300):
        A = int(rng.integers(1, 9))
        N = (rng.integers(0, 6, A) * (rng.random(A) < 0.6)).astype(int)
        prior = rng.dirichlet(np.ones(A))
        lo, hi = sorted(rng.normal(0.0, 1.0, 2))
        out.append(node(A, N.tolist(), prior.tolist(), rng.normal(0.0, 1.0, A).tolist(), float(rng.normal()), float(lo), float(hi),
                        int(rng.choice(N)), rng.gumbel(size=A).astype(np.float32).tolist(), float(rng.choice([50.0, 0.0, 7.5])),
                        float(rng.choice([1.0, 0.1]))))
    return out


def test_nodes_against_the_python_restatement(drv):
    cases = nodes()
    I = np.array([c[0] for c in cases], dtype=np.int32)
    D = np.array([c[1] for c in cases], dtype=np.float64)
    F = np.array([c[2] for c in cases], dtype=np.float32)
    oi, od = drv.run('nodes', [len(cases)], [I, D, F], [np.int32, np.float64])
    oi, od = oi.reshape(-1, 5), od.reshape(-1, 25)
    for k in range(len(cases)):
        A, N, cv_s = int(I[k, 0]), I[k, 1:1 + int(I[k, 0])].tolist(), int(I[k, 9])
        with np.errstate(divide='ignore'):
            logit = np.log(D[k, :A])
        ev = G.evaluate(N, D[k, :A], logit, D[k, 8:8 + A], D[k, 16], D[k, 17], D[k, 18], D[k, 19], D[k, 20])
        want = [G.pick(G.root_scores(N, ev, F[k], cv_s))[0], G.pick(G.below_scores(N, ev))[0], G.pick(G.root_scores(N, ev, F[k], ev['max_n']))[0],
                ev['sum_n'], ev['max_n']]
        assert oi[k].tolist() == want, (k, oi[k], want)
        assert abs(od[k, 0] - ev['vmix']) <= 1e-12
        for name, off in (('cq', 1), ('s', 9), ('pi', 17)):
            got, ref = od[k, off:off + A], np.array(ev[name])
            same_inf = np.isinf(ref) & (got == ref)
            assert (same_inf | (np.abs(np.where(same_inf, 0.0, got) - np.where(same_inf, 0.0, ref)) <= 1e-12)).all(), (k, name, got, ref)
        assert abs(sum(ev['pi']) - 1.0) <= 1e-12
    # the crafted nodes, by what they are there for
    assert od[0, 0] == 0.3 and oi[0, 3] == 0                              # nothing visited: v_mix is v_hat
    assert od[2, 17 + 1] == 0.0 and od[2, 9 + 1] == -np.inf and oi[2, 0] != 1   # a zero prior: pi' 0, never the root's action despite g = 9
    assert np.array_equal(od[3, 1:6], [0.5, od[3, 0], 0.5, od[3, 0], od[3, 0]])     # lo == hi: the completed values are not rescaled
    assert oi[4, 0] == 2                                                  # the tie between actions 1 and 2 goes to the larger
