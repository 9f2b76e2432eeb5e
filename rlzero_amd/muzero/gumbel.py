"""Gumbel MuZero's search rule (Danihelka et al., "Policy improvement by planning with Gumbel", ICLR 2022) restated on the host:
the considered-visits table the library is handed (``MuZeroTree.set_gumbel``) and a float64 twin of the whole search, node by node,
that follows csrc/rz_mz_gumbel.h operation for operation -- its one summation order included -- and is fed network outputs.  The twin
is the arbiter of the kernel's trees (tests/test_mz_gumbel_gpu.py) and of the header's scalar reference (tests/test_mz_gumbel_host.py).
Python floats are IEEE doubles, one rounding per operation; ``exp`` and ``log`` are the C library's."""
import math

import numpy as np

INF = float('inf')


def considered_visits(m, n):
    """cv[s], s = 0 .. n - 1: the visit count a root action must have to be eligible at simulation s -- Sequential Halving of n
    simulations over m actions as one table (rzmzg::considered_visits).  int32 [n]."""
    m, n = int(m), int(n)
    if m <= 1:
        return np.arange(n, dtype=np.int32)
    phases = (m - 1).bit_length()   # ceil(log2 m)
    cv, considered, base = [], m, 0
    while len(cv) < n:
        per = max(1, n // (phases * considered))
        for v in range(per):
            cv.extend([base + v] * considered)
        base += per
        considered = max(2, considered // 2)
    return np.array(cv[:n], dtype=np.int32)


def sum8(t):
    """The one order of every sum over actions: lane q adds its two terms, the lanes add as mz_rowsum does."""
    t = list(t) + [0.0] * (8 - len(t))
    return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))


def evaluate(N, prior, logit, q, v_hat, lo, hi, c_visit=50.0, c_scale=1.0):
    """rzmzg::evaluate of one node's children (sequences of A entries; q is read where N > 0)
    -> dict sum_n, max_n, vmix, cq [A], s [A] = logit + sigma(cq), pi [A]."""
    A = len(N)
    seen = [N[a] > 0 for a in range(A)]
    sum_n, max_n = int(sum(N)), int(max(N))
    sp = sum8([float(prior[a]) if seen[a] else 0.0 for a in range(A)])
    spq = sum8([float(prior[a]) * float(q[a]) if seen[a] else 0.0 for a in range(A)])
    vmix = (v_hat + (float(sum_n) / sp) * spq) / (1.0 + float(sum_n)) if sum_n > 0 and sp > 0.0 else float(v_hat)
    scale = (c_visit + float(max_n)) * c_scale
    cq, s = [], []
    for a in range(A):
        x = float(q[a]) if seen[a] else vmix
        cq.append((x - lo) / (hi - lo) if hi > lo else x)
        s.append(float(logit[a]) + scale * cq[a])
    mx = max(s)
    te = [math.exp(x - mx) for x in s]
    den = sum8(te)
    return {'sum_n': sum_n, 'max_n': max_n, 'vmix': vmix, 'cq': cq, 's': s, 'pi': [x / den for x in te]}


def pick(scores):
    """The arg-max over (score, action) -- the larger action wins a tie, all -inf gives the largest action -- and the gap between
    the best and the second-best score (inf when there is no finite second)."""
    best, act = -INF, -1
    for a, sc in enumerate(scores):
        if sc > best or (sc == best and a > act):
            best, act = sc, a
    second = max([sc for a, sc in enumerate(scores) if a != act], default=-INF)
    return act, (best - second if second > -INF else INF)


def root_scores(N, ev, g, cv_s):
    return [float(g[a]) + ev['s'][a] if N[a] == cv_s else -INF for a in range(len(N))]


def below_scores(N, ev):
    return [ev['pi'][a] - float(N[a]) / (1.0 + float(ev['sum_n'])) for a in range(len(N))]


def gumbel_search_reference(root_prior, root_value, gumbel, reward, probs, value, cv, discount, c_visit=50.0, c_scale=1.0):
    """The search of G games, node by node.  root_prior [G, A] (the stored float64 priors of the roots), root_value [G] (the roots'
    raw network values), gumbel float32 [G, A], reward / value float32 [S, G] and probs float32 [S, G, A] (the network's outputs of
    simulation s, whichever leaf the twin reaches), cv int32 [S].  -> dict of arrays: the trees (N, first_child, value_sum, prior,
    reward, v_hat: [G, 1 + A (S + 1)], top [G]), lo / hi [G], parent / edge / leaf [S, G], action [G], pi float64 [G, A],
    most_visited bool [G, A] and min_gap [G], the smallest gap between the best and the second-best score over a game's decisions."""
    root_prior = np.asarray(root_prior, dtype=np.float64)
    G, A = root_prior.shape
    S = len(cv)
    cap = 1 + A * (S + 1)
    out = {'N': np.zeros((G, cap), np.int32), 'first_child': np.full((G, cap), -1, np.int32), 'value_sum': np.zeros((G, cap)),
           'prior': np.zeros((G, cap)), 'reward': np.zeros((G, cap), np.float32), 'v_hat': np.zeros((G, cap), np.float32),
           'top': np.zeros(G, np.int32), 'lo': np.zeros(G), 'hi': np.zeros(G), 'parent': np.zeros((S, G), np.int32),
           'edge': np.zeros((S, G), np.int32), 'leaf': np.zeros((S, G), np.int32), 'action': np.zeros(G, np.int32),
           'pi': np.zeros((G, A)), 'most_visited': np.zeros((G, A), bool), 'min_gap': np.full(G, INF)}
    for gi in range(G):
        N, fc, vsum = out['N'][gi], out['first_child'][gi], out['value_sum'][gi]
        prior, rew, vhat = out['prior'][gi], out['reward'][gi], out['v_hat'][gi]
        logit = np.full(cap, -INF)

        def add_children(node, top, p):
            fc[node] = top
            prior[top:top + A] = np.asarray(p, dtype=np.float64)
            with np.errstate(divide='ignore'):
                logit[top:top + A] = np.log(prior[top:top + A])

        def node_eval(node, lo, hi):
            c = range(fc[node], fc[node] + A)
            q = [float(rew[s]) + discount * (vsum[s] / float(N[s])) if N[s] > 0 else 0.0 for s in c]
            return [int(N[s]) for s in c], evaluate([int(N[s]) for s in c], [prior[s] for s in c], [logit[s] for s in c], q,
                                                    float(vhat[node]), lo, hi, c_visit, c_scale)

        add_children(0, 1, root_prior[gi])
        vhat[0] = root_value[gi]
        top, lo, hi, gap = 1 + A, INF, -INF, INF
        for s in range(S):
            node, path = 0, [0]
            while fc[node] >= 0:
                n_c, ev = node_eval(node, lo, hi)
                act, d = pick(root_scores(n_c, ev, gumbel[gi], int(cv[s])) if node == 0 else below_scores(n_c, ev))
                gap = min(gap, d)
                out['parent'][s, gi], out['edge'][s, gi] = node, act
                node = fc[node] + act
                path.append(node)
            out['leaf'][s, gi] = node
            rew[node], vhat[node] = reward[s, gi], value[s, gi]
            add_children(node, top, probs[s, gi])
            top += A
            v = float(value[s, gi])
            for slot in reversed(path):
                vsum[slot] = vsum[slot] + v
                N[slot] += 1
                nv = vsum[slot] / float(N[slot])
                hi, lo = max(hi, nv), min(lo, nv)
                v = float(rew[slot]) + discount * v
        n_c, ev = node_eval(0, lo, hi)
        act, d = pick(root_scores(n_c, ev, gumbel[gi], ev['max_n']))
        out['top'][gi], out['lo'][gi], out['hi'][gi] = top, lo, hi
        out['action'][gi], out['pi'][gi], out['min_gap'][gi] = act, ev['pi'], min(gap, d)
        out['most_visited'][gi] = np.asarray(n_c) == ev['max_n']
    return out
