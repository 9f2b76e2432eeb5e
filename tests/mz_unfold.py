"""Read a finished MuZero search back out of its tree (plain numpy, no GPU): test infrastructure.

The kernels leave every game's complete tree in ``MuZeroTree.nodes()``: N, first_child, value_sum, prior, reward per slot.
That holds everything a per-simulation trace would have said:

* order ......... slots are handed out in expansion order, so the expanded non-root slots sorted by ``first_child`` are the
                  simulations in order;
* parent, action  the children of slot s sit at ``first_child[s] + a``;
* probabilities . the children's ``prior`` are the network's float32 probabilities (widened);
* reward ........ stored in the node (float32);
* value ......... the backup identity  value_sum[s] = v[s] + sum over children (N_c * reward_c + discount * value_sum_c)
                  (no v term for the root: the root is expanded by the initial inference, not by a simulation).

``unfold`` REFUSES (raises ``TreeRefused``) any tree the kernels cannot have written; it never guesses.  The value it returns
is the float32 nearest to the recovered double, and that double must lie within 1/8 of a float32 ulp of it: the backup sums a
few dozen doubles, so an honest tree recovers the network's float32 to ~1e-13 relative, and a corrupted ``value_sum`` does not
decode to something plausible.
"""
import collections
import math

import numpy as np

Expansion = collections.namedtuple('Expansion', 'slot parent action path reward probs value')


class TreeRefused(ValueError):
    """The node records are not a tree the search kernels can have written."""


def _refuse(msg, *args):
    raise TreeRefused(msg % args)


def unfold(nodes, top, n_actions, discount):
    """One game's node records (structured array [slots]: N, first_child, value_sum, prior, reward) and its ``top``
    -> (expansions, root_prior): the list of ``Expansion`` in simulation order -- slot, parent slot, action, path of actions
    from the root, reward (np.float32), probs (np.float32 [A], the children's priors), value (np.float32) -- and the root's
    prior vector (float64 [A], as stored: after the noise)."""
    A, top = int(n_actions), int(top)
    discount = float(discount)
    if A < 1 or top < 1 + A or top > len(nodes) or (top - 1) % A:
        _refuse('top %d is not 1 + k * %d within %d slots', top, A, len(nodes))
    N = [int(x) for x in nodes['N'][:top]]
    fc = [int(x) for x in nodes['first_child'][:top]]
    vs = [float(x) for x in nodes['value_sum'][:top]]
    prior = [float(x) for x in nodes['prior'][:top]]
    rew32 = nodes['reward'][:top].astype(np.float32)
    rew = [float(x) for x in rew32]

    # the child blocks: handed out one after the other, one per expansion (the root's first)
    expanded = [s for s in range(top) if fc[s] >= 0]
    want = list(range(1, top, A))
    if sorted(fc[s] for s in expanded) != want:
        _refuse('first_child values %r are not 1, 1 + A, ... below top %d', sorted(fc[s] for s in expanded)[:8], top)
    if fc[0] != 1:
        _refuse('the root owns block %d, not the first', fc[0])
    parent, action = {}, {}
    for s in expanded:
        for a in range(A):
            parent[fc[s] + a] = s
            action[fc[s] + a] = a
    order = sorted((s for s in expanded if s != 0), key=lambda s: fc[s])
    if len(order) != N[0]:
        _refuse('%d expansions, root N = %d', len(order), N[0])
    for s in order:   # a block is handed out when its owner is expanded: after the owner's own slot was handed out
        if fc[s] <= s:
            _refuse('slot %d owns the earlier block %d', s, fc[s])

    # visit counts, and what an untouched node looks like
    for s in range(top):
        if fc[s] >= 0:
            kids = sum(N[fc[s] + a] for a in range(A))
            if N[s] != kids + (0 if s == 0 else 1):
                _refuse('N[%d] = %d, its children sum to %d', s, N[s], kids)
        elif N[s] != 0 or vs[s] != 0.0 or rew[s] != 0.0:
            _refuse('slot %d is not expanded but carries N %d, value_sum %r, reward %r', s, N[s], vs[s], rew[s])
        if not math.isfinite(vs[s]) or not math.isfinite(rew[s]) or not math.isfinite(prior[s]):
            _refuse('slot %d holds a non-finite number', s)

    def below(s):   # what the backups through the children of s added to value_sum[s]
        terms = []
        for a in range(A):
            c = fc[s] + a
            terms.append(N[c] * rew[c])
            terms.append(discount * vs[c])
        return terms

    resid = math.fsum([vs[0]] + [-t for t in below(0)])
    if abs(resid) > 1e-9 * max(1.0, abs(vs[0])):
        _refuse('root value_sum %r differs from its children\'s backups by %r', vs[0], resid)

    out = []
    paths = {0: ()}
    for s in order:
        p = parent[s]
        if p not in paths:
            _refuse('slot %d was expanded before its parent %d', s, p)
        paths[s] = paths[p] + (action[s], )
        v = math.fsum([vs[s]] + [-t for t in below(s)])
        v32 = np.float32(v)
        if not np.isfinite(v32) or abs(v - float(v32)) > float(np.spacing(np.abs(v32))) / 8.0:
            _refuse('slot %d: recovered value %r is not a float32 (nearest %r)', s, v, float(v32))
        probs = np.array([prior[fc[s] + a] for a in range(A)], dtype=np.float64)
        probs32 = probs.astype(np.float32)
        if not np.array_equal(probs32.astype(np.float64), probs):
            _refuse('slot %d: the children\'s priors %r are not float32 values', s, probs.tolist())
        out.append(Expansion(s, p, action[s], paths[s], rew32[s], probs32, v32))
    return out, np.array([prior[1 + a] for a in range(A)], dtype=np.float64)


def slot_of_path(nodes, path):
    """The slot the actions ``path`` lead to from the root."""
    s = 0
    for a in path:
        s = int(nodes['first_child'][s]) + a
    return s
