"""The tree arena's documented limits restated on the oracle's tree (helpers of test_arena_limits.py; no GPU needed).

rz_create sizes a game's arena from n_playout and pool_factor (A actions per position):

    qcap = int((pool_factor + 1) * n_playout) + 8      expanded nodes = prior blocks
    pcap = qcap * A                                     prior floats
    cap  = qcap * A + 2  (puct)  |  qcap * 16 + 2 A + 64  (uct_ref)      record slots

and rz_advance_roots carries a kept subtree only when, summed over its expanded nodes in breadth-first order (k legal moves, a
child block of `block_cap` records each),

    sum k        <= pcap - (n_playout + 1) * A
    1 + sum cap  <= cap - (n_playout + 1) * 8 - 2 A
    count        <= qcap - n_playout - 1

Everything here is computed from the oracle's RefNode tree and the capacities rz_get_stats reports -- never from a device tree."""
import numpy as np

from oracle.gomoku_ref import RefGomoku

FIRST_CAP = 4   # child records reserved at a node's first visited child (rz_tree.h: kFirstCap)


def qcap_of(pool_factor, n_playout):
    return int((pool_factor + 1.0) * n_playout) + 8


def block_limit(pool_factor, n_playout):
    """L: the largest number of expanded nodes a carried subtree may have."""
    return qcap_of(pool_factor, n_playout) + 0 - n_playout - 1


def pool_factor_for(limit, n_playout):
    """A pool_factor whose block limit is exactly `limit` (the middle of the interval that floors to it)."""
    pf = (limit + 1 - 8 + 0.5) / float(n_playout)
    assert pf > 0.0 and block_limit(pf, n_playout) == limit, (limit, n_playout, pf)
    return pf


def block_cap(nv, k, score_mode):
    """Records of the child block of a node with k legal moves of which nv were visited: all k under puct; under uct_ref the
    growth rule 4, 8, ... doubling, capped at k (no block before the first visit)."""
    if score_mode == 'puct':
        return k
    if nv == 0:
        return 0
    cap = min(k, FIRST_CAP)
    while cap < nv:
        cap = min(2 * cap, k)
    return cap


def subtree_need(node, score_mode):
    """-> (expanded nodes, prior floats, record slots incl. the root's) of the subtree under `node`, walked breadth-first over
    expanded nodes the way advance_body's queue does."""
    count = floats = 0
    slots = 1
    queue = [node] if node.kids else []
    head = 0
    while head < len(queue):
        x = queue[head]
        head += 1
        k = len(x.kids)
        visited = [kid for kid in x.kids if kid.n > 0]
        # (uct_ref visits children in ascending order: the visited ones are a prefix; puct keeps a record of every child)
        if score_mode != 'puct':
            assert all(kid.n > 0 for kid in x.kids[:len(visited)])
        count += 1
        floats += k
        slots += block_cap(len(visited), k, score_mode)
        queue.extend(kid for kid in (x.kids if score_mode == 'puct' else visited) if kid.kids)
    return count, floats, slots


def predict_drop(root, move, score_mode, n_playout, n_actions, arena_slots, prior_floats):
    """The decision of advance_body for update_with_move(move) on the oracle's `root`: True when the kept subtree is dropped.
    arena_slots / prior_floats: rz_stats (the engine's capacities); qcap = prior_floats / A."""
    if move not in root.acts:
        return False
    kid = root.child(move)
    if kid.n == 0 and score_mode != 'puct':
        return False   # a never-visited child is a fresh node in the reference too
    count, floats, slots = subtree_need(kid, score_mode)
    qcap = prior_floats // n_actions
    return (floats > prior_floats - (n_playout + 1) * n_actions or
            slots > arena_slots - (n_playout + 1) * 8 - 2 * n_actions or
            count > qcap - n_playout - 1)


def capacities(pool_factor, n_playout, n_actions, score_mode):
    """(arena_slots, prior_floats) as rz_create sizes them -- for choosing seeds on the CPU; the tests assert that rz_get_stats
    reports the same numbers before they rely on a prediction made with them."""
    qcap = qcap_of(pool_factor, n_playout)
    cap = qcap * n_actions + 2 if score_mode == 'puct' else qcap * 16 + 2 * n_actions + 64
    return cap, qcap * n_actions


def late_root(B, n_row, n_empty, seed):
    """A nearly full board without a line of three (cell (y, x) is black when (x + 2 y) mod 4 < 2: runs of two at most in every
    direction) with `n_empty` free cells and the stones balanced."""
    rs = np.random.RandomState(seed)
    S = B * B
    black = [c for c in range(S) if (c % B + 2 * (c // B)) % 4 < 2]
    white = [c for c in range(S) if (c % B + 2 * (c // B)) % 4 >= 2]
    rs.shuffle(black)
    rs.shuffle(white)
    nb, nw = (S - n_empty + 1) // 2, (S - n_empty) // 2
    assert nb <= len(black) and nw <= len(white)
    b, w = black[:nb], white[:nw]
    env = RefGomoku.from_moves(B, n_row, [m for pair in zip(b, w) for m in pair] + b[nw:])
    assert not env.game_end_winner()[0] and len(env.leagel_actions()) == n_empty
    return env


def pick_move(root, rule):
    """The move of a game by rule, not by chance: 'most' / 'least' = the most / least visited VISITED child (the first of equals),
    'unvisited' = a never-visited child when there is one (else the least visited)."""
    visited = [(kid.n, i) for i, kid in enumerate(root.kids) if kid.n > 0]
    if rule == 'unvisited':
        for a, kid in zip(root.acts, root.kids):
            if kid.n == 0:
                return a
        rule = 'least'
    if rule == 'most':
        n, i = max(visited, key=lambda t: (t[0], -t[1]))
    else:
        n, i = min(visited, key=lambda t: (t[0], t[1]))
    return root.acts[i]


def hex_tree(d):
    return {k: (n, float(w).hex()) for k, (n, w) in d.items()}


FRESH = {(): (0, float(0.0).hex())}
