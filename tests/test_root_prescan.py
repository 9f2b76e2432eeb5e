"""The root pre-scan of the resident search (rz_tree.h: RootPre / root_prescan / select_body's hook; rz_delta.h: k_delta_res).

While wave 0 backs a simulation up, wave 1 scores every child of the root except the one the path went through (`r`); the next
selection scores child r alone and takes it against the helper's first maximum.  The rule (CPU): that choice is the first maximum
over all children.  The kernel (GPU): the resident search against the two-launch step (k_trunk_delta + k_tree_step_def, which scans
the root itself) -- the same trees bit for bit, the same delta counters -- with BOTH answers of the consumer occurring (child r wins
again / a sibling wins), and the number of root scans answered from the helper exactly what the host derives:

    a fresh root of k legal moves is expanded by simulation 0, its children are first visited by simulations 1 .. k, every later
    simulation t > k scans the root.  The selection of simulation t finds an answer when the selection of t - 1 was made in the same
    launch (it left the stash) and saw every child visited (t - 1 >= k).  So per game and launch over simulations [s, s + n):
    select_first != 0 -> the selections s .. s + n - 1 are the launch's, answered: t >= max(s + 1, k + 1);
    select_first == 0 -> the selection of s is rz_select_step's, answered: t >= max(s + 2, k + 1).
    No other fall-back exists for a fresh, non-terminal root (the helper's guards -- the parent term's table, the records' byte range
    -- are the scan's own error cases and do not occur here).

Exact ties: a root child that is a terminal win gets W = N, so winners of equal counts tie exactly.  Under the first-maximum rule the
winners are taken in index order, so the child just visited ties with winners of LOWER index only (the one of higher index that tied
it before the visit is now ahead); a tie of child r with a sibling of higher index cannot be produced by terminal wins, and is
covered by the CPU part below."""
import numpy as np
import pytest

STATS = ('delta', 'no_base', 'cells', 'tiles3', 'tiles2')
NONE = 0x7fffffff


# ---------------------------------------------------------------------------------------------------------------- the rule (CPU)

def _wave_first_max(scores, skip=-1):
    """scan_children + wave_first_max: lane l keeps the first strict maximum of its slots l, l + 64, ..., the wave's maximum is
    taken over the lanes, and among the lanes whose best equals it the lowest (slot, lane) wins.  -> (best, index) or (-inf, NONE)."""
    best = np.full(64, -np.inf)
    besti = np.full(64, NONE, dtype=np.int64)
    for r0, sc in enumerate(scores):
        lane = r0 % 64
        if r0 != skip and sc > best[lane]:
            best[lane], besti[lane] = sc, r0
    mx = -np.inf
    for b in best:
        mx = b if b > mx else mx
    hit = [int(i) for b, i in zip(best, besti) if i != NONE and b == mx]
    if not hit:
        return -np.inf, NONE
    i = min(hit, key=lambda i: (i // 64, i % 64))
    return float(scores[i]), i


def _consumer(scores, r):
    """select_body's level 0 with an answer: child r's score against the helper's (best, besti) over the others."""
    best, besti = _wave_first_max(scores, skip=r)
    sr = scores[r]
    cand = sr > -np.inf
    take = cand and (besti == NONE or sr > best or (sr == best and r < besti))
    return r if take else besti


def _python_max(scores):
    """node.py's max(children, key=score): the first maximum (candidates: scores above -inf, as in the lanes' strict `>`)."""
    best, besti = -np.inf, NONE
    for i, sc in enumerate(scores):
        if sc > best:
            best, besti = sc, i
    return besti


def test_child_r_against_masked_argmax_is_the_argmax():
    rs = np.random.RandomState(5)
    cases = 0
    for trial in range(3000):
        k = int(rs.choice([1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 121, 200, 225, 256]))
        kind = trial % 5
        if kind == 0:
            scores = rs.standard_normal(k)
        elif kind == 1:   # few distinct values: ties everywhere, below and above r
            scores = rs.choice([-1.0, 0.0, 0.25, 1.0], k)
        elif kind == 2:   # signed zeros (-0.0 == 0.0: neither is above the other)
            scores = rs.choice([-0.0, 0.0], k)
        elif kind == 3:   # one value everywhere, and children that are no candidates
            scores = np.where(rs.rand(k) < 0.3, -np.inf, 1.5)
        else:             # the maximum twice: once below, once above a random child
            scores = rs.standard_normal(k)
            scores[rs.randint(k)] = scores[rs.randint(k)] = 7.0
        scores = scores.astype(np.float64)
        want = _python_max(scores)
        assert _wave_first_max(scores)[1] == want
        for r in sorted({0, k - 1, int(rs.randint(k)), int(rs.randint(k)), want if want != NONE else 0}):
            assert _consumer(scores, r) == want, (scores, r)
            cases += 1
    assert cases > 6000
    # the tie of child r with a sibling of lower and of higher index, signed zeros included
    for a, b in ((1.0, 1.0), (0.0, -0.0), (-0.0, 0.0)):
        scores = np.array([-3.0, a, -2.0, b, -1.0])
        for r in range(5):
            assert _consumer(scores, r) == 1, (a, b, r)


# ------------------------------------------------------------ the resident search (k_delta_res) against the two-launch step (GPU)

def _net(B, seed, value_scale=None):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(seed)
    net = PolicyValueNet(B)
    if value_scale is not None:   # values away from 0: the value head's last layer, scaled (tanh saturates)
        with torch.no_grad():
            net.val_fc2.weight.mul_(value_scale)
            net.val_fc2.bias.mul_(value_scale)
    return net


def _edge_roots(B, count, seed):
    """Roots whose last move lies on a corner or an edge, and one empty board (tests/test_window_sets.py's construction)."""
    from oracle.gomoku_ref import RefGomoku
    rs = np.random.RandomState(seed)
    S = B * B
    lasts = [0, B - 1, S - B, S - 1, B // 2, (B // 2) * B, (B // 2) * B + B - 1, S - 1 - B // 2]
    envs = [RefGomoku(B, 5)]
    while len(envs) < count:
        last = lasts[len(envs) % len(lasts)]
        others = [int(c) for c in rs.permutation(S) if c != last][:2 * rs.randint(0, 8)]
        e = RefGomoku.from_moves(B, 5, others + [last])
        if not e.game_end_winner()[0]:
            envs.append(e)
    return envs


def _filled_roots(B, count, seed, n_empty, black_cells=(), empty_cells=()):
    """Nearly full boards (tests/test_window_sets.py's _late_roots: cell (y, x) black when (x + 2 y) mod 4 < 2 -- no line anywhere --,
    `n_empty` random cells left free, balanced by freeing a few more), with `black_cells` forced black and `empty_cells` forced free."""
    from oracle.gomoku_ref import RefGomoku
    rs = np.random.RandomState(seed)
    S = B * B
    envs = []
    while len(envs) < count:
        keep = set(black_cells) | set(empty_cells)
        empty = set(empty_cells) | set(int(c) for c in rs.choice([c for c in range(S) if c not in keep], n_empty, replace=False))
        black = [c for c in range(S) if c not in empty and (c in black_cells or (c % B + 2 * (c // B)) % 4 < 2)]
        white = [c for c in range(S) if c not in empty and c not in black]
        while len(black) != len(white):   # (black to move)
            big = black if len(black) > len(white) else white
            free = [c for c in big if c not in keep]
            big.remove(free[rs.randint(len(free))])
        rs.shuffle(black)
        rs.shuffle(white)
        e = RefGomoku.from_moves(B, 5, [m for pair in zip(black, white) for m in pair])
        if not e.game_end_winner()[0]:
            envs.append(e)
    return envs


def _legal(env):
    occ = env.bitboards()[0] | env.bitboards()[1]
    return [c for c in range(env.board_size ** 2) if not (occ >> c) & 1]


def _winning_children(env):
    """Indices (ranks among the legal moves) of the root's children that end the game with a line of the side to move."""
    out = []
    for rank, c in enumerate(_legal(env)):
        e = env.clone()
        e.step(c)
        if e.game_end_winner()[0]:
            out.append(rank)
    return out


def _search(net, envs, chunks, resident, select_first_0=False, c_puct=5.0):
    """Searches from `envs`, `chunks` simulations at a time -> (root visits, whole trees, delta counters, root scans answered from
    the pre-scan, the resident launches as (simulations, select_first)).  select_first_0: every chunk after the first is continued
    as rz_select_step + the resident launch with select_first = 0."""
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine, check, int_to_bits
    B = envs[0].board_size
    sims = sum(chunks)
    evaluator = HipNetEvaluator(net, B, 'cuda:0', max_boards=len(envs))
    evaluator.resident_search = resident
    evaluator.delta_trunk = True
    launches = []
    launch = evaluator.search_resident

    def recorded(eng_, n, first=False):
        launches.append((int(n), bool(first)))
        return launch(eng_, n, first)
    evaluator.search_resident = recorded
    eng = MCTSEngine(B, 5, n_games=len(envs), n_playout=sims, c_puct=c_puct, device='cuda:0', add_noise=True, noise_seed=3)
    assert evaluator.resident_ok(eng) == resident and evaluator.deferred_ok(eng) and evaluator.delta_ok(eng)
    stones = np.array([[int_to_bits(e.bitboards()[0]), int_to_bits(e.bitboards()[1])] for e in envs], dtype=np.uint64)
    eng.set_roots(stones, [e.current_player() for e in envs], [e.last_move for e in envs], reset_trees=True)
    eng.set_noise_keys()
    evaluator.hip.delta_stats(reset=True)
    for i, n in enumerate(chunks):
        if select_first_0 and i > 0:
            m = eng._deferred_begin(evaluator, n)
            assert m == n
            check(eng.lib.rz_select_step(eng.handle, None, eng.stream()), 'rz_select_step')
            evaluator.search_resident(eng, n, False)
            eng._def_pending += n
            eng._def_stream = eng.torch.cuda.current_stream(eng.device)
            eng.flush_deferred()
        else:
            eng.simulate(evaluator, n, use_graph=False)
    st = evaluator.hip.delta_stats()
    visits = eng.root_visits().copy()
    trees = [eng.tree_dump(g) for g in range(len(envs))]
    eng.check()
    eng.close()
    evaluator.hip.close()
    return visits, trees, {k: st[k] for k in STATS}, st['prescans'], launches


def _answers_expected(envs, launches):
    """The derivation of the module's docstring."""
    total = 0
    for env in envs:
        k = len(_legal(env))
        s = 0
        for n, first in launches:
            total += max(0, s + n - max(s + (1 if first else 2), k + 1))
            s += n
    return total


def _same(net, envs, chunks, select_first_0=False, c_puct=5.0):
    """-> (the common root visits, the common trees, root scans answered from the pre-scan)."""
    v_res, t_res, s_res, pre, launches = _search(net, envs, chunks, True, select_first_0, c_puct)
    v_two, t_two, s_two, pre_two, launches_two = _search(net, envs, chunks, False, False, c_puct)
    print('chunks %s: resident launches %s, answered %d (derived %d), counters %s' % (chunks, launches, pre, _answers_expected(envs, launches), s_res))
    assert launches_two == [] and pre_two == 0   # (the two-launch step has no helper)
    assert sum(n for n, _ in launches) == sum(chunks)
    assert s_res['delta'] + s_res['no_base'] == len(envs) * sum(chunks), s_res
    assert s_res == s_two
    assert np.array_equal(v_res, v_two)
    assert t_res == t_two
    assert pre > 0
    assert pre == _answers_expected(envs, launches), (pre, launches)
    return v_res, t_res, pre


@pytest.mark.gpu
@pytest.mark.parametrize('B,sims,chunks', [(11, 400, [150, 130, 120]), (15, 300, [240, 60]), (16, 330, [100, 200, 30])])
def test_benchmark_c_puct_one_launch_and_chunks(B, sims, chunks):
    """c_puct = 5 (the benchmark's): fresh trees, non-terminal roots, more simulations than the root has children; one launch and
    several.  Exploration decides: mostly a sibling of the child just visited wins."""
    envs = _edge_roots(B, 6, seed=B)
    assert all(len(_legal(e)) + 1 < sims for e in envs)
    net = _net(B, 60 + B)
    visits, _, _ = _same(net, envs, [sims])
    assert sum(chunks) == sims
    _same(net, envs, chunks)
    # (in one launch every root scan is answered; had child r won each time, one child would hold all of them: a sibling won too)
    for g, e in enumerate(envs):
        assert visits[g].max() - 1 < sims - 1 - len(_legal(e))


@pytest.mark.gpu
def test_small_c_puct_the_child_just_visited_wins_again():
    """c_puct = 0.05 and values away from 0: exploitation decides.  Some root child holds more than half of the simulations made
    after the breadth-first phase, so it was chosen twice in a row (pigeonhole) -- child r against the helper's maximum, won by r --
    and the trees are the two-launch step's, which shows the same majority on its own.  (Seed and scale were chosen with the
    two-launch step alone: of seeds 71 .. 73 and scales 2 .. 16 only seed 73 gives its most visited child a majority -- 58 .. 68 % of
    the simulations behind the breadth-first phase at scale 2, all of them from scale 4 on; the others spread them evenly.)"""
    B, sims = 11, 400
    envs = _edge_roots(B, 6, seed=21)
    net = _net(B, 73, value_scale=2.0)
    v_two = _search(net, envs, [sims], False, False, 0.05)[0]
    majority = [g for g, e in enumerate(envs) if v_two[g].max() - 1 > (sims - 1 - len(_legal(e))) / 2]
    assert majority, 'the yardstick itself shows no child with a majority: another seed / scale'
    visits, _, _ = _same(net, envs, [sims], c_puct=0.05)
    assert [g for g, e in enumerate(envs) if visits[g].max() - 1 > (sims - 1 - len(_legal(e))) / 2] == majority
    _same(net, envs, [130, 150, 120], c_puct=0.05)


@pytest.mark.gpu
@pytest.mark.parametrize('n_empty,lo,hi,sims', [(40, 16, 64, 200), (9, 2, 16, 120)])
def test_late_roots_with_few_children(n_empty, lo, hi, sims):
    """Fewer than 64 / fewer than 16 children (two stages of the arg-max less in the helper's scan, empty lanes, one lane slot)."""
    B = 11
    envs = _filled_roots(B, 6, seed=n_empty, n_empty=n_empty)
    assert all(lo <= len(_legal(e)) < hi for e in envs), [len(_legal(e)) for e in envs]
    net = _net(B, 80 + n_empty)
    _same(net, envs, [sims])
    _same(net, envs, [sims // 2, sims - sims // 2])


@pytest.mark.gpu
def test_exact_ties_between_winning_children():
    """Roots whose side to move has four winning cells (two open fours), among other free cells of lower and of higher index: the
    winners' scores tie exactly whenever their counts are equal (W = N), the just-visited winner against winners of lower index."""
    B, sims = 11, 160
    fours = [2 * B + x for x in (1, 2, 3, 4)] + [7 * B + x for x in (6, 7, 8, 9)]
    ends = [2 * B + 0, 2 * B + 5, 7 * B + 5, 7 * B + 10]
    envs = _filled_roots(B, 4, seed=2, n_empty=8, black_cells=fours, empty_cells=ends)
    winners = [_winning_children(e) for e in envs]
    for e, w in zip(envs, winners):
        k = len(_legal(e))
        assert e.current_player() == 0 and k < 64 and len(w) >= 4 and w[0] > 0 and w[-1] < k - 1, (k, w)
    net = _net(B, 90)
    _, trees, _ = _same(net, envs, [sims])
    for e, w, tree in zip(envs, winners, trees):
        legal = _legal(e)
        counts = [tree[(legal[r], )][0] for r in w]
        assert all(tree[(legal[r], )] == (n, float(n)) for r, n in zip(w, counts))   # (every visit a win: W = N exactly)
        assert max(counts) - min(counts) <= 1 and counts == sorted(counts, reverse=True) and min(counts) >= 3, counts
    _same(net, envs, [70, 90])


@pytest.mark.gpu
def test_select_first_zero_continuations():
    """Launches whose first leaf comes from rz_select_step (select_first = 0): the first selection made inside each has no stash and
    scans the root itself, the rest are answered."""
    B = 15
    envs = _edge_roots(B, 6, seed=7)
    _same(_net(B, 50), envs, [240, 40, 30], select_first_0=True)
