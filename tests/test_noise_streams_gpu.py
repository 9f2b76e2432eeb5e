"""The device noise streams sample by sample against their host restatements (tests/device_streams.py).

AlphaZero: the stored prior of every child of every expanded node is 0.75 p + 0.25 eta with eta the Dirichlet(0.3) draw of counter
`ctr` of the game's key, the child keyed by its ACTION.  p comes from a twin engine without noise (under the reference's selection
rule no prior is ever read, so the two trees are the same node for node) or, under PUCT with the synthetic evaluator, is 1 / k.  The
counter of an expansion is its rank by prior-block offset (PB) within its game: blocks and counters are handed out together.  All
three hand-copied places of the draw are reached: the in-step expansion (rz_tree.h), deferred_priors_body (the flush of the deferred
route, of the resident search, and the kept-rows flush of the device move step) and the level-synchronous multi-simulation step.

MuZero whole moves: with the noise at weight 1 the stored root priors ARE the draw (float64, normalised in float64), and the action
of every record is the restatement's draw from the record's own visit counts.

Tolerance, sample by sample: |eta_dev - eta_ref| <= T_rel * eta_ref + R.  R = the read-back's resolution: 4 ulp(prior) / 0.25 for
the float32 AlphaZero priors, 0 for MuZero's float64 ones.  T_rel = 4 x the largest relative difference between the restatement's own
float32 and float64 evaluations on the very keys of the test (4: hardware transcendentals of ~1 ulp against numpy's float32); it must
stay below 1e-2, where a wrong key or counter moves eta by eta itself.  A node is compared only when every child's acceptance margin
in the float64 restatement is at least 1e-4 (else float32 may take the other branch of the rejection test): at most 10 % of a case's
nodes may be left out, and those still sum to 1 with no negative eta.

MEASURED, MI355X (profiles/noise_streams/agreement.txt, written by profiles/noise_streams/measure.py): T_rel computed on the CPU /
the device's worst relative difference (AlphaZero: beyond R)
  in-step, 9 x 9              2.18e-05 / 3.0e-08      in-step, 15 x 15            2.92e-05 / 1.2e-07
  in-step, Connect4 6 x 7     1.16e-05 / 0            in-step, Connect4 12 x 16   1.17e-05 / 0
  in-step, 3 x 3 (1, 2 moves) 5.17e-06 / 0            in-step PUCT, 9 x 9         2.16e-05 / 8.0e-08
  in-step PUCT, Connect4      1.16e-05 / 0            multi-sim K = 5, 9 x 9      2.18e-05 / 3.0e-08
  multi-sim K = 5, Connect4   1.16e-05 / 0            deferred flush (both)       3.24e-05 / 3.3e-08
  kept-rows flush             7.64e-06 / 0            two searches, default keys  2.81e-05 / 6.6e-08
  two searches, explicit keys 2.03e-05 / 1.1e-07
  MuZero alpha 0.25           1.05e-05 / 4.6e-06      MuZero alpha 1.0            3.68e-05 / 4.1e-06
  MuZero alpha 1.5            1.42e-05 / 1.5e-06      MuZero alpha 0.1            2.11e-05 / 9.0e-06
  action draws: 5 x 13824 records, none differs, none skipped
Left out for a small margin: 1.4 - 1.5 % of the nodes at 81 children, 4.0 % at 225, below 0.1 % elsewhere.

What the comparison found while it was written: gamma03's literal c = 0.33903103f is 2.2e-6 below 1 / sqrt(9 d) = 0.33903178.  A
restatement with the exact c was off by up to 4e-5 on draws with a small v = 1 + c x, which nodes of 7 and 16 children showed and
nodes of 81 hid behind R; with the literal the device agrees as above.  The distribution is unaffected (the host test's KS).

Mutations of one line each, new tests / the two old noise tests (test_dirichlet_noise_on_priors, ..._noise_is_dirichlet):
  child keyed `+ lane` in deferred_priors_body       3 fail (both deferred flushes, the kept-rows flush) / pass
  pend_ctr[rec] = 0                                  the same 3 fail / pass
  boost exponent 1.0f / 0.33f                        14 fail (every AlphaZero test) / pass
  MuZero per-action key `a` for `a + 1`              4 fail (the root noise at every alpha) / pass
  `cum >= target` for `cum > target`                 none fails / pass: the two differ only where uniform * total equals a partial
                                                     sum exactly, one draw in 2^53 -- no honest input tells them apart
"""
import numpy as np
import pytest

import device_streams as ds

AZ_GAMES = 64
MARGIN = 1e-4
EXCLUDED_CAP = 0.10
# cells: the children of an empty Gomoku root (None: Connect4 -- its trees are deep, its nodes small)
AZ_CASES = {
    'gomoku_9x9': dict(game='gomoku', shape=9, n_row=5, sims=60, seed=11, cells=81),
    'gomoku_15x15': dict(game='gomoku', shape=15, n_row=5, sims=60, seed=12, cells=225),
    'connect4_6x7': dict(game='connect4', shape=(6, 7), n_row=4, sims=60, seed=13, cells=None),
    'connect4_12x16': dict(game='connect4', shape=(12, 16), n_row=4, sims=40, seed=14, cells=None),
}
MZ_ENVS, MZ_SEED = 512, 9
MZ_ALPHAS = (0.25, 1.0, 1.5, 0.1)
MEASURED = {}   # route -> (T_rel, observed): what profiles/noise_streams/measure.py writes down


# ---------------------------------------------------------------------------------------------------------------------- AlphaZero
def _engine(case, **kw):
    from rlzero_amd.engine import MCTSEngine
    kw.setdefault('n_games', AZ_GAMES)
    kw.setdefault('n_playout', case['sims'])
    return MCTSEngine(case['shape'], case['n_row'], device='cuda:0', game=case['game'], noise_seed=case['seed'], **kw)


def _set_roots(eng, envs):
    from rlzero_amd.engine import int_to_bits
    stones = np.array([[int_to_bits(e.bitboards()[0]), int_to_bits(e.bitboards()[1])] for e in envs], dtype=np.uint64)
    eng.set_roots(stones, [e.current_player() for e in envs], [e.last_move for e in envs], reset_trees=True)


def _expanded(eng, g, occ0, arena=None):
    """The expanded nodes of game g -> {action path: (slot, legal actions, PB, child priors float32)}, walking the arena from the root."""
    ar = eng.arena(g) if arena is None else arena
    out, stack = {}, [((), 0, occ0)]
    while stack:
        path, s, occ = stack.pop()
        k = int(ar['K'][s])
        if k == 0:
            continue
        legal = eng.legal_actions(occ)
        assert len(legal) == k, (g, path, k, len(legal))
        pb = int(ar['PB'][s])
        out[path] = (s, np.array(legal, dtype=np.int64), pb, ar['PRI'][pb:pb + k].copy())
        fc = int(ar['FC'][s])
        for r in range(int(ar['NV'][s])):
            stack.append((path + (legal[r], ), fc + r, occ | (1 << eng.cell_of_action(occ, legal[r]))))
    return out


def _root_occ(eng):
    from rlzero_amd.engine import bits_to_int
    stones, _, _ = eng.get_roots()
    return [bits_to_int(stones[g, 0]) | bits_to_int(stones[g, 1]) for g in range(eng.n_games)]


def _by_block(nodes):
    """Paths in the order their prior blocks were handed out."""
    return sorted(nodes, key=lambda p: nodes[p][2])


class _Samples(object):
    """(key, counter, legal actions, stored priors, p) of the expansions of a case; ``check`` compares them all in one pass."""

    def __init__(self):
        self.keys, self.ctrs, self.legal, self.pri, self.p, self.tag = [], [], [], [], [], []

    def add(self, key, ctr, legal, pri, p, tag):
        assert pri.dtype == np.float32 and p.dtype == np.float32 and len(pri) == len(p) == len(legal)
        self.keys.append(np.uint64(key))
        self.ctrs.append(int(ctr))
        self.legal.append(legal)
        self.pri.append(pri)
        self.p.append(p)
        self.tag.append(tag)

    def add_game(self, key, nodes, plain=None, ctr_of=None, tag=None, p_of_k=None):
        """Every expanded node of one game: counters by block order unless ``ctr_of`` {path: counter} says otherwise; p from the
        twin's nodes ``plain`` (same paths, same blocks) or the uniform prior of k children ``p_of_k[k]``."""
        order = _by_block(nodes)
        if plain is not None:
            assert sorted(plain) == sorted(nodes) and all(plain[q][2] == nodes[q][2] for q in nodes), tag
        for rank, path in enumerate(order):
            _, legal, _, pri = nodes[path]
            p = plain[path][3] if plain is not None else np.full(len(legal), p_of_k[len(legal)], dtype=np.float32)
            self.add(key, rank if ctr_of is None else ctr_of[path], legal, pri, p, (tag, path))

    def check(self, route):
        assert len(self.keys) > 0
        keys, ctrs = np.array(self.keys, dtype=np.uint64), np.array(self.ctrs, dtype=np.int64)
        ref, margins = ds.alphazero_eta_many(keys, ctrs, self.legal)
        ref32, _ = ds.alphazero_eta_many(keys, ctrs, self.legal, dtype=np.float32)
        keep = np.array([float(m.min()) >= MARGIN for m in margins])
        share = 1.0 - keep.mean()
        spread = max(ds.relative_spread(ref[i], ref32[i]) for i in np.nonzero(keep)[0])
        t_rel = 4.0 * spread
        worst, worst_at = 0.0, None
        bad = []
        for i, (eta_ref, pri, p) in enumerate(zip(ref, self.pri, self.p)):
            pri64 = pri.astype(np.float64)
            eta = (pri64 - 0.75 * p.astype(np.float64)) / 0.25
            res = 4.0 * np.spacing(pri).astype(np.float64) / 0.25
            assert abs(eta.sum() - 1.0) <= res.sum() + 1e-6 and (eta >= -res).all(), (route, self.tag[i], eta.sum())
            if len(pri) == 1:   # one legal move: eta = 1 exactly, the prior 1 within an ulp
                assert eta_ref[0] == 1.0 and abs(pri64[0] - 1.0) <= np.spacing(np.float32(1.0)), (route, self.tag[i], pri64)
            if not keep[i]:
                continue
            diff = np.abs(eta - eta_ref)
            excess = float(np.max(np.maximum(diff - res, 0.0) / eta_ref))
            if excess > worst:
                worst, worst_at = excess, self.tag[i]
            if (diff > t_rel * eta_ref + res).any():
                j = int(np.argmax(diff - t_rel * eta_ref - res))   # (the child furthest out: its action, eta_ref, eta_dev, R)
                bad.append((self.tag[i], self.ctrs[i], int(self.legal[i][j]), float(eta_ref[j]), float(eta[j]), float(res[j])))
                print('  outside: %s counter %d\n    ref %s\n    dev %s\n    R   %s' % (self.tag[i], self.ctrs[i], eta_ref.tolist(), eta.tolist(), res.tolist()))
        print('%s: %d nodes, %.2f %% left out (margin < %g), T_rel = %.3e, device worst relative excess over R = %.3e at %s'
              % (route, len(keep), 100 * share, MARGIN, t_rel, worst, worst_at))
        MEASURED[route] = (t_rel, worst, len(keep), share)
        assert t_rel < 1e-2, (route, t_rel)
        assert share <= EXCLUDED_CAP, (route, share)
        assert not bad, (route, len(bad), bad[:6])


def _search(case, evaluator, roots=None, keys=None, **kw):
    eng = _engine(case, **kw)
    if roots is None:
        eng.reset_games()
    else:
        _set_roots(eng, roots)
    if keys is not None:
        eng.set_noise_keys(keys)
    eng.simulate(evaluator, case['sims'])
    eng.check()
    return eng


def _default_keys(case, n=AZ_GAMES):
    return ds.default_noise_key(case['seed'], np.arange(n))


def _twin_case(case, evaluator, route, roots=None, n_games=AZ_GAMES, **kw):
    """A noisy engine and its twin without noise under the reference's rule -> every expansion of every game compared."""
    noisy = _search(case, evaluator, roots, add_noise=True, n_games=n_games, **kw)
    plain = _search(case, evaluator, roots, add_noise=False, n_games=n_games, **kw)
    occ = _root_occ(noisy)
    keys = _default_keys(case, n_games)
    samples, deepest = _Samples(), 0
    for g in range(n_games):
        a, b = noisy.arena(g), plain.arena(g)
        assert all(np.array_equal(a[f], b[f]) for f in ('N', 'W', 'FC', 'NV', 'K', 'PB')), (route, g)   # the same tree node for node
        nodes = _expanded(noisy, g, occ[g], a)
        samples.add_game(keys[g], nodes, _expanded(plain, g, occ[g], b), tag=g)
        deepest = max(deepest, max(len(q) for q in nodes))
    noisy.close()
    plain.close()
    samples.check(route)
    return deepest


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(AZ_CASES))
def test_in_step_expansion_noise_is_the_restatement(name):
    """rz_tree.h's copy: SyntheticEvaluator('v0'), every child of every expanded node of 64 games.  15 x 15: actions over four mask
    words, 225 children; Connect4: the action is the column, not the cell; 12 x 16: a rectangular board."""
    from rlzero_amd.engine import SyntheticEvaluator
    case = AZ_CASES[name]
    deepest = _twin_case(case, SyntheticEvaluator('v0'), 'in-step ' + name)
    assert deepest >= (1 if case['cells'] else 2)


@pytest.mark.gpu
def test_nodes_of_one_and_two_legal_moves():
    """3 x 3 from positions with 1 and with 2 legal moves: with one child eta = 1 exactly and the prior 1 within an ulp (asserted for
    every such node by the comparison itself); the children of the two-move roots are one-move nodes with counters of their own."""
    from oracle.gomoku_ref import RefGomoku
    from rlzero_amd.engine import SyntheticEvaluator
    case = dict(game='gomoku', shape=3, n_row=3, sims=6, seed=15, cells=None)
    moves = [0, 1, 2, 4, 3, 5, 7, 6]
    roots = [RefGomoku.from_moves(3, 3, moves if g % 2 else moves[:-1]) for g in range(AZ_GAMES)]
    assert not any(e.game_end_winner()[0] for e in roots)
    assert sorted(len(e.leagel_actions()) for e in roots[:2]) == [1, 2]
    _twin_case(case, SyntheticEvaluator('v0'), 'in-step 3x3 with 1 and 2 legal moves', roots=roots)


def _uniform_priors(case, evaluator, depth):
    """{k: the synthetic evaluator's prior of a node of k children}: the roots' expansions of an engine WITHOUT noise whose game j
    starts from j scattered stones.  The evaluator hands the tree step logf(1 / k) and the tree step stores expf of it: that float32
    is 1 / k only within a few ulp (an ulp of the logarithm, 4.4 at k = 81, is 8 ulp of the prior), more than the read-back
    resolution R allows -- so p is read from the device, bit for bit, as on the other routes."""
    from oracle.gomoku_ref import RefGomoku
    n = depth if case['game'] == 'gomoku' else 1
    eng = _engine(case, n_games=n, n_playout=1, add_noise=False, score_mode='puct')
    if case['game'] == 'gomoku':   # stones two cells apart, colours alternating: no line
        _set_roots(eng, [RefGomoku.from_moves(case['shape'], case['n_row'], [2 * i for i in range(j)]) for j in range(n)])
    else:
        eng.reset_games()
    eng.simulate(evaluator, 1)
    eng.check()
    pri = eng.root_priors()
    out = {}
    for j in range(n):
        vals = pri[j][pri[j] > 0]
        assert len(set(vals.tolist())) == 1
        out[len(vals)] = vals[0]
        assert abs(float(vals[0]) * len(vals) - 1.0) < 1e-5
    eng.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['gomoku_9x9', 'connect4_6x7'])
def test_puct_expansion_noise_is_the_restatement(name):
    """Under PUCT the selection reads the noisy priors, so the twin's tree is another one: p is the synthetic evaluator's uniform
    prior of a node of k children, read from an engine without noise (_uniform_priors)."""
    from rlzero_amd.engine import SyntheticEvaluator
    case = AZ_CASES[name]
    eng = _search(case, SyntheticEvaluator('v0'), add_noise=True, score_mode='puct')
    occ, keys, samples = _root_occ(eng), _default_keys(case), _Samples()
    nodes = [_expanded(eng, g, occ[g]) for g in range(AZ_GAMES)]
    eng.close()
    p_of_k = _uniform_priors(case, SyntheticEvaluator('v0'), 16)
    for g in range(AZ_GAMES):
        samples.add_game(keys[g], nodes[g], tag=g, p_of_k=p_of_k)
    samples.check('in-step puct ' + name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['gomoku_9x9', 'connect4_6x7'])
def test_multi_sim_step_noise_is_the_restatement(name):
    """rz_engine.hip's level-synchronous step at K = 5: several nodes take their counters (ctr0 + the expansions of the slots before
    them) in one step."""
    from rlzero_amd.engine import SyntheticEvaluator
    _twin_case(AZ_CASES[name], SyntheticEvaluator('v0'), 'multi-sim K=5 ' + name, sims_in_flight=5)


def _hip_evaluator(board, resident):
    import torch
    from rlzero_amd.engine import HipNetEvaluator
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(board)
    ev = HipNetEvaluator(PolicyValueNet(board).to('cuda:0'), board, 'cuda:0', max_boards=AZ_GAMES)
    ev.deferred_priors = True
    ev.resident_search = resident
    return ev


@pytest.mark.gpu
@pytest.mark.parametrize('resident', [False, True], ids=['deferred_steps', 'resident_search'])
def test_deferred_flush_noise_is_the_restatement(resident):
    """deferred_priors_body behind a HipNet on 9 x 9: p is the net's softmax (the twin's stored priors), so the mix is tested on
    non-uniform priors, each record mixed with the counter its step stored (pend_ctr)."""
    from rlzero_amd.engine import MCTSEngine
    case = dict(AZ_CASES['gomoku_9x9'], sims=50, seed=16)
    ev = _hip_evaluator(9, resident)
    probe = MCTSEngine(9, 5, n_games=AZ_GAMES, n_playout=50, device='cuda:0', add_noise=True)
    r = ev.route(probe)
    probe.close()
    assert r.deferred and bool(r.resident) == resident, r
    _twin_case(case, ev, 'deferred flush, %s' % ('resident search' if resident else 'step by step'))
    ev.hip.check_flags()
    ev.hip.close()


@pytest.mark.gpu
def test_kept_rows_flush_noise_is_the_restatement():
    """The device move step on 11 x 11 (48 simulations: the root, then its children in order): only the priors a move keeps are
    written, by the kept-rows flush.  After move 1 the root is the drawn child, expanded with counter 1 + its rank; after move 2 it
    is a child expanded in the SECOND search, whose counters go on from 48 -- the key is the game's (rz_play.h noise_key), p the
    twin's root priors."""
    import torch
    from move_step_twin import SEED, Twin
    from rlzero_amd.engine import bits_to_int
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    G, sims, cells = 8, 48, 121
    torch.manual_seed(4)
    net = PolicyValueNet(11).to('cuda:0')
    noisy, plain = Twin(True, net, G, sims, add_noise=True), Twin(True, net, G, sims, add_noise=False)
    salt = np.uint64(0x6E6F697365000000)
    samples, played = _Samples(), [[] for _ in range(G)]
    for ply in range(2):
        rows = noisy.move(), plain.move()
        assert np.array_equal(rows[0], rows[1])   # the same moves: the draw reads visit counts
        for gid in range(G):
            mv = int(rows[0][gid, 3])
            assert mv >= 0
            legal_before = [c for c in range(cells) if c not in played[gid]]
            ctr = ply * sims + (1 if ply == 0 else 0) + legal_before.index(mv)
            played[gid].append(mv)
            got = {}
            for twin in (noisy, plain):
                slot = int(twin.slot_of[gid])
                stones, _, _ = twin.eng.get_roots()
                occ = bits_to_int(stones[slot, 0]) | bits_to_int(stones[slot, 1])
                assert occ == sum(1 << c for c in played[gid])
                ar = twin.eng.arena(slot)
                k, pb = int(ar['K'][0]), int(ar['PB'][0])
                assert k == cells - len(played[gid])
                got[twin] = ar['PRI'][pb:pb + k].copy()
            key = ds.mix64(ds.mix64(np.uint64(SEED) ^ salt) ^ np.uint64(gid))
            samples.add(key, ctr, np.array([c for c in range(cells) if c not in played[gid]]), got[noisy], got[plain], (gid, ply))
    noisy.close()
    plain.close()
    samples.check('kept-rows flush (device move step)')


@pytest.mark.gpu
@pytest.mark.parametrize('explicit', [False, True], ids=['default_keys', 'set_noise_keys'])
def test_counters_go_on_after_update_with_move(explicit):
    """6 x 6, two searches with update_with_move between them: the kept subtree's priors are still the draws of the counters its
    nodes had (found again by their paths), and the second search's expansions -- the blocks behind the copied ones, in block order --
    take the counters after the first search's last: never a restart.  With explicit keys (rz_set_noise_keys) the same holds; the
    mapping stays exact because the copied blocks lie in front of every new one."""
    from rlzero_amd.engine import SyntheticEvaluator
    case = dict(game='gomoku', shape=6, n_row=4, sims=50, seed=17, cells=36)
    keys = _default_keys(case)
    if explicit:
        keys = np.arange(AZ_GAMES, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(5)
    got = {}
    for noise in (True, False):
        eng = _search(case, SyntheticEvaluator('vlin'), add_noise=noise, keys=keys if explicit and noise else None)
        occ = _root_occ(eng)
        first = [_expanded(eng, g, occ[g]) for g in range(AZ_GAMES)]
        moves = eng.root_visits().argmax(axis=1).astype(np.int32)
        eng.advance_and_step(moves, moves)
        kept_floats = [len(eng.arena(g)['PRI']) for g in range(AZ_GAMES)]
        eng.simulate(SyntheticEvaluator('vlin'), case['sims'])
        eng.check()
        occ2 = _root_occ(eng)
        second = [_expanded(eng, g, occ2[g]) for g in range(AZ_GAMES)]
        got[noise] = (first, moves, kept_floats, second)
        eng.close()
    (first, moves, kept_floats, second), (p_first, p_moves, _, p_second) = got[True], got[False]
    assert np.array_equal(moves, p_moves)
    samples, carried, fresh = _Samples(), 0, 0
    for g in range(AZ_GAMES):
        samples.add_game(keys[g], first[g], p_first[g], tag=(g, 'first search'))
        ctr_first = {path: c for c, path in enumerate(_by_block(first[g]))}
        m, ctr_of, new = int(moves[g]), {}, []
        for path in _by_block(second[g]):
            if second[g][path][2] < kept_floats[g]:   # a copied block: the node was expanded in the first search, below the move
                ctr_of[path] = ctr_first[(m, ) + path]
                carried += 1
            else:
                new.append(path)
        for c, path in enumerate(new):
            assert (m, ) + path not in ctr_first
            ctr_of[path] = len(first[g]) + c
        fresh += len(new)
        samples.add_game(keys[g], second[g], p_second[g], ctr_of=ctr_of, tag=(g, 'second search'))
    assert carried >= AZ_GAMES and fresh >= AZ_GAMES * (case['sims'] - 2)
    samples.check('two searches around update_with_move, %s keys' % ('explicit' if explicit else 'default'))


# ---------------------------------------------------------------------------------------------------------------------- MuZero
_MZ_RUNS = {}
MZ_LAUNCHES, MZ_MOVES_PER_LAUNCH = 9, 3


def _mz_run(alpha, temperature, n_sims=2):
    """27 whole moves of 512 CartPole environments in launches of three, noise at weight 1 -> the root priors behind every launch,
    every record, and (episode, steps) before every move, rebuilt from the records' done flags and checked against the device's."""
    key = (alpha, temperature, n_sims)
    if key not in _MZ_RUNS:
        import torch
        from rlzero_amd.muzero import CartPoleBatch, MuZeroNet, MuZeroSelfPlay
        torch.manual_seed(6)
        net = MuZeroNet().to('cuda:0').eval()   # (untrained: a weak player, episodes of a dozen moves)
        env = CartPoleBatch(MZ_ENVS, 'cuda:0', seed=22)
        sp = MuZeroSelfPlay(net, env, n_sims=n_sims, seed=MZ_SEED, root_dirichlet_alpha=alpha, root_exploration_fraction=1.0,
                            temperature=temperature, fused_moves=True, moves_per_launch=MZ_MOVES_PER_LAUNCH)
        priors = []
        for _ in range(MZ_LAUNCHES):
            sp.collect(MZ_MOVES_PER_LAUNCH)
            priors.append(sp.tree.root_children('prior').cpu().numpy().copy())
        n_moves = MZ_LAUNCHES * MZ_MOVES_PER_LAUNCH
        ring, _ = sp.device_history()
        rec = ring[:, :n_moves].copy()
        steps, episode = np.zeros((n_moves + 1, MZ_ENVS), np.int64), np.zeros((n_moves + 1, MZ_ENVS), np.int64)
        for t in range(n_moves):
            done = rec[:, t, 9] != 0.0
            steps[t + 1] = np.where(done, 0, steps[t] + 1)
            episode[t + 1] = episode[t] + done
        assert np.array_equal(steps[-1], env.steps.cpu().numpy()) and np.array_equal(episode[-1], env.episode)
        sp.tree.check()
        sp.close()
        _MZ_RUNS[key] = dict(priors=priors, rec=rec, steps=steps, episode=episode, n_sims=n_sims)
    return _MZ_RUNS[key]


MZ_PAIRS = [(0.25, 1.0), (1.0, 0.5), (1.5, 0.25), (0.1, 0.0)]   # (alpha, temperature): every alpha, every temperature, four runs
assert tuple(a for a, _ in MZ_PAIRS) == MZ_ALPHAS


@pytest.mark.gpu
@pytest.mark.parametrize('alpha,temperature', MZ_PAIRS)
def test_whole_move_root_noise_is_the_restatement(alpha, temperature):
    """root_exploration_fraction = 1: tree.root_children('prior') behind a launch of three moves is muzero_eta of (episode, steps)
    before the launch's last move, per environment, for two actions (whole moves are CartPole's: the ABI takes no other count).
    Nine launches: the keys cross launch, move and episode boundaries -- environments in their second or later episode are counted."""
    run = _mz_run(alpha, temperature)
    g = np.arange(MZ_ENVS)
    worst, t_rel_max, left_out, later_episodes, total = 0.0, 0.0, 0, 0, 0
    for launch, pri in enumerate(run['priors']):
        t = MZ_MOVES_PER_LAUNCH * launch + MZ_MOVES_PER_LAUNCH - 1
        ep, st = run['episode'][t], run['steps'][t]
        ref, margin, _ = ds.muzero_eta(MZ_SEED, g, ep, st, 2, alpha)
        ref32, _, _ = ds.muzero_eta(MZ_SEED, g, ep, st, 2, alpha, dtype=np.float32)
        assert pri.dtype == np.float64 and pri.shape == ref.shape
        assert np.max(np.abs(pri.sum(axis=1) - 1.0)) <= 1e-12 and (pri >= 0).all()
        keep = margin.min(axis=1) >= MARGIN
        t_rel = 4.0 * ds.relative_spread(ref[keep], ref32[keep])
        rel = np.abs(pri[keep] - ref[keep]) / ref[keep]
        worst, t_rel_max = max(worst, float(rel.max())), max(t_rel_max, t_rel)
        left_out += int((~keep).sum())
        total += MZ_ENVS
        later_episodes += int((ep[keep] > 0).sum())
        assert t_rel < 1e-2
        assert (rel <= t_rel).all(), (alpha, launch, float(rel.max()), t_rel, np.nonzero(keep)[0][np.argmax(rel.max(axis=1))])
    route = 'MuZero whole moves, alpha %g' % alpha
    print('%s: %d moves, %d left out, %d in a later episode, T_rel up to %.3e, device worst relative difference %.3e'
          % (route, total, left_out, later_episodes, t_rel_max, worst))
    MEASURED[route] = (t_rel_max, worst, total, left_out / total)
    assert left_out <= EXCLUDED_CAP * total
    assert later_episodes >= MZ_ENVS   # (episode boundaries were crossed: the key's episode and the restart of steps are looked at)


@pytest.mark.gpu
@pytest.mark.parametrize('alpha,temperature,n_sims', [p + (2, ) for p in MZ_PAIRS] + [(0.25, 0.5, 16)])
def test_whole_move_action_draws_are_the_restatement(alpha, temperature, n_sims):
    """Every record of the runs above (and of one at 16 simulations): the action is muzero_action of the record's visit counts and
    the (episode, steps) before its move -- exactly, at T = 1, 0.5, 0.25 and T -> 0 (arg-max, the lowest index on ties: with two
    simulations a third of the records tie).  At T != 1 the device's pow may differ from numpy's in the last bit: a record is skipped
    only if the restatement's |cum - target| is below 1e-9 x total; the count is stated and expected to be zero."""
    run = _mz_run(alpha, temperature, n_sims)
    rec, n_moves = run['rec'], run['rec'].shape[1]
    g = np.broadcast_to(np.arange(MZ_ENVS)[:, None], (MZ_ENVS, n_moves))
    visits = rec[:, :, 6:8].astype(np.int64)
    assert (visits.sum(axis=2) == n_sims).all()
    inv_t = 1.0 / temperature if temperature > 0 else 0.0
    want, gap = ds.muzero_action(MZ_SEED, g, run['episode'][:-1].T, run['steps'][:-1].T, visits, inv_t)
    got = rec[:, :, 4].astype(np.int64)
    skip = (gap < 1e-9) & (inv_t != 1.0)
    ties = int((visits[:, :, 0] == visits[:, :, 1]).sum())
    route = 'MuZero action draw, T = %g, %d simulations' % (temperature, n_sims)
    print('%s: %d records, %d skipped (|cum - target| < 1e-9 total), %d ties, %d in a later episode, action 1 drawn %d times'
          % (route, got.size, int(skip.sum()), ties, int((run['episode'][:-1] > 0).sum()), int(got.sum())))
    MEASURED[route] = (0.0, float(np.mean(want[~skip] != got[~skip])), got.size, float(skip.mean()))
    assert np.array_equal(want[~skip], got[~skip]), np.argwhere((want != got) & ~skip)[:8]
    assert skip.sum() <= 1e-6 * skip.size + 1
    assert (run['episode'][:-1] > 0).sum() >= MZ_ENVS and 0 < got.sum() < got.size
    if temperature == 0.0:
        assert ties > 0 and (got[visits[:, :, 0] == visits[:, :, 1]] == 0).all()


