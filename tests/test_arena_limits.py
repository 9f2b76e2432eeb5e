"""The tree arena's limits: dropped subtrees, full arenas, containment -- every comparison against the CPU oracle
(oracle/mcts_ref.py; the documented limits restated on its tree in arena_rules.py).

A. The carry limit of rz_advance_roots / k_play_apply (advance_body) is the documented rule: per game and move the device carried
   exactly the oracle's kept subtree or holds a fresh root, as the three inequalities restated in arena_rules.predict_drop say.
B. A full arena is flagged and contained: bit-equal to the oracle up to the last chunk before the first refused expansion; then
   flagged, the bump pointers inside the arena, every record offset inside it, the small and inactive games between the
   overflowing ones (their arenas are adjacent in one allocation) still the oracle's, and a reset recovers.
C. A legitimate near-depth-first search (c_puct = 0) at the default pool_factor never fills its arena.

Which test reaches which branch (flag: implementation -> test):

  REUSE_DROPPED, advance_body in k_advance behind ...
      k_select + k_expand_backup ........ test_carry_rule[*-plain], test_block_limit_boundary
      k_tree_step ....................... test_carry_rule[*-fused], test_slot_limit_boundary, test_deep_search_fits
      k_tree_step_def + deferred flush .. test_carry_rule_net_routes[two_launch-*]
      k_trunk_split<RES> (6 x 6) ........ test_carry_rule_net_routes[resident-6]
      k_delta_res (15 x 15) ............. test_carry_rule_net_routes[resident-15]
  REUSE_DROPPED, advance_body in k_play_apply ... test_carry_rule_device_moves
  BLOCKS_FULL, expand_backup_body (rz_tree.h) in ...
      k_expand_backup ................... test_full_arena[plain-*]
      k_tree_step ....................... test_full_arena[fused-*]
      k_tree_step_def, eager / graph .... test_full_arena_net_routes[two_launch-6 / two_launch_graph-6]
      k_trunk_split<RES> ................ test_full_arena_net_routes[resident-6]
      k_delta_res ....................... test_full_arena_net_routes[resident-15]
      k_tree_step_vl (sequential) ....... test_full_arena_in_flight[6] / [15]
  BLOCKS_FULL, k_tree_step_ml's bump allocation (the `fits` guard) ... test_full_arena_in_flight[6] / [15]
  ARENA_FULL, select_body's `fresh = 2` stop (uct_ref) ... test_arena_full_uct_ref (k_tree_step), test_full_arena_in_flight[15]
      (k_tree_step_vl)
  ARENA_FULL, k_tree_step_ml phase C ... test_full_arena_in_flight[15]
  ARENA_FULL under puct (expand_backup_body's and k_tree_step_ml's dense branch): UNREACHABLE through the ABI.  Dense arenas have
      cap = qcap * A + 2 record slots and pcap = qcap * A prior floats; every expansion takes k of both and the root one more
      slot, so top = ptop + 1 always (fresh tree and carried subtree alike) and top + k > cap means ptop + k > pcap + 1: the
      BLOCKS_FULL test (ptop + k > pcap) of the same branch comes first.

The prior-float limit of the carry rule (sum k > (qcap - n_playout - 1) * A) cannot bind before the block limit either: k <= A
for every node.  It is restated in the prediction all the same.

What notices an undone guard: the block inequality of advance_body off by one -- test_block_limit_boundary and test_carry_rule; the
slot inequality -- test_slot_limit_boundary; select_body's `fresh = 2` stop -- test_arena_full_uct_ref (the top would pass 730, and
the arena's 898 slots); the `fits` guard of k_tree_step_ml -- test_full_arena_in_flight (prior blocks past the game's ptop, the
bump pointers past the arena).

No oracle exists for several simulations in flight (virtual loss): there the neighbours are compared with the same engine built
with an ample pool_factor, and the two implementations with each other."""
import functools

import numpy as np
import pytest

import arena_rules as ar
from oracle import evaluators as ev
from oracle.gomoku_ref import RefGomoku
from oracle.mcts_ref import RefSearch, inverse_cdf_choice, tree_dump

pytestmark = pytest.mark.gpu

ARENA_FULL, BLOCKS_FULL, REUSE_DROPPED = 1, 2, 32   # include/rlzero_hip.h: RZ_FLAG_*


# ------------------------------------------------------------------------------------------------ helpers
def _oracle_fn(kind, score_mode):
    """v0 / vlin for the oracle; under puct with the priors the device gives a node without a policy: 1.0f / k in f32."""
    base = {'v0': ev.v0, 'vlin': ev.vlin}[kind]
    if score_mode != 'puct':
        return base

    def fn(env):
        pri, v = base(env)
        p = float(np.float32(1.0) / np.float32(len(pri))) if pri else 0.0
        return [(a, p) for a, _ in pri], v
    return fn


def _device_eval(kind, score_mode):
    """The synthetic evaluator; under puct without its log-priors (exp(log(1 / k)) is not 1 / k to the bit): the expansion then
    writes 1.0f / k, which the oracle's evaluator above restates exactly."""
    from rlzero_amd.engine import SyntheticEvaluator
    if score_mode != 'puct':
        return SyntheticEvaluator(kind)

    class Uniform(SyntheticEvaluator):
        def __call__(self, eng):
            SyntheticEvaluator.__call__(self, eng)
            return None, eng.value
    return Uniform(kind)


def _set_roots(eng, envs, mask=None):
    from rlzero_amd.engine import int_to_bits
    stones = np.array([[int_to_bits(e.bitboards()[0]), int_to_bits(e.bitboards()[1])] for e in envs], dtype=np.uint64)
    eng.set_roots(stones, [e.current_player() for e in envs], [e.last_move for e in envs], mask=mask, reset_trees=True)


def _tree(eng, g):
    return ar.hex_tree(eng.tree_dump(g))


def _ref_tree(ref):
    return ar.hex_tree(tree_dump(ref.root))


def _search(route, eng, evaluator, n):
    if route == 'plain':   # k_select + k_expand_backup, one pair per simulation
        for _ in range(n):
            eng.sim_step(evaluator)
    elif route == 'graph':
        eng.simulate(evaluator, n, use_graph=True, sims_per_graph=8)
    else:                  # k_tree_step / the evaluator's own route
        eng.simulate(evaluator, n)


def _clear(eng):
    from rlzero_amd._hip import check
    check(eng.lib.rz_clear_errors(eng.handle), 'rz_clear_errors')


def _capacities_are(eng, pool_factor, n_playout, n_actions, score_mode):
    st = eng.stats()
    assert (st.arena_slots, st.prior_floats) == ar.capacities(pool_factor, n_playout, n_actions, score_mode)
    return st


def _offsets_inside(eng, g, st):
    """Every offset held by a record of game g's tree lies inside that game's arena, and no two child blocks overlap.  Walked
    from the root: the unused tail of a child block is not initialised."""
    a = eng.arena(g)
    assert 1 <= a['top'] <= st.arena_slots and len(a['PRI']) <= st.prior_floats
    stack, blocks, seen = [0], [], 0
    while stack:
        slot = stack.pop()
        seen += 1
        assert seen <= a['top']
        k, nv, fc, pb = int(a['K'][slot]), int(a['NV'][slot]), int(a['FC'][slot]), int(a['PB'][slot])
        if k == 0:
            continue
        assert 0 <= nv <= k and 0 <= pb and pb + k <= len(a['PRI']), (g, slot, k, nv, fc, pb)
        if nv > 0:
            assert 1 <= fc and fc + nv <= a['top'], (g, slot, k, nv, fc)
            blocks.append((fc, fc + nv))
            stack.extend(range(fc, fc + nv))
    blocks.sort()
    assert all(x[1] <= y[0] for x, y in zip(blocks, blocks[1:])), g


# ------------------------------------------------------------------------------------------------ A: the carry rule
N_MOVES = 6


def _carry_starts(B, n_row):
    """(start, rule of its moves): an open board, the centre opening (a never-visited child is kept), late roots with few empty
    cells (deep trees: most- and least-visited children) and a near-terminal start."""
    from test_production_routes import _near_wins
    c = B * (B // 2) + B // 2
    return [(RefGomoku(B, n_row), 'most'), (RefGomoku.from_moves(B, n_row, [c]), 'unvisited'),
            (ar.late_root(B, n_row, 8, 1), 'most'), (ar.late_root(B, n_row, 9, 2), 'most'), (ar.late_root(B, n_row, 10, 3), 'least'),
            (ar.late_root(B, n_row, 11, 5), 'most'), (ar.late_root(B, n_row, 12, 6), 'most'), (ar.late_root(B, n_row, 9, 4), 'least'),
            (_near_wins(B, n_row)[0], 'least')]   # (one move short of a line: the most-visited move would end the game at once)


def _plan_game(start, rule, fn, sims, c_puct, score_mode, n_actions, caps, n_moves, after=None):
    """One game on the oracle, following the PREDICTED drops: per move the tree after the search, the move, whether the kept
    subtree is dropped, (expanded nodes of the kept subtree), the tree after update_with_move; then one more search."""
    env, ref, out = start.clone(), RefSearch(fn, sims, c_puct, score_mode=score_mode), []
    for m in range(n_moves + 1):
        if env.game_end_winner()[0]:
            break
        ref.simulate(env, 1.0)
        searched = _ref_tree(ref)
        if after is not None:
            after(ref)
        if m == n_moves:
            out.append(dict(searched=searched, move=None))
            break
        move = ar.pick_move(ref.root, rule)
        need = ar.subtree_need(ref.root.child(move), score_mode)
        drop = ar.predict_drop(ref.root, move, score_mode, sims, n_actions, *caps)
        ref.update_with_move(-1 if drop else move)   # the documented deviation: a dropped subtree is a fresh root
        env.step(move)
        pri = [(a, kid.p) for a, kid in zip(ref.root.acts, ref.root.kids)]
        out.append(dict(searched=searched, move=move, drop=drop, need=need, advanced=_ref_tree(ref), priors=pri))
    return out


CARRY = {   # id: (score_mode, c_puct, pool_factor) -- 6 x 6, four in a row, 64 simulations per move, vlin
    'uct5': ('uct_ref', 5.0, 0.02), 'uct05': ('uct_ref', 0.5, 0.1), 'puct5': ('puct', 5.0, 0.02), 'puct05': ('puct', 0.5, 0.3)}
CARRY_B, CARRY_N, CARRY_SIMS = 6, 4, 64


@functools.lru_cache(maxsize=None)
def _carry_plan(case):
    score_mode, c_puct, pf = CARRY[case]
    caps = ar.capacities(pf, CARRY_SIMS, CARRY_B * CARRY_B, score_mode)
    plan = [_plan_game(s, rule, _oracle_fn('vlin', score_mode), CARRY_SIMS, c_puct, score_mode, CARRY_B * CARRY_B, caps, N_MOVES)
            for s, rule in _carry_starts(CARRY_B, CARRY_N)]
    # on the oracle alone: both outcomes occur, each in a quarter of the (game, move) pairs at least
    pairs = [mv for game in plan for mv in game if mv['move'] is not None]
    dropped = sum(1 for mv in pairs if mv['drop'])
    kept_big = sum(1 for mv in pairs if not mv['drop'] and mv['need'][0] > 1)
    assert 4 * dropped >= len(pairs) and 4 * kept_big >= len(pairs), (case, len(pairs), dropped, kept_big)
    return plan


def _play_plan(eng, plan, starts, search, score_mode, n_actions):
    """The batch on the device along the oracle's plan: the trees after every search and after every advance, the drop count, the
    flags.  -> predicted drops."""
    G = len(plan)
    _set_roots(eng, starts)
    drops = 0
    for m in range(max(len(game) for game in plan)):
        active = np.array([1 if len(plan[g]) > m else 0 for g in range(G)], dtype=np.uint8)
        eng.set_active(active)
        search()
        for g in range(G):
            if active[g]:
                assert _tree(eng, g) == plan[g][m]['searched'], 'game %d, search %d' % (g, m)
        moves = np.array([plan[g][m]['move'] if active[g] and plan[g][m]['move'] is not None else -2 for g in range(G)], dtype=np.int32)
        if (moves < 0).all():
            break
        eng.advance(moves)   # tree reuse before the boards change; the read-outs below name children by the NEW board's legal moves
        eng.step(np.where(moves >= 0, moves, -1).astype(np.int32))
        drops += sum(1 for g in range(G) if moves[g] >= 0 and plan[g][m]['drop'])
        pri = eng.root_priors() if score_mode == 'puct' else None
        for g in range(G):
            if moves[g] < 0:
                continue
            mv = plan[g][m]
            # the oracle's kept subtree, or -- exactly where the restated rule says so -- a single fresh root
            assert _tree(eng, g) == mv['advanced'], 'game %d, advance %d (predicted %s)' % (g, m, 'dropped' if mv['drop'] else 'kept')
            if mv['drop']:
                assert mv['advanced'] == ar.FRESH
            elif score_mode == 'puct' and mv['priors']:   # the carried root's prior block, f32 bits
                got = np.array([pri[g][a] for a, _ in mv['priors']], dtype=np.float32)
                want = np.array([p for _, p in mv['priors']], dtype=np.float32)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), 'priors of game %d, advance %d' % (g, m)
        st = eng.check()   # (a dropped subtree is no error: does not raise)
        assert st.reuse_dropped == drops and st.error_flags == (REUSE_DROPPED if drops else 0) and st.first_bad_game == -1
        assert eng.poll_errors() == drops
    assert drops > 0
    _clear(eng)
    st = eng.stats()
    assert st.reuse_dropped == 0 and st.error_flags == 0 and eng.poll_errors() == 0
    return drops


@pytest.mark.parametrize('route', ['plain', 'fused'])
@pytest.mark.parametrize('case', sorted(CARRY))
def test_carry_rule(case, route):
    """9 games, 6 moves with tree reuse, moves by rule: after every advance the device holds the oracle's kept subtree or -- exactly
    where the three inequalities restated from the oracle's tree say so -- a fresh root; the count, the flag, check(), poll_errors()
    and rz_clear_errors agree; the games that kept their subtree in the same batch are the oracle's throughout."""
    from rlzero_amd.engine import MCTSEngine
    score_mode, c_puct, pf = CARRY[case]
    plan = _carry_plan(case)
    starts = [s for s, _ in _carry_starts(CARRY_B, CARRY_N)]
    eng = MCTSEngine(CARRY_B, CARRY_N, n_games=len(starts), n_playout=CARRY_SIMS, c_puct=c_puct, pool_factor=pf, score_mode=score_mode,
                     device='cuda:0')
    _capacities_are(eng, pf, CARRY_SIMS, CARRY_B * CARRY_B, score_mode)
    evaluator = _device_eval('vlin', score_mode)
    _play_plan(eng, plan, starts, lambda: _search(route, eng, evaluator, CARRY_SIMS), score_mode, CARRY_B * CARRY_B)
    eng.close()


@pytest.mark.parametrize('score_mode', ['uct_ref', 'puct'])
def test_block_limit_boundary(score_mode):
    """One targeted game: c = the expanded nodes of the subtree its first move keeps (the oracle's count).  Two engines whose
    pool_factor puts the block limit L = qcap - n_playout - 1 at c and at c - 1: the first carries the subtree, the second drops it
    (the rule: dropped when c > L).  An open board beside it keeps its one-node subtree in both."""
    from rlzero_amd.engine import MCTSEngine
    B, n_row, sims, c_puct = 6, 4, 64, 5.0
    A = B * B
    start, other = ar.late_root(B, n_row, 8, 1), RefGomoku(B, n_row)
    fn = _oracle_fn('vlin', score_mode)
    ref = RefSearch(fn, sims, c_puct, score_mode=score_mode)
    ref.simulate(start, 1.0)
    move = ar.pick_move(ref.root, 'most')
    c = ar.subtree_need(ref.root.child(move), score_mode)[0]
    assert c >= 8   # (the smallest limit a pool_factor can give is 7)
    ref2 = RefSearch(fn, sims, c_puct, score_mode=score_mode)
    ref2.simulate(other, 1.0)
    move2 = ar.pick_move(ref2.root, 'most')
    searched, searched2 = _ref_tree(ref), _ref_tree(ref2)
    ref.update_with_move(move)
    ref2.update_with_move(move2)
    for limit in (c, c - 1):
        pf = ar.pool_factor_for(limit, sims)
        caps = ar.capacities(pf, sims, A, score_mode)
        ref_root = RefSearch(fn, sims, c_puct, score_mode=score_mode)
        ref_root.simulate(start, 1.0)
        drop = ar.predict_drop(ref_root.root, move, score_mode, sims, A, *caps)
        assert drop == (limit == c - 1)   # the restated rule: kept at L = c, dropped at L = c - 1
        eng = MCTSEngine(B, n_row, n_games=2, n_playout=sims, c_puct=c_puct, pool_factor=pf, score_mode=score_mode, device='cuda:0')
        st = _capacities_are(eng, pf, sims, A, score_mode)
        assert st.prior_floats // A - sims - 1 == limit
        _set_roots(eng, [start, other])
        evaluator = _device_eval('vlin', score_mode)
        _search('plain', eng, evaluator, sims)
        assert _tree(eng, 0) == searched and _tree(eng, 1) == searched2
        eng.advance(np.array([move, move2], dtype=np.int32))
        eng.step(np.array([move, move2], dtype=np.int32))
        assert _tree(eng, 0) == (ar.FRESH if drop else _ref_tree(ref)), 'L = %d, c = %d' % (limit, c)
        assert _tree(eng, 1) == _ref_tree(ref2)
        st = eng.check()
        assert st.reuse_dropped == (1 if drop else 0) and st.error_flags == (REUSE_DROPPED if drop else 0)
        eng.close()


def test_slot_limit_boundary():
    """The record-slot inequality, where it binds before the block limit: dense (puct) arenas of a board with A < 8 actions -- 2 x 2,
    two in a row (A = 4).  There cap - (n_playout + 1) * 8 - 2 A = 4 (qcap - n_playout - 1) - 6 - 4 (n_playout + 1) falls with
    n_playout while the block limit stays at 7 or more and the prior limit at 4 (qcap - n_playout - 1).  The kept subtree of the first
    move needs s slots (the oracle's count): an engine whose slot limit is >= s carries it, the next smaller arena (the limit moves
    in steps of A) drops it -- with the block and prior inequalities far from binding in both."""
    from rlzero_amd.engine import MCTSEngine
    B, n_row, sims, c_puct, score_mode, A = 2, 2, 16, 5.0, 'puct', 4
    start = RefGomoku(B, n_row)
    fn = _oracle_fn('vlin', score_mode)
    ref = RefSearch(fn, sims, c_puct, score_mode=score_mode)
    ref.simulate(start, 1.0)
    move = ar.pick_move(ref.root, 'most')
    count, floats, slots = ar.subtree_need(ref.root.child(move), score_mode)
    assert count >= 2
    searched = _ref_tree(ref)
    ref.update_with_move(move)
    seen = set()
    for units in range(1, 3 * sims):   # int(pool_factor * n_playout) = units
        pf = (units + 0.5) / sims
        cap, pcap = ar.capacities(pf, sims, A, score_mode)
        slot_limit, qcap = cap - (sims + 1) * 8 - 2 * A, pcap // A
        if not (slots - A <= slot_limit < slots + A):
            continue
        drop = slots > slot_limit
        # (the other two inequalities do not bind here: the slot limit alone decides)
        assert count <= qcap - sims - 1 and floats <= pcap - (sims + 1) * A
        ref_root = RefSearch(fn, sims, c_puct, score_mode=score_mode)
        ref_root.simulate(start, 1.0)
        assert ar.predict_drop(ref_root.root, move, score_mode, sims, A, cap, pcap) == drop
        eng = MCTSEngine(B, n_row, n_games=2, n_playout=sims, c_puct=c_puct, pool_factor=pf, score_mode=score_mode, device='cuda:0')
        _capacities_are(eng, pf, sims, A, score_mode)
        _set_roots(eng, [start, start])
        eng.simulate(_device_eval('vlin', score_mode), sims)
        assert _tree(eng, 0) == searched
        eng.advance(np.array([move, -2], dtype=np.int32))
        eng.step(np.array([move, -1], dtype=np.int32))
        assert _tree(eng, 0) == (ar.FRESH if drop else _ref_tree(ref)), 'slots %d, limit %d' % (slots, slot_limit)
        assert _tree(eng, 1) == searched
        assert eng.check().reuse_dropped == (1 if drop else 0)
        eng.close()
        seen.add(drop)
    assert seen == {True, False}


NET_CARRY = [('two_launch', 6, 4, 48, 0.02), ('resident', 6, 4, 48, 0.02), ('two_launch', 15, 5, 32, 0.02), ('resident', 15, 5, 32, 0.02)]


@pytest.mark.parametrize('route,B,n_row,sims,pf', NET_CARRY, ids=['%s-%d' % c[:2] for c in NET_CARRY])
def test_carry_rule_net_routes(route, B, n_row, sims, pf):
    """The carry rule behind the net routes: advance follows a deferred prior flush (k_tree_step_def) or the resident search
    (k_trunk_split<RES> on 6 x 6, k_delta_res on 15 x 15).  The oracle is fed the device's own leaf values (test_production_routes'
    probe).  Late roots, so that the trees go deep enough for both outcomes; three moves."""
    import torch
    from test_production_routes import _Probe
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(7)
    net = PolicyValueNet(B)
    probe = _Probe(net, 'gomoku', B, n_row)
    A = B * B
    caps = ar.capacities(pf, sims, A, 'uct_ref')
    starts = [(ar.late_root(B, n_row, 6, 1), 'most'), (RefGomoku(B, n_row), 'most'), (ar.late_root(B, n_row, 7, 2), 'most'),
              (ar.late_root(B, n_row, 8, 3), 'least'), (ar.late_root(B, n_row, 7, 4), 'most'), (ar.late_root(B, n_row, 9, 5), 'most'),
              (ar.late_root(B, n_row, 6, 6), 'least'), (ar.late_root(B, n_row, 8, 7), 'most')]
    plan = [_plan_game(s, rule, probe, sims, 5.0, 'uct_ref', A, caps, 3) for s, rule in starts]
    pairs = [mv for game in plan for mv in game if mv['move'] is not None]
    assert any(mv['drop'] for mv in pairs) and any(not mv['drop'] and mv['need'][0] > 1 for mv in pairs)
    evaluator = HipNetEvaluator(net, B, 'cuda:0', max_boards=len(starts))
    evaluator.resident_search = route == 'resident'
    eng = MCTSEngine(B, n_row, n_games=len(starts), n_playout=sims, pool_factor=pf, device='cuda:0')
    _capacities_are(eng, pf, sims, A, 'uct_ref')
    assert evaluator.deferred_ok(eng) and evaluator.resident_ok(eng) == (route == 'resident')
    if route == 'resident':
        assert evaluator.resident_delta_ok(eng) == (B == 15)
    _play_plan(eng, plan, [s for s, _ in starts], lambda: eng.simulate(evaluator, sims), 'uct_ref', A)
    evaluator.hip.check_flags()
    eng.close()
    evaluator.hip.close()
    probe.close()


def test_carry_rule_device_moves():
    """k_play_apply calls the same advance_body from the move step on the device: self-play games under puct with a small c_puct (deep
    trees) and a small pool_factor.  The device-driven games are the host-driven ones on another engine (same moves, pi bits, winners,
    same number of dropped subtrees), and both are the oracle's games played with the PREDICTED drops."""
    from rlzero_amd.engine import MCTSEngine
    from rlzero_amd.selfplay import BatchedSelfPlay, move_uniform
    B, n_row, sims, c_puct, pf, seed, ids = 6, 4, 32, 0.5, 0.1, 5, list(range(10))
    A = B * B
    caps = ar.capacities(pf, sims, A, 'puct')
    fn = _oracle_fn('vlin', 'puct')
    want, drops = {}, 0
    for gid in ids:
        choice = inverse_cdf_choice(move_uniform(seed, np.full(64, gid), np.arange(64)))
        env, ref, moves = RefGomoku(B, n_row), RefSearch(fn, sims, c_puct, score_mode='puct'), []
        while not env.game_end_winner()[0]:
            acts, probs = ref.simulate(env, 1.0)
            move = choice(acts, probs)
            drop = ar.predict_drop(ref.root, move, 'puct', sims, A, *caps)
            drops += drop
            ref.update_with_move(-1 if drop else move)
            env.step(move)
            moves.append(int(move))
        want[gid] = (env.game_end_winner()[1], moves)
    assert drops >= len(ids)   # (on the oracle alone: the rule is exercised, about once a game at least)
    runs = []
    for device_moves in (True, False):
        eng = MCTSEngine(B, n_row, n_games=4, n_playout=sims, c_puct=c_puct, pool_factor=pf, score_mode='puct', device='cuda:0')
        _capacities_are(eng, pf, sims, A, 'puct')
        sp = BatchedSelfPlay(eng, _device_eval('vlin', 'puct'), temperature=1.0, seed=seed)
        trajs = sp.run_device(ids) if device_moves else sp.run(ids)
        st = eng.check()
        assert st.error_flags == REUSE_DROPPED and st.reuse_dropped == drops, (device_moves, st.reuse_dropped, drops)
        for t in trajs:
            assert (t.winner, t.moves) == want[t.game_id], (device_moves, t.game_id)
        runs.append(trajs)
        eng.close()
    for x, y in zip(*runs):
        assert np.array_equal(np.asarray(x.pis).view(np.uint64), np.asarray(y.pis).view(np.uint64)), x.game_id


# ------------------------------------------------------------------------------------------------ B: a full arena
FULL_SIMS, FULL_PF, CHUNK, FULL_TOTAL = 16, 0.01, 8, 80


def _full_batch(B, n_row):
    """Even slots: open positions, whose trees grow with every simulation; odd slots: late roots of 3 empty cells at most (a game
    tree of 16 nodes: they can never fill anything); the last slot inactive."""
    c = B * (B // 2) + B // 2
    opens = [RefGomoku(B, n_row), RefGomoku.from_moves(B, n_row, [c]), RefGomoku.from_moves(B, n_row, [c, c + 1]),
             RefGomoku.from_moves(B, n_row, [0, c, B - 1])]
    lates = [ar.late_root(B, n_row, 3, 1), ar.late_root(B, n_row, 2, 2), ar.late_root(B, n_row, 3, 3), ar.late_root(B, n_row, 3, 4)]
    envs = [e for pair in zip(opens, lates) for e in pair]
    active = np.ones(len(envs), dtype=np.uint8)
    active[-1] = 0
    return envs, active


def _first_refused(ref, env, qcap, pcap, upto):
    """Run the oracle simulation by simulation -> the first simulation (1-based) whose expansion the arena refuses: expanded nodes
    beyond qcap or prior floats beyond pcap (None: none up to `upto`).  The oracle itself goes on unbounded."""
    first = None

    def usage(node):
        count, floats, stack = 0, 0, [node]
        while stack:
            x = stack.pop()
            if x.kids:
                count += 1
                floats += len(x.kids)
                stack.extend(x.kids)
        return count, floats
    for s in range(1, upto + 1):
        ref.playout(env.clone())
        count, floats = usage(ref.root)
        if first is None and (count > qcap or floats > pcap):
            first = s
    return first


def _full_arena_case(B, n_row, fn, make_engine, search, close=None):
    """The asserts of part B for one implementation.  fn: the oracle's evaluator; make_engine() -> (engine, its evaluator);
    search(eng, evaluator, n)."""
    from rlzero_amd._hip import HipError
    A = B * B
    envs, active = _full_batch(B, n_row)
    G = len(envs)
    cap, pcap = ar.capacities(FULL_PF, FULL_SIMS, A, 'uct_ref')
    qcap = pcap // A
    # the oracle: every game up to FULL_TOTAL simulations, the trees at every chunk boundary; the first refused expansion
    refused, trees = [], []
    for g, env in enumerate(envs):
        ref, per = RefSearch(fn, FULL_SIMS, 5), {}
        first = None
        for done in range(CHUNK, FULL_TOTAL + 1, CHUNK):
            f = _first_refused(ref, env, qcap, pcap, CHUNK)
            if first is None and f is not None:
                first = done - CHUNK + f
            per[done] = _ref_tree(ref)
        refused.append(first)
        trees.append(per)
    assert all(refused[g] is not None for g in range(0, G - 1, 2)) and all(refused[g] is None for g in range(1, G, 2))
    safe = (min(r for r in refused[:G - 1] if r is not None) - 1) // CHUNK * CHUNK   # the last chunk boundary before any refusal
    assert CHUNK <= safe < FULL_TOTAL
    eng, evaluator = make_engine()
    st = _capacities_are(eng, FULL_PF, FULL_SIMS, A, 'uct_ref')
    _set_roots(eng, envs)
    eng.set_active(active)
    for done in range(CHUNK, FULL_TOTAL + 1, CHUNK):
        search(eng, evaluator, CHUNK)
        if done <= safe:   # before the overflow: every game, the open ones included
            for g in range(G - 1):
                assert _tree(eng, g) == trees[g][done], 'game %d after %d simulations' % (g, done)
            if done == safe:
                assert eng.check().error_flags == 0
    with pytest.raises(HipError, match='block queue full'):
        eng.check()
    st = eng.stats()
    assert st.error_flags & BLOCKS_FULL and not st.error_flags & ~(BLOCKS_FULL | ARENA_FULL)
    assert st.first_bad_game == 0 and st.max_slots_used <= st.arena_slots and st.max_blocks_used <= qcap
    for g in range(1, G - 1, 2):   # the small neighbours: the oracle's, for the same number of simulations
        assert _tree(eng, g) == trees[g][FULL_TOTAL], 'neighbour %d' % g
    assert _tree(eng, G - 1) == ar.FRESH   # the inactive game
    for g in range(0, G - 1, 2):
        _offsets_inside(eng, g, st)
    # recovery: flags cleared, the flagged games reset -- a search of n_playout simulations is the oracle's again
    _clear(eng)
    mask = np.array([1 if g % 2 == 0 else 0 for g in range(G)], dtype=np.uint8)
    _set_roots(eng, envs, mask=mask)
    search(eng, evaluator, FULL_SIMS)
    for g in range(G - 1):
        if g % 2 == 0:
            assert _tree(eng, g) == trees[g][FULL_SIMS], 'game %d after the reset' % g
        else:
            ref = RefSearch(fn, FULL_TOTAL + FULL_SIMS, 5)
            ref.simulate(envs[g], 1.0)
            assert _tree(eng, g) == _ref_tree(ref), 'neighbour %d after the reset' % g
    assert _tree(eng, G - 1) == ar.FRESH
    assert eng.check().error_flags == 0
    eng.close()
    if close is not None:
        close(evaluator)


@pytest.mark.parametrize('B,n_row', [(6, 4), (9, 5), (15, 5)])
@pytest.mark.parametrize('route', ['plain', 'fused'])
def test_full_arena(route, B, n_row):
    """k_select + k_expand_backup and the fused k_tree_step with the synthetic evaluator: 5 x n_playout simulations in an arena
    sized for n_playout with a minimal pool_factor (a caller that runs more simulations than it sized for)."""
    from rlzero_amd.engine import MCTSEngine, SyntheticEvaluator

    def make():
        return (MCTSEngine(B, n_row, n_games=8, n_playout=FULL_SIMS, pool_factor=FULL_PF, device='cuda:0'), SyntheticEvaluator('vlin'))
    _full_arena_case(B, n_row, ev.vlin, make, lambda eng, evaluator, n: _search(route, eng, evaluator, n))


NET_FULL = [('two_launch', 6, 4), ('two_launch_graph', 6, 4), ('resident', 6, 4), ('resident', 15, 5)]


@pytest.mark.parametrize('route,B,n_row', NET_FULL, ids=['%s-%d' % c[:2] for c in NET_FULL])
def test_full_arena_net_routes(route, B, n_row):
    """k_tree_step_def (eager and replayed from a captured graph) and the resident kernels (k_trunk_split<RES> on 6 x 6, k_delta_res
    on 15 x 15), which go on looping over their simulations after a game has been flagged.  The oracle is fed the device's values."""
    import torch
    from test_production_routes import _Probe
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(3)
    net = PolicyValueNet(B)
    probe = _Probe(net, 'gomoku', B, n_row)

    def make():
        evaluator = HipNetEvaluator(net, B, 'cuda:0', max_boards=8)
        evaluator.resident_search = route == 'resident'
        eng = MCTSEngine(B, n_row, n_games=8, n_playout=FULL_SIMS, pool_factor=FULL_PF, device='cuda:0')
        assert evaluator.deferred_ok(eng) and evaluator.resident_ok(eng) == (route == 'resident')
        if route == 'resident':
            assert evaluator.resident_delta_ok(eng) == (B == 15)
        if route == 'two_launch_graph':
            eng.reset_games()
            eng.warm_graph(evaluator, CHUNK)
        return eng, evaluator

    def close(evaluator):
        evaluator.hip.check_flags()
        evaluator.hip.close()
    _full_arena_case(B, n_row, probe, make,
                     lambda eng, evaluator, n: _search('graph' if route == 'two_launch_graph' else 'own', eng, evaluator, n), close)
    probe.close()


def _growth(k):
    """Record slots a node of k children has taken from the bump allocator once all of them are visited (every outgrown block
    stays where it is until the next advance): 4 + 8 + ... + k."""
    total, cap = 0, 0
    while cap < k:
        cap = min(k, ar.FIRST_CAP) if cap == 0 else min(2 * cap, k)
        total += cap
    return total


def test_arena_full_uct_ref():
    """RZ_FLAG_ARENA_FULL under uct_ref: the selection's `fresh = 2` stop, reached on 15 x 15 by going on after BLOCKS_FULL until the
    visited-child blocks exhaust the record slots.  The arithmetic (rz_create: n_playout 16, pool_factor 0.01 -> qcap = 24 expanded
    nodes, cap = 24 * 16 + 2 * 225 + 64 = 898 slots), with the v0 evaluator and c_puct = 0 (every score is 0: the first child wins):
    simulation 1 expands the root, 2 .. 24 its first 23 children (BLOCKS_FULL from 25 on), 2 .. 226 visit the root's 225 children --
    1 + (4 + 8 + .. + 128 + 225) = 478 slots; from 227 on every simulation descends into child 0 (expanded, 224 children) and visits
    its next child: 4 + 8 + .. + 128 = 252 more slots after 128 of them (top = 730), and the 129th needs a block of 224: 954 > 898.
    That simulation -- number 355 -- is stopped at child 0 and flagged; the top stays at 730.  The late roots beside the game are
    the oracle's for the same number of simulations, and the tree of the game itself stays consistent (root N = simulations)."""
    from rlzero_amd._hip import HipError
    from rlzero_amd.engine import MCTSEngine, SyntheticEvaluator
    B, n_row, A = 15, 5, 225
    cap, pcap = ar.capacities(FULL_PF, FULL_SIMS, A, 'uct_ref')
    qcap = pcap // A
    assert (qcap, cap) == (24, 898)
    root_done = 1 + A                                       # simulations until every child of the root is visited
    top_root = 1 + _growth(A)
    fit, top, block = 0, top_root, 0                        # children of child 0 visited before the block that does not fit
    while True:
        nxt = min(A - 1, ar.FIRST_CAP) if block == 0 else min(2 * block, A - 1)
        if top + nxt > cap:
            break
        top, block, fit = top + nxt, nxt, nxt
    first_full = root_done + fit + 1
    assert (top_root, top, first_full) == (478, 730, 355)
    envs = [RefGomoku(B, n_row), ar.late_root(B, n_row, 3, 1), RefGomoku(B, n_row), ar.late_root(B, n_row, 2, 2)]
    eng = MCTSEngine(B, n_row, n_games=4, n_playout=FULL_SIMS, c_puct=0.0, pool_factor=FULL_PF, device='cuda:0')
    _capacities_are(eng, FULL_PF, FULL_SIMS, A, 'uct_ref')
    _set_roots(eng, envs)
    eng.set_active(np.array([1, 1, 0, 1], dtype=np.uint8))
    evaluator = SyntheticEvaluator('v0')
    eng.simulate(evaluator, first_full - 1)
    st = eng.stats()
    assert st.error_flags == BLOCKS_FULL and st.max_slots_used == top and st.max_blocks_used == qcap
    eng.simulate(evaluator, 1)
    st = eng.stats()
    assert st.error_flags == BLOCKS_FULL | ARENA_FULL and st.max_slots_used == top
    with pytest.raises(HipError, match='arena full'):
        eng.check()
    total = first_full + 5
    eng.simulate(evaluator, 5)
    st = eng.stats()
    assert st.first_bad_game == 0 and st.max_slots_used == top <= st.arena_slots and st.max_blocks_used == qcap
    _offsets_inside(eng, 0, st)
    got = eng.tree_dump(0)
    assert got[()][0] == total and len(got) == 1 + A + fit   # every simulation counted at the root; no node past the refused block
    for g in (1, 3):
        ref = RefSearch(ev.v0, total, 0.0)
        ref.simulate(envs[g], 1.0)
        assert _tree(eng, g) == _ref_tree(ref), 'neighbour %d' % g
    assert _tree(eng, 2) == ar.FRESH
    eng.close()


@pytest.mark.parametrize('B,n_row,total', [(6, 4, 80), (15, 5, 480)], ids=['6', '15'])
def test_full_arena_in_flight(B, n_row, total):
    """sims_in_flight = 4, both implementations (the level-synchronous k_tree_step_ml and its one-wave restatement k_tree_step_vl).
    6 x 6: BLOCKS_FULL (the `fits` guard of the bump allocation).  15 x 15 with v0 and c_puct = 0 (the search goes down the first
    child, as in test_arena_full_uct_ref): ARENA_FULL as well -- k_tree_step_ml's phase C, where a child block that cannot grow
    keeps its place and the slots that chose a child past it stop at the node.  There is no oracle for virtual loss: the small and
    inactive games must be bit-equal to the same configuration built with an ample pool_factor, and the two implementations must
    agree on them."""
    from rlzero_amd.engine import MCTSEngine, SyntheticEvaluator
    A = B * B
    kind, c_puct = ('vlin', 5.0) if B == 6 else ('v0', 0.0)
    envs, active = _full_batch(B, n_row)
    G = len(envs)
    cap, pcap = ar.capacities(FULL_PF, FULL_SIMS, A, 'uct_ref')
    small = {}
    for impl in ('level_sync', 'sequential'):
        for pf in (FULL_PF, 40.0):
            eng = MCTSEngine(B, n_row, n_games=G, n_playout=FULL_SIMS, c_puct=c_puct, pool_factor=pf, device='cuda:0', sims_in_flight=4,
                             in_flight_impl=impl)
            _set_roots(eng, envs)
            eng.set_active(active)
            evaluator = SyntheticEvaluator(kind)
            for _ in range(total // 40):
                eng.simulate(evaluator, 40)
            st = eng.stats()
            if pf == FULL_PF:
                assert (st.arena_slots, st.prior_floats) == (cap, pcap)
                assert st.error_flags == (BLOCKS_FULL | ARENA_FULL if B == 15 else BLOCKS_FULL), (impl, st.error_flags)
                assert st.first_bad_game == 0 and st.max_slots_used <= st.arena_slots and st.max_blocks_used <= pcap // A
                for g in range(0, G - 1, 2):
                    _offsets_inside(eng, g, st)
                    assert eng.tree_dump(g)[()][0] == total   # every simulation is counted at the root
            else:
                assert st.error_flags == 0
            small[impl, pf] = [_tree(eng, g) for g in range(1, G, 2)]
            assert small[impl, pf][-1] == ar.FRESH   # the inactive game
            eng.close()
    assert small['level_sync', FULL_PF] == small['level_sync', 40.0] == small['sequential', FULL_PF] == small['sequential', 40.0]


# ------------------------------------------------------------------------------------------------ C: a legitimate deep search
@pytest.mark.parametrize('score_mode', ['uct_ref', 'puct'])
@pytest.mark.parametrize('B', [9, 15])
def test_deep_search_fits(B, score_mode):
    """The default pool_factor, 64 simulations per move, vlin with c_puct = 0: each search is as close to depth-first as the rule
    allows -- the worst case for '16 record slots per expansion' (a first block of 4 per new node) and the only place where the
    reserve (n_playout + 1) * 8 + 2 A of the carry rule meets a tree that is not breadth-first.  Ten moves, always keeping the
    most-visited child (a late root among the starts: under uct_ref an open board's search cannot leave the root's children): no
    flag but REUSE_DROPPED, the arena never full, the oracle's trees (following the predicted drops)."""
    from rlzero_amd.engine import MCTSEngine
    n_row, sims, c_puct, pf, A = 5, 64, 0.0, 2.0, B * B
    c = B * (B // 2) + B // 2
    starts = [RefGomoku(B, n_row), ar.late_root(B, n_row, 14, 1), ar.late_root(B, n_row, 20, 2)]
    if B == 9:   # (the oracle's search of an open 15 x 15 board is the slow part: one such game there)
        starts.append(RefGomoku.from_moves(B, n_row, [c]))
    caps = ar.capacities(pf, sims, A, score_mode)
    fn = _oracle_fn('vlin', score_mode)
    plan = [_plan_game(s, 'most', fn, sims, c_puct, score_mode, A, caps, 10) for s in starts]
    eng = MCTSEngine(B, n_row, n_games=len(starts), n_playout=sims, c_puct=c_puct, score_mode=score_mode, device='cuda:0')
    st = _capacities_are(eng, pf, sims, A, score_mode)
    evaluator = _device_eval('vlin', score_mode)
    _set_roots(eng, starts)
    drops = 0
    for m in range(11):
        active = np.array([1 if len(game) > m else 0 for game in plan], dtype=np.uint8)
        if not active.any():
            break
        eng.set_active(active)
        eng.simulate(evaluator, sims)
        st = eng.check()
        assert st.max_slots_used < st.arena_slots and not st.error_flags & ~REUSE_DROPPED
        for g, game in enumerate(plan):
            if active[g]:
                assert _tree(eng, g) == game[m]['searched'], 'game %d, search %d' % (g, m)
        moves = np.array([game[m]['move'] if active[g] and game[m]['move'] is not None else -2 for g, game in enumerate(plan)], dtype=np.int32)
        if (moves < 0).all():
            break
        eng.advance(moves)
        eng.step(np.where(moves >= 0, moves, -1).astype(np.int32))
        drops += sum(1 for g, game in enumerate(plan) if moves[g] >= 0 and game[m]['drop'])
        for g, game in enumerate(plan):
            if moves[g] >= 0:
                assert _tree(eng, g) == game[m]['advanced'], 'game %d, advance %d' % (g, m)
    st = eng.check()
    assert st.reuse_dropped == drops and not st.error_flags & ~REUSE_DROPPED and st.max_slots_used < st.arena_slots
    eng.close()
