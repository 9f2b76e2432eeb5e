"""Policy on demand (k_delta_res<false>: the two value planes of a leaf; k_trunk_policy_rows: the four policy planes of the records a
flush lists) against the REFERENCE'S OWN runs and against the net in float64, on boards of 11, 15 and 16 rows -- two- and four-word
bitboards, last moves up to cell 255, store columns of games 32 and up -- with values and logits that matter (tests/golden/g9_*,
oracle.evaluators.sharp_weights).  tests/test_policy_on_demand.py compares the two kernels only with their twin k_delta_res<true> on
11 x 11 and flat weights; tests/test_sharp_net_rows.py never attaches the move step, so it runs neither.

Every test runs in two modes on the same attached engine: 'on_demand' and 'store' (the switch off: the search writes the feature
store).  A failure in 'on_demand' alone lies in the two kernels or in the record's words (pend_lw, pend_stones); one in both, in the
heads GEMM by rows, the deferred priors or the f32 log-softmax.

Tolerances are the fixture's (tests/sharp_fixture.py), none from a device: E for a value -- |W - W_ref| <= N E at every node -- and,
for a prior, E_lp + 2^-22 on |log(float64(prior)) - logp64|: E_lp is four times torch's own f32 error of the log-probabilities (what
test_sharp_net_rows.test_a allows them), 2^-22 the f32 expf and the rounding of the stored prior (half an ulp each, relative).  The
float64 side is oracle.evaluators.net_forward on the CPU, one batch per case, computed once (profiles/sharp_net_agreement.logp64_of);
test_the_reference_alone_stays_four_times_inside_the_bound shows that torch f32 itself stays within E_lp / 4 + 2^-22 of it.  The
measured figures: profiles/sharp_net/agreement.txt."""
import os
import sys

import numpy as np
import pytest
import sharp_fixture as sf

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles'))

MODES = ('on_demand', 'store')
EXPF = 2.0 ** -22
MIN_EXPANDED = {11: 140, 15: 390, 16: 290}


def _cases(B):
    cases = sf.search(B)['cases']
    assert all(c['robust'] for c in cases), 'every g9 search case is robust (tests/test_sharp_fixture.py)'
    return cases


# ----------------------------------------------------------------------------------------------- 1. CPU: the preconditions
@pytest.mark.parametrize('B', sf.BOARDS)
def test_the_reference_alone_stays_four_times_inside_the_bound(B):
    """The nodes a case expands are its non-terminal leaves: enough of them, deep enough; and on them torch f32, one position a call
    as the reference evaluates, is within E_lp / 4 + 2^-22 of net_forward in float64 in max |log(f32 exp(logp32)) - logp64| over the
    legal cells -- the GPU tests below allow E_lp + 2^-22.  Over ALL expanded nodes the figures are 1.6e-6, 2.4e-6 and 3.0e-6 at 11, 15
    and 16 rows against 6.8e-6, 9.3e-6 and 1.2e-5, the smallest prior 2.3e-5; batch 1 takes about 25 s a board for all of them, so
    this test SAMPLES every eighth node of every case, the root's always among them."""
    import torch
    from oracle.evaluators import net_forward
    from sharp_net_agreement import expanded_leaves, leaf_planes, logp64_rows
    _, E_lp = sf.tolerances(B)
    w = sf.weights(B)
    worst, smallest, deepest = 0.0, 1.0, 0
    for rec in _cases(B):
        paths = expanded_leaves(rec)
        assert len(set(paths)) == len(paths) >= MIN_EXPANDED[B], (B, rec['name'], len(paths))
        assert paths[0] == ()
        deepest = max(deepest, max(len(p) for p in paths))
        sample = paths[::8]
        planes = leaf_planes(B, rec, sample)
        logp64 = logp64_rows(B, rec, sample)
        for i in range(len(sample)):
            with torch.no_grad():
                logp32 = net_forward(w, planes[i:i + 1])[0].numpy()[0]
            prior = np.exp(logp32)
            assert prior.dtype == np.float32
            legal = (planes[i, 0] + planes[i, 1]).reshape(-1) == 0
            assert legal.sum() == B * B - len(rec['pre']) - len(sample[i])
            worst = max(worst, float(np.max(np.abs(np.log(prior.astype(np.float64)) - logp64[i])[legal])))
            smallest = min(smallest, float(prior[legal].min()))
    print(B, worst, E_lp / 4 + EXPF, smallest, deepest)
    assert worst <= E_lp / 4 + EXPF, (B, worst, E_lp / 4 + EXPF)
    assert smallest >= 2.0 ** -100   # (no denormal prior: the relative bound on expf holds)
    assert B == 11 or deepest >= 3, deepest


# ----------------------------------------------------------------------------------------------- 2, 3. GPU: one search per board and mode
_searches = {}


def _searched(B, mode):
    """7 copies of every case of the board in one engine (case k in slots k, k + n, ..: game indices up to 34 / 41), one sim_chunk of
    the cases' simulations, everything read to the host once and left unchanged."""
    from sharp_net_agreement import COPIES, search_attached
    if (B, mode) not in _searches:
        try:
            _searches[B, mode] = search_attached(B, _cases(B), mode == 'on_demand', COPIES)
        except BaseException as exc:   # (kept: after a failure no dependent test starts the same search on the GPU again)
            _searches[B, mode] = exc
    if isinstance(_searches[B, mode], BaseException):
        raise _searches[B, mode]
    return _searches[B, mode]


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('B', sf.BOARDS)
def test_trees_of_a_search_on_the_move_step(B, mode):
    """test_sharp_net_rows.test_d's assertions for every slot: each node's N equals the reference's dump, |W - W_ref| <= N E, the root
    visits equal the record's, pi within 1e-12; and the copies of a case equal its first copy node by node, byte by byte."""
    from rlzero_amd.selfplay import visits_to_pi
    from sharp_net_agreement import COPIES, tree_difference
    cases = _cases(B)
    n, E = len(cases), sf.tolerances(B)[0]
    r = _searched(B, mode)
    assert COPIES == 7 and len(r['trees']) == 7 * n > 32
    assert r['route'].resident and r['route'].resident_delta
    assert r['launches'] == ({True: 1, False: 0} if mode == 'on_demand' else {True: 0, False: 1}), r['launches']
    assert r['stats']['delta'] > 0, r['stats']
    if any(c['name'] == 'late' for c in cases):
        assert r['stats']['no_base'] > 0, r['stats']
    for g, tree in enumerate(r['trees']):
        rec = cases[g % n]
        bad, worst = tree_difference(tree, rec)
        if g < n:
            print(B, mode, rec['name'], bad, worst, E)
        assert bad == 0, (B, mode, g, rec['name'], bad)
        assert worst <= E, (B, mode, g, rec['name'], worst, E)
        visits = r['visits'][g]
        assert [int(visits[a]) for a in rec['acts']] == rec['N'] and int(visits.sum()) == sum(rec['N'])
        pi = visits_to_pi(visits[rec['acts']], rec['T'])
        assert np.max(np.abs(pi - np.array([float.fromhex(p) for p in rec['pi']]))) <= 1e-12
        assert r['reachable'][g] == r['reachable'][g % n], (B, mode, g, rec['name'])


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('B', sf.BOARDS)
def test_priors_of_a_full_flush(B, mode):
    """The arena behind that search (on demand: every record flushed by rows): the expanded paths are the fixture's non-terminal
    leaves, every block has one prior per legal move, and each prior's log is within E_lp + 2^-22 of the float64 net's; root_priors()
    is the root's block scattered by action."""
    from sharp_net_agreement import block_errors, expanded_leaves, logp64_of, prior_errors
    cases = _cases(B)
    _, E_lp = sf.tolerances(B)
    r = _searched(B, mode)
    for k, rec in enumerate(cases):
        blocks = r['blocks'][k]
        assert set(blocks) == set(expanded_leaves(rec)), (B, mode, rec['name'])
        ref = logp64_of(B, rec)
        for path, (legal, pri) in blocks.items():
            assert len(pri) == len(legal) == B * B - len(rec['pre']) - len(path), (B, mode, rec['name'], path)
            worst, _ = block_errors({path: (legal, pri)}, ref)
            assert worst <= E_lp + EXPF, (B, mode, rec['name'], path, worst, E_lp + EXPF)
        legal, pri = blocks[()]
        for g in range(k, len(r['trees']), len(cases)):
            want = np.zeros(B * B, np.float32)
            want[legal] = pri
            assert np.array_equal(r['root_priors'][g].view(np.uint8), want.view(np.uint8)), (B, mode, g)
    rows = prior_errors(B, mode == 'on_demand', r)   # (the report's figures are these)
    print(B, mode, E_lp + EXPF, rows)
    assert [x[0] for x in rows] == [c['name'] for c in cases]
    assert all(worst <= E_lp + EXPF and wrong_k == 0 for _, worst, _, wrong_k in rows)


# ----------------------------------------------------------------------------------------------- 4. GPU: what a move keeps
@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('B,how', [(B, 'play_move') for B in sf.BOARDS] + [(15, 'move_graph')])
def test_priors_and_counts_a_move_keeps(B, how, mode):
    """A search and the device's move (the flush between the draw and the apply is the kept flush, on demand by rows): the new root is
    the fixture's child of the drawn move, N and W below it are the dump's subtree, and every reachable expanded node's priors are
    within the bound for pre + [move] + path.  Without the near-win root (a winning move would end the game); the graph at 15 rows."""
    from sharp_net_agreement import attached_twin, block_errors, boards_of, expanded_blocks, expanded_leaves, logp64_of, tree_difference
    cases = [c for c in _cases(B) if c['name'] != 'near_win']
    assert len(cases) == len(_cases(B)) - 1
    E, E_lp = sf.tolerances(B)
    twin = attached_twin(B, cases, mode == 'on_demand', graph=(how == 'move_graph'))
    eng = twin.eng
    eng.flush_kept_stats(reset=True)
    rows = twin.move()
    assert sorted(twin.slot_of.tolist()) == list(range(len(cases)))
    stones, to_move, last = eng.get_roots()
    checked = 0
    for row, slot in zip(rows, twin.slot_of.tolist()):
        rec = cases[slot]
        mv = int(row[3])
        assert row[4] & 16 and int(row[5]) == rec['n_playout']   # (searched; N of the root)
        assert [int(row[8 + a]) for a in rec['acts']] == rec['N']
        assert mv >= 0 and not row[4] & 2, (B, mode, rec['name'], mv, int(row[4]))   # (no stall at stall_margin 0: a move was drawn)
        if row[4] & 8:
            continue
        checked += 1
        assert mv in rec['acts'] and rec['N'][rec['acts'].index(mv)] > 0
        want_st, want_tm, want_last = boards_of([rec['pre'] + [mv]])
        assert np.array_equal(stones[slot], want_st[0]) and to_move[slot] == want_tm[0] and last[slot] == want_last[0] == mv
        below = dict(rec, tree=[[p[1:], n, w] for p, n, w in rec['tree'] if p and p[0] == mv])
        bad, worst = tree_difference(eng.tree_dump(slot), below)
        print(B, mode, how, rec['name'], mv, bad, worst, E)
        assert bad == 0 and len(below['tree']) > 0, (B, mode, rec['name'], mv, bad)
        assert worst <= E, (B, mode, rec['name'], mv, worst, E)
        blocks = expanded_blocks(eng, slot)
        assert set(blocks) == set(p[1:] for p in expanded_leaves(rec) if p and p[0] == mv), (B, mode, rec['name'], mv)
        worst, wrong_k = block_errors(blocks, logp64_of(B, rec), prefix=(mv, ))
        print(B, mode, how, rec['name'], mv, len(blocks), worst, E_lp + EXPF)
        assert wrong_k == 0 and worst <= E_lp + EXPF, (B, mode, rec['name'], mv, wrong_k, worst, E_lp + EXPF)
    assert checked >= len(cases) - 1, (checked, len(cases))   # (at most one game may have ended with its move)
    got, pending = eng.flush_kept_stats()
    assert 0 < got <= pending, (got, pending)
    assert twin.modes() == ({True: 1, False: 0} if mode == 'on_demand' else {True: 0, False: 1})
    twin.close()


# ----------------------------------------------------------------------------------------------- 5. GPU: twins beyond 11 x 11
def _position(B, stones, last):
    """Player 0's and player 1's cells alternately, then ``last`` by the player whose turn it is: no five, the game goes on."""
    from oracle.gomoku_ref import RefGomoku
    env = RefGomoku.from_moves(B, 5, list(stones) + [last])
    assert not env.game_end_winner()[0] and env.last_move == last
    return env


def _twin_moves(a, b, plies, without_base=0):
    import test_policy_on_demand as tpd
    for ply in range(plies):
        if ply < without_base:   # (test_rows_without_a_base's sequence: the bases dropped between the search and the move)
            for t in (a, b):
                t.search()
                t.ev.hip.delta_invalidate()
            rows = a.move(search=False), b.move(search=False)
        else:
            rows = a.move(), b.move()
        tpd._same(a, b, rows, ply)
    got, pending = a.eng.flush_kept_stats()
    assert 0 < got <= pending
    a.close()
    b.close()


@pytest.mark.gpu
def test_twins_on_three_word_boards():
    """13 x 13 (169 cells: three words), bit for bit against the twin that writes the store: the refill's empty boards and positions
    whose last moves are the corners 0, 12, 156, 168; the first two moves with the bases dropped behind the search."""
    import test_flush_kept as tfk
    import test_policy_on_demand as tpd
    from oracle.gomoku_ref import RefGomoku
    B = 13
    spread = [30, 31, 70, 71, 100, 101, 140, 141]   # both colours in words 0, 1 and 2
    roots = [RefGomoku(B, 5) for _ in range(4)] + [_position(B, spread, last) for last in (0, 12, 156, 168)]
    assert all(x >> 6 in (0, 1, 2) for x in spread) and 168 >> 6 == 2
    a, b = tpd._pair(tfk._net('gomoku', B)[0], len(roots), 200, board=B, roots=roots, roots_by_game=True)
    _twin_moves(a, b, 3, without_base=2)


@pytest.mark.gpu
def test_twins_on_four_word_boards_with_noise():
    """16 x 16, 40 games (the store's second tile), Dirichlet noise, 200 simulations, three moves: half the slots from the fixture's
    late root (14 empty cells: deep trees, kept leaves three stones down), half from positions whose last moves are 0, 15, 240 and 255
    with both colours' stones in all four words."""
    import test_flush_kept as tfk
    import test_policy_on_demand as tpd
    from oracle.gomoku_ref import RefGomoku
    B, G = 16, 40
    late = [c for c in sf.search(B)['cases'] if c['name'] == 'late'][0]
    assert B * B - len(late['pre']) == 14
    spread = [34, 35, 100, 101, 170, 171, 230, 231]
    assert sorted(set(x >> 6 for x in spread[0::2])) == sorted(set(x >> 6 for x in spread[1::2])) == [0, 1, 2, 3]
    made = [_position(B, spread, last) for last in (0, 15, 240, 255)]
    roots = [RefGomoku.from_moves(B, 5, late['pre']) if g % 2 == 0 else made[(g // 2) % 4] for g in range(G)]
    a, b = tpd._pair(tfk._net('gomoku', B)[0], G, 200, board=B, roots=roots, roots_by_game=True)
    _twin_moves(a, b, 3)
