"""Boards of 11, 15 and 16 rows -- the row-tile trunk, the receptive-field kernels (k_trunk_delta / k_delta_res) and the two- and
four-word bitboards -- against the REFERENCE'S OWN runs on weights whose values matter (tests/golden/g9_*, oracle.evaluators.sharp_weights:
value std >= 0.2 where numpy_weights' values are constant to 1e-4).

Every tolerance is read from the fixture: E = 4 x max |torch f32 - torch f64| of the value over every recorded position and leaf
(E_lp likewise for the log-probabilities), measured on the CPU when the fixture was generated; the factor: the device and torch
round independently (x 2), and the split-f16 trunk is allowed twice the exact-f32 kernel's error (x 2).  E <= 2e-6 and E_lp <= 2e-5
(tests/test_sharp_fixture.py).  The end-to-end tests compare only searches and plies that the oracle rebuilds identically under
values moved by +-E (four sign patterns) and in fp64 -- so no assertion here has an escape clause for near-ties.  The measured
figures: profiles/sharp_net/agreement.txt (profiles/sharp_net_agreement.py, whose functions these tests call)."""
import os
import sys

import numpy as np
import pytest
import sharp_fixture as sf

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles'))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('B', sf.BOARDS)
def test_a_the_net_on_the_reference_s_positions(B):
    """HipNet.forward (default route, 'direct', 'split_f16_tiles') and the receptive-field kernel (bases 1, 2 and 3 stones back, and
    without a base) on the 24 recorded positions: value within E, log-probabilities within E_lp of the reference's."""
    from sharp_net_agreement import forward_errors
    E, E_lp = sf.tolerances(B)
    errors = forward_errors(B)
    print(B, E, E_lp, errors)
    assert len(errors) == 7
    for route, (dv, dl) in errors.items():
        assert dv <= E and dl <= E_lp, (B, route, dv, E, dl, E_lp)


@pytest.mark.parametrize('B', sf.BOARDS)
def test_b_the_tree_rebuilds_the_reference_s_tree_from_its_values(B):
    """The reference's per-simulation leaf values fed through HostEvaluator: root record and whole tree bit for bit (boards of two
    and four bitboard words; up to 9 x 9 this is test_gpu_parity.test_replay_recorded_leaf_values)."""
    from rlzero_amd.engine import HostEvaluator
    from test_gpu_parity import _check_case, _engine, _make_env, _set_roots
    from oracle.gomoku_ref import RefGomoku
    for rec in sf.search(B)['cases']:
        n = rec['n']
        values = iter(sf.leaf_values(rec))
        boards = iter([rec['pre'] + p for p, _ in rec['leaves']])

        def replay(env, _values=values, _boards=boards):
            assert sorted(env.states.keys()) == sorted(next(_boards))
            legal = env.leagel_actions()
            return [(a, 1.0 / max(len(legal), 1)) for a in legal], next(_values)

        env = RefGomoku.from_moves(B, n, rec['pre'])
        eng = _engine(B, n, n_games=1, n_playout=rec['n_playout'])
        _set_roots(eng, [env], reset_trees=True)
        host = HostEvaluator(replay, lambda s0, s1, tm, last, B=B, n=n: _make_env(B, n, s0, s1, tm, last))
        _check_case(eng, host, dict(rec, n_nodes=len(rec['tree'])), env)
        eng.close()


@pytest.mark.parametrize('B', sf.BOARDS)
def test_c_every_leaf_the_reference_evaluated_on_the_receptive_field_route(B):
    """Base = the search's root, leaves = every non-terminal leaf of the recorded search, through rz_net_delta_leaves: value within E
    of the reference's; the late roots' searches hold leaves against the base and leaves that took the passes without one."""
    from sharp_net_agreement import leaf_errors
    E, _ = sf.tolerances(B)
    rows = leaf_errors(B)
    print(B, E, rows)
    for name, dv, delta, no_base in rows:
        assert dv <= E, (B, name, dv, E)
        assert delta > 0
    late = [r for r in rows if r[0] == 'late']
    if B != 11:
        assert late and all(r[2] > 0 and r[3] > 0 for r in late), late


@pytest.mark.parametrize('resident', [True, False], ids=['resident', 'two_launch'])
@pytest.mark.parametrize('B', sf.BOARDS)
def test_d_the_device_s_own_search_builds_the_reference_s_tree(B, resident):
    """All robust cases of a board in one engine, searched with the device's own values: every node's N equals the reference's dump,
    |W - W_ref| <= N E, pi within 1e-12 -- on the resident route (k_delta_res) and on the two-launch step (k_trunk_delta)."""
    from rlzero_amd.selfplay import visits_to_pi
    from sharp_net_agreement import search_on_device, tree_difference
    E, _ = sf.tolerances(B)
    cases = [c for c in sf.search(B)['cases'] if c['robust']]
    assert len(cases) >= 3
    trees, visits, stats, route = search_on_device(B, cases, resident)
    assert route.delta and route.resident == resident and stats['delta'] > 0, (route, stats)
    if resident:
        assert route.resident_delta and stats['prescans'] > 0, (route, stats)
    else:
        assert route.deferred and stats['prescans'] == 0, (route, stats)
    assert B != 15 or any(c['name'] == 'late' for c in cases)   # (the fixture keeps the 15 x 15 late root robust: test_sharp_fixture.py)
    if any(c['name'] == 'late' for c in cases):
        assert stats['no_base'] > 0, stats
    for g, (rec, tree) in enumerate(zip(cases, trees)):
        bad, worst = tree_difference(tree, rec)
        print(B, rec['name'], bad, worst, E)
        assert bad == 0, (B, rec['name'], bad)
        assert worst <= E, (B, rec['name'], worst, E)
        assert [int(visits[g][a]) for a in rec['acts']] == rec['N']
        pi = visits_to_pi(visits[g][rec['acts']], rec['T'])
        assert np.max(np.abs(pi - np.array([float.fromhex(p) for p in rec['pi']]))) <= 1e-12


@pytest.mark.parametrize('k', range(4))
def test_e_the_device_plays_the_reference_s_games(k):
    """The recorded games over their robust plies through the reference's API on the device: visit vectors and moves identical, and the
    searches ran on the receptive-field route."""
    from sharp_net_agreement import play_on_device
    game = sf.games()[k]
    agree, stats = play_on_device(game, game['robust_plies'])
    assert stats['delta'] > 0, stats
    assert agree == game['robust_plies'], (game['B'], game['seed'], agree, game['robust_plies'])
