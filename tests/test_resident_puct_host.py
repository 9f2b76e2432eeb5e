"""The resident search under PUCT (rz_net_search_resident_puct, ABI 46), without a GPU: route.decide's opt-in switch leaves every Route
as it was while it is off and turns ``resident`` on exactly in the cells of its rule; the header declares the entry point and the
ctypes table matches; for_network's refusals (through plan_route) name their reason."""
import itertools
import os
import re

import pytest

from rlzero_amd import _hip, route
from rlzero_amd.selfplay import plan_route

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CUS = 256
BOARDS = [(3, 3), (6, 6), (6, 7), (9, 9), (10, 10), (11, 11), (15, 15)]
CELLS = list(itertools.product(BOARDS, ('uct_ref', 'puct'), (1, 4), ('auto', 'f32'), (True, False), (64, 256, 300)))


def _args(board, score_mode, in_flight, heads, use_positions, n_games):
    return dict(rows=board[0], cols=board[1], heads_algo=heads, use_positions=use_positions, score_mode=score_mode, in_flight=in_flight,
                n_games=n_games, n_cus=N_CUS)


def test_switch_off_changes_no_route():
    """Every cell, every other switch at both values: decide(resident_puct=False) is decide() without the argument."""
    for cell in CELLS:
        for algo, split_ok, same_board, resident_search in itertools.product(('split_f16', 'split_f16_tiles', 'direct'), (True, False),
                                                                             (True, False), (True, False)):
            kw = dict(_args(*cell), algo=algo, split_ok=split_ok, same_board=same_board, resident_search=resident_search, environ={})
            assert route.decide(resident_puct=False, **kw) == route.decide(**kw), (cell, algo, split_ok, same_board, resident_search)


def test_switch_on_is_resident_exactly_in_the_cells_of_the_rule():
    hits = 0
    for cell in CELLS:
        board, score_mode, in_flight, heads, use_positions, n_games = cell
        for algo, split_ok, same_board, resident_search in itertools.product(('split_f16', 'direct'), (True, False), (True, False), (True, False)):
            kw = dict(_args(*cell), algo=algo, split_ok=split_ok, same_board=same_board, resident_search=resident_search, environ={})
            off, on = route.decide(**kw), route.decide(resident_puct=True, **kw)
            rule = (algo == 'split_f16' and split_ok and use_positions and in_flight == 1 and score_mode == 'puct' and
                    board[0] <= 10 and board[1] <= 10 and same_board and heads != 'f32' and resident_search and n_games <= N_CUS)
            if score_mode == 'puct':
                assert not off.resident and not off.deferred, cell   # (today's PUCT cells: the three-launch step)
                assert on.resident == rule, (cell, algo, split_ok, same_board, resident_search)
            if rule:
                hits += 1
                assert on.resident_per_cu == 1 and not on.deferred and not on.needs_planes and not on.resident_delta
                assert route.resident_puct_refusal(board[0], board[1], algo, split_ok, heads, use_positions, resident_search, score_mode,
                                                   in_flight, n_games, N_CUS, same_board) is None
            else:
                assert on == off, (cell, algo, split_ok, same_board, resident_search)   # (the switch moves nothing else)
    assert hits == 5 * 2   # five boards of up to 10 rows x 64 / 256 games, everything else as the rule wants it
    # the integer constant of the C ABI names the rule as well as the string
    assert route.decide(6, 7, score_mode=_hip.SCORE_PUCT, n_games=6, n_cus=N_CUS, resident_puct=True).resident


def test_header_declares_the_entry_and_the_binding_matches():
    header = open(os.path.join(REPO, 'include', 'rlzero_hip.h')).read()
    assert '#define RZ_ABI_VERSION %d' % _hip.ABI_VERSION in header and _hip.ABI_VERSION >= 46
    m = re.search(r'int rz_net_search_resident_puct\(([^)]*)\);', header)
    assert m, 'include/rlzero_hip.h does not declare rz_net_search_resident_puct'
    params = [p.strip() for p in m.group(1).split(',')]
    assert params == ['rz_net *net', 'rz_engine *engine', 'int32_t n_sims', 'int32_t select_first', 'void *stream']
    table = open(os.path.join(REPO, 'rlzero_amd', '_hip.py')).read()
    row = re.search(r"'rz_net_search_resident_puct': \(c_int, \[([^\]]*)\]\)", table)
    assert row and [a.strip() for a in row.group(1).split(',')] == ['P', 'P', 'c_int32', 'c_int32', 'P']
    assert 'ABI 46' in header[header.index('RESIDENT SEARCH UNDER PUCT'):m.start()]


@pytest.mark.parametrize('kw, word', [
    (dict(rows=11, cols=11), '11 x 11'),
    (dict(rows=15, cols=15), 'up to 10 rows'),
    (dict(in_flight=4), 'sims_in_flight 4'),
    (dict(score_mode='uct_ref'), "score_mode 'uct_ref'"),
    (dict(host_evaluator=True), 'host evaluator'),
    (dict(net_algo='direct'), "net_algo 'direct'"),
    (dict(net_algo='winograd_f4'), 'split-f16 trunk'),
    (dict(n_games=300, lanes=1), '300 games per lane on 256 CUs'),
    (dict(n_games=1024), '512 games per lane'),        # (the table splits 1024 games into two lanes)
    (dict(resident_search=False), 'switched off'),
])
def test_for_network_refusals_name_their_reason(kw, word):
    """What BatchedSelfPlay.for_network(resident_puct=True) asks before it builds anything: a ValueError, never another route."""
    base = dict(rows=6, cols=7, game='connect4', net_algo=None, score_mode='puct', in_flight=1, n_games=6, n_cus=N_CUS)
    base.update(kw)
    with pytest.raises(ValueError) as err:
        plan_route(resident_puct=True, **base)
    assert 'resident_puct=True cannot be served' in str(err.value) and word in str(err.value), str(err.value)
    base.pop('host_evaluator', None), base.pop('lanes', None)
    plan_route(**base)   # (without the switch the same numbers plan a route as before)


def test_plan_route_with_the_switch_on():
    """Served: the plan is the PUCT plan (plan_lanes is told nothing new), and batches beyond the CU count go the way plan_lanes
    splits them -- 300 games are three lanes of 100."""
    for n_games in (6, 256, 300):
        want = plan_route(6, 7, 'connect4', None, 'puct', 1, n_games=n_games, n_cus=N_CUS)
        assert plan_route(6, 7, 'connect4', None, 'puct', 1, n_games=n_games, n_cus=N_CUS, resident_puct=True) == want
        assert want['resident_per_cu'] == 1 and not want['deferred']


def test_evaluator_switch_is_off_by_default():
    from rlzero_amd.engine import HipNetEvaluator
    assert HipNetEvaluator.resident_puct is False
    assert object.__new__(HipNetEvaluator).resident_puct is False
