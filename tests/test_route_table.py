"""The evaluation route, cell by cell, against the tables recorded before the rule moved into rlzero_amd/route.py.

``route_table.json`` (beside this file) was written at the commit before the move, "Test every evaluation route across weight
reloads; drop stale bases", by the code of this module itself:

    python -c "import sys; sys.path[:0] = ['.', 'tests']; import test_route_table as t; t.write_tables()"

with ``_plan_cell`` replaced by the block that ``BatchedSelfPlay.for_network`` then held inline:

    deferred = (deferred_priors is not False and K == 1 and score_mode in ('uct_ref', 0)
                and game == 'gomoku' and 11 <= rows0 <= 16 and 11 <= cols0 <= 16
                and net_algo in (None, 'split_f16', 'split_f16_tiles', 'split_f16_fp8'))
    small_trunk = (K == 1 and deferred_priors is not False and score_mode in ('uct_ref', 0)
                   and net_algo in (None, 'split_f16', 'split_f16_tiles'))
    delta_res = (deferred and resident_search is not False and delta_trunk is not False and net_algo in (None, 'split_f16')
                 and os.environ.get('RZ_NET_DELTA', '1') != '0' and os.environ.get('RZ_NET_DELTA_RESIDENT', '1') != '0')
    compact_res = (small_trunk and not deferred and resident_search is not False and net_algo in (None, 'split_f16')
                   and max(rows0, cols0) <= 10 and compact_grid_board(rows0, cols0))
    return (deferred, rows0 * cols0 if (small_trunk or K > 1) else None, K, 2 if (delta_res or compact_res) else 1)

The evaluator's predicates are pure logic: they run here on objects made without their constructors (no library, no GPU), with a
stand-in for torch that reports 256 CUs.  Every cell must give what it gave then -- the odd ones included (two resident games per
CU answered by an evaluator that has no resident route): the move changed where the rule lives, not the rule.
"""
import itertools
import json
import os
import string
import types

import pytest

from rlzero_amd import _hip
from rlzero_amd.engine import HipNet, HipNetEvaluator

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'route_table.json')

BOARDS = ((3, 3), (6, 6), (6, 7), (7, 7), (8, 7), (9, 9), (10, 10), (11, 11), (15, 15), (16, 16), (17, 17))
ALGOS = ('direct', 'winograd_f4', 'split_f16', 'split_f16_tiles', 'split_f16_fp8')
SWITCHES = ('deferred_priors', 'delta_trunk', 'resident_search')
ENV = ('RZ_NET_DELTA', 'RZ_NET_DELTA_RESIDENT', 'RZ_NET_COMPACT')
VARIANTS = ('base', ) + SWITCHES + ENV   # nothing changed / that switch off / that variable '0'
# the axes inside one (variant, board, algo) row of the table, the last one fastest
INNER = dict(split_ok=(True, False), score_mode=(_hip.SCORE_UCT_REF, _hip.SCORE_PUCT), in_flight=(1, 4), heads=('auto', 'f32'),
             use_positions=(True, False), games=(64, 300, 512, 1024))
N_CUS = 256

_TORCH = types.SimpleNamespace(cuda=types.SimpleNamespace(
    get_device_properties=lambda device: types.SimpleNamespace(multi_processor_count=N_CUS)))


def make_evaluator(rows, cols, algo, split_ok=True, heads='auto', use_positions=True, off=None):
    """A HipNetEvaluator (and its HipNet) with the state the route depends on and nothing else."""
    hip = object.__new__(HipNet)
    hip.handle, hip.torch, hip.device, hip.n_cus = None, _TORCH, None, N_CUS   # (either way of asking for the CUs)
    hip.rows, hip.cols, hip.n_cells, hip.n_actions = rows, cols, rows * cols, rows * cols
    hip.algo, hip.heads_algo, hip._split_ok, hip._store, hip._delta_games, hip.generation = algo, heads, split_ok, (0, 0), 0, 0
    ev = object.__new__(HipNetEvaluator)
    ev.hip, ev.use_positions = hip, use_positions
    if off is not None:
        setattr(ev, off, False)
    return ev


def make_engine(rows, cols, score_mode=_hip.SCORE_UCT_REF, in_flight=1, games=64):
    return types.SimpleNamespace(rows=rows, cols=cols, score_mode=score_mode, sims_in_flight=in_flight, n_games=games, _capturing=False)


def outcome(ev, eng):
    return [bool(ev.needs_obs), bool(ev.deferred_ok(eng)), bool(ev.delta_ok(eng)), bool(ev.resident_delta_ok(eng)), bool(ev.resident_ok(eng)),
            int(ev.resident_per_cu(eng)), bool(ev.delta_three_launch_ok(eng)), bool(ev.hip.compact_resident())]


def _with_variant(variant, monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if variant in ENV:
        monkeypatch.setenv(variant, '0')
    return variant if variant in SWITCHES else None


def predicate_rows(monkeypatch):
    """-> {'variant board algo': [outcome of every INNER cell]} over the whole grid."""
    rows = {}
    for variant in VARIANTS:
        off = _with_variant(variant, monkeypatch)
        for (r, c), algo in itertools.product(BOARDS, ALGOS):
            cells = []
            for split_ok, score, k, heads, pos, games in itertools.product(*INNER.values()):
                cells.append(outcome(make_evaluator(r, c, algo, split_ok, heads, pos, off), make_engine(r, c, score, k, games)))
            rows['%s %dx%d %s' % (variant, r, c, algo)] = cells
    return rows


# ---------------------------------------------------------------------------------------------- for_network's plan
PLAN_BOARDS = tuple(('gomoku', b) for b in BOARDS) + (('connect4', (6, 7)), )
PLAN_ALGOS = (None, ) + ALGOS
PLAN_INNER = dict(score_mode=('uct_ref', 'puct'), in_flight=(1, 4), deferred_priors=(None, False), delta_trunk=(None, False),
                  resident_search=(None, False))
PLAN_VARIANTS = ('base', ) + ENV


def library_accepts(algo, rows, cols):
    """rz_net_set_algo refuses 'split_f16_fp8' on a board outside 11 .. 16 rows and columns: the only cells left out."""
    return algo != 'split_f16_fp8' or (11 <= rows <= 16 and 11 <= cols <= 16)


def _plan_cell(game, rows, cols, net_algo, score_mode, K, deferred_priors, delta_trunk, resident_search):
    from rlzero_amd.selfplay import plan_route
    kw = plan_route(rows, cols, game, net_algo, score_mode, K, deferred_priors=deferred_priors, delta_trunk=delta_trunk,
                    resident_search=resident_search, n_games=64, n_cus=N_CUS)
    return [kw['deferred'], kw['cells'], kw['in_flight'], kw['resident_per_cu']]


def plan_rows(monkeypatch):
    rows = {}
    for variant in PLAN_VARIANTS:
        _with_variant(variant, monkeypatch)
        for (game, (r, c)), algo in itertools.product(PLAN_BOARDS, PLAN_ALGOS):
            if library_accepts(algo, r, c):
                rows['%s %s %dx%d %s' % (variant, game, r, c, algo)] = [_plan_cell(game, r, c, algo, *cell)
                                                                         for cell in itertools.product(*PLAN_INNER.values())]
    return rows


# ---------------------------------------------------------------------------------------------- the table file
def _pack(rows):
    """Rows of outcomes -> (the distinct outcomes, {row: one letter per cell})."""
    kinds = sorted({json.dumps(cell) for cells in rows.values() for cell in cells})
    letter = {k: string.ascii_letters[i] for i, k in enumerate(kinds)}
    return [json.loads(k) for k in kinds], {name: ''.join(letter[json.dumps(cell)] for cell in cells) for name, cells in rows.items()}


def _unpack(kinds, packed):
    return {name: [kinds[string.ascii_letters.index(ch)] for ch in text] for name, text in packed.items()}


def write_tables():
    mp = pytest.MonkeyPatch()
    try:
        out = {}
        for key, rows in (('predicates', predicate_rows(mp)), ('plan', plan_rows(mp))):
            out[key + '_outcomes'], out[key] = _pack(rows)
    finally:
        mp.undo()
    with open(TABLE, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')


def _recorded(key):
    with open(TABLE) as f:
        table = json.load(f)
    return _unpack(table[key + '_outcomes'], table[key])


def _differences(got, want):
    assert sorted(got) == sorted(want)
    return ['%s cell %d: %s, recorded %s' % (name, i, a, b) for name in want for i, (a, b) in enumerate(zip(got[name], want[name])) if a != b
            ] + [name for name in want if len(got[name]) != len(want[name])]


def test_every_predicate_in_every_cell(monkeypatch):
    """(needs_obs, deferred_ok, delta_ok, resident_delta_ok, resident_ok, resident_per_cu, delta_three_launch_ok, compact_resident)
    over boards x algorithms x split_ok x score mode x simulations in flight x heads x use_positions x games, with each switch off
    and each environment variable '0' in turn: 7 x 7 040 cells."""
    want = _recorded('predicates')
    assert sum(len(v) for v in want.values()) == 7 * 7040
    bad = _differences(predicate_rows(monkeypatch), want)
    assert not bad, '%d cells differ, the first: %s' % (len(bad), bad[:5])


def test_for_network_plans_as_before(monkeypatch):
    """What for_network hands plan_lanes (deferred, cells, in_flight, resident_per_cu) in every cell the library accepts."""
    want = _recorded('plan')
    assert sum(len(v) for v in want.values()) == 4 * (12 * 6 - 9) * 32
    bad = _differences(plan_rows(monkeypatch), want)
    assert not bad, '%d cells differ, the first: %s' % (len(bad), bad[:5])


def test_plan_and_evaluator_agree_on_games_per_cu(monkeypatch):
    """The plan's resident_per_cu is what the evaluator built for the cell answers when its resident route is on, and 1 otherwise."""
    bad = []
    for variant in PLAN_VARIANTS:
        _with_variant(variant, monkeypatch)
        for (game, (r, c)), algo in itertools.product(PLAN_BOARDS, PLAN_ALGOS):
            if not library_accepts(algo, r, c):
                continue
            for score, k, dp, dt, rs in itertools.product(*PLAN_INNER.values()):
                ev = make_evaluator(r, c, algo or 'split_f16')
                for name, value in (('deferred_priors', dp), ('delta_trunk', dt), ('resident_search', rs)):
                    if value is not None:
                        setattr(ev, name, value)
                eng = make_engine(r, c, {'uct_ref': _hip.SCORE_UCT_REF, 'puct': _hip.SCORE_PUCT}[score], k)
                want = ev.resident_per_cu(eng) if ev.resident_ok(eng) else 1
                got = _plan_cell(game, r, c, algo, score, k, dp, dt, rs)[3]
                if got != want:
                    bad.append((variant, game, r, c, algo, score, k, dp, dt, rs, got, want))
    assert not bad, '%d cells differ, the first: %s' % (len(bad), bad[:5])
