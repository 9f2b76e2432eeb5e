"""The per-ply temperature schedule, host side (no GPU): the two builders, batch_pi_and_moves with one T per row, pi_temperature, what
set_temperature_schedule refuses, and the trainer's options."""
import contextlib
import importlib.util
import os

import numpy as np
import pytest
from conftest import REPO

from rlzero_amd.selfplay import BatchedSelfPlay, batch_pi_and_moves, decay_schedule, draw_move, step_schedule, visits_to_pi


def test_step_schedule():
    got = step_schedule(1.0, 4, 1e-3)
    assert got.dtype == np.float64
    assert got.tolist() == [1.0, 1.0, 1.0, 1.0, 1e-3]
    assert step_schedule(0.5, 0, 2.0).tolist() == [2.0]
    assert step_schedule(2, 1, 1).tolist() == [2.0, 1.0] and step_schedule(2, 1, 1).dtype == np.float64
    with pytest.raises(ValueError):
        step_schedule(1.0, -1, 1.0)


def test_decay_schedule():
    got = decay_schedule(1.0, 0.0, 1.0, 4)
    assert got.dtype == np.float64
    assert got.tolist() == [1.0, 0.5, 0.25, 0.125]
    # t_end + (t_start - t_end) * 0.5 ** (ply / halflife): powers of two are exact
    assert decay_schedule(1.0, 0.5, 2.0, 5)[[0, 2, 4]].tolist() == [1.0, 0.75, 0.625]
    want = [0.1 + (0.8 - 0.1) * 0.5 ** (p / 19.0) for p in range(7)]
    assert decay_schedule(0.8, 0.1, 19, 7).tolist() == want
    assert decay_schedule(1.0, 0.25, 3.0, 0).shape == (0, )


def _rows():
    """Visits with ties, illegal cells and rows of different legal counts (A = 9)."""
    visits = np.array([[5, 5, 0, 12, 12, 1, 0, 3, 3],
                       [0, 40, 40, 0, 0, 0, 0, 0, 1],
                       [7, 0, 0, 0, 0, 0, 0, 0, 0],
                       [1, 2, 3, 4, 5, 6, 7, 8, 9],
                       [9, 9, 9, 9, 0, 0, 0, 0, 0],
                       [0, 0, 0, 17, 0, 17, 2, 0, 0]], dtype=np.int64)
    legal = np.array([[1, 1, 1, 1, 1, 1, 0, 1, 1],
                      [0, 1, 1, 1, 0, 0, 0, 0, 1],
                      [1, 0, 0, 0, 0, 0, 0, 0, 0],
                      [1, 1, 1, 1, 1, 1, 1, 1, 1],
                      [1, 1, 1, 1, 1, 0, 0, 1, 0],
                      [0, 0, 1, 1, 0, 1, 1, 0, 0]], dtype=bool)
    visits = np.where(legal, visits, 0)
    uniforms = np.array([0.37, 0.5, 0.999, 0.0, 0.6180339887, 0.49999999])
    return visits, legal, uniforms


@pytest.mark.parametrize('temps', [[1.0, 0.5, 1e-3, 1.0, 0.5, 1e-3], [1e-3, 1e-3, 1.0, 0.5, 1.0, 0.5], [0.5] * 6])
def test_batch_with_a_temperature_per_row_is_the_scalar_call_per_row(temps):
    visits, legal, us = _rows()
    temps = np.array(temps)
    pis, moves = batch_pi_and_moves(visits, legal, temps, us)
    assert pis.dtype == np.float64 and pis.shape == visits.shape
    for r in range(len(us)):
        pi_r, mv_r = batch_pi_and_moves(visits[r:r + 1], legal[r:r + 1], float(temps[r]), us[r:r + 1])
        assert np.array_equal(pis[r].view(np.uint64), pi_r[0].view(np.uint64)), r
        assert moves[r] == mv_r[0]
        # ... and the per-game expressions of the reference
        acts = np.nonzero(legal[r])[0]
        want = visits_to_pi(visits[r][acts], float(temps[r]))
        assert np.array_equal(pis[r][acts].view(np.uint64), want.view(np.uint64)), r
        assert moves[r] == draw_move(acts, want, us[r])
    # the scalar call itself is unchanged by an array of that one T
    one = batch_pi_and_moves(visits, legal, 0.5, us)
    many = batch_pi_and_moves(visits, legal, np.full(len(us), 0.5), us)
    assert np.array_equal(one[0].view(np.uint64), many[0].view(np.uint64)) and np.array_equal(one[1], many[1])


class _Eng(object):
    n_cells = 9
    play_match_on = False


class _Lane(object):
    def __init__(self):
        self.eng, self.evaluator, self.stream = _Eng(), None, None


def _stub():
    sp = BatchedSelfPlay.__new__(BatchedSelfPlay)
    sp.lanes = [_Lane(), _Lane()]
    sp.eng, sp.seed, sp.temperature = sp.lanes[0].eng, 3, 1.0
    sp.temperature_schedule, sp.pi_temperature = None, None
    sp._on = lambda lane: contextlib.nullcontext()
    return sp


def test_lookup_by_ply_and_pi_temperature():
    visits, legal, us = _rows()
    plies = np.array([0, 1, 2, 3, 7, 8])
    sp = _stub()
    assert sp._temps(plies) == 1.0
    sp.set_temperature_schedule(step_schedule(1.0, 2, 1e-3))
    assert sp._temps(plies).tolist() == [1.0, 1.0, 1e-3, 1e-3, 1e-3, 1e-3]
    pis, moves = sp._pis_moves(visits, legal, plies, us)
    want = batch_pi_and_moves(visits, legal, np.array([1.0, 1.0, 1e-3, 1e-3, 1e-3, 1e-3]), us)
    assert np.array_equal(pis.view(np.uint64), want[0].view(np.uint64)) and np.array_equal(moves, want[1])
    # pi_temperature: pi at the other T, the chosen moves unchanged
    sp.set_temperature_schedule(step_schedule(1.0, 2, 1e-3), pi_temperature=0.5)
    pis2, moves2 = sp._pis_moves(visits, legal, plies, us)
    assert np.array_equal(moves2, moves)
    assert np.array_equal(pis2.view(np.uint64), batch_pi_and_moves(visits, legal, 0.5, us)[0].view(np.uint64))
    assert not np.array_equal(pis2, pis)
    for r in range(len(us)):
        acts = np.nonzero(legal[r])[0]
        assert np.array_equal(pis2[r][acts].view(np.uint64), visits_to_pi(visits[r][acts], 0.5).view(np.uint64))
    # off again
    sp.set_temperature_schedule(None)
    assert sp.temperature_schedule is None and sp.pi_temperature is None and sp._temps(plies) == 1.0


def test_set_temperature_schedule_refuses():
    sp = _stub()
    for bad in ([1.0, 0.0], [-1.0], [1.0, float('nan')], [float('inf')], [], [1.0] * 10):
        with pytest.raises(ValueError):
            sp.set_temperature_schedule(bad)
        assert sp.temperature_schedule is None
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            sp.set_temperature_schedule([1.0], pi_temperature=bad)
        assert sp.temperature_schedule is None and sp.pi_temperature is None
    sp.set_temperature_schedule([1.0] * 9)
    assert sp.temperature_schedule.tolist() == [1.0] * 9
    # a lane in match mode: its move step would refuse
    sp.lanes[1].eng = type('E', (_Eng, ), {'play_match_on': True})()
    with pytest.raises(ValueError, match='match'):
        sp.set_temperature_schedule([0.5])
    assert sp.temperature_schedule.tolist() == [1.0] * 9


def _trainer():
    spec = importlib.util.spec_from_file_location('train_alphazero_tool', os.path.join(REPO, 'tools', 'train_alphazero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trainer_parses_the_options():
    tool = _trainer()
    off = tool.parse_args([])
    assert off.temperature_schedule is None and off.pi_temperature is None
    args = tool.parse_args(['--games-in-flight', '16', '--temperature-schedule', 'step:1.0:30:0.001', '--pi-temperature', '0.5'])
    assert args.temperature_schedule == ('step', 1.0, 30, 0.001) and args.pi_temperature == 0.5
    assert tool.temperature_table(args.temperature_schedule, 36).tolist() == [1.0] * 30 + [0.001]
    args = tool.parse_args(['--games-in-flight', '16', '--temperature-schedule', 'decay:1:0.25:6'])
    assert args.temperature_schedule == ('decay', 1.0, 0.25, 6.0) and args.pi_temperature is None
    table = tool.temperature_table(args.temperature_schedule, 36)
    assert table.shape == (36, ) and table[0] == 1.0 and table[6] == 0.25 + 0.75 * 0.5
    assert np.array_equal(table, decay_schedule(1.0, 0.25, 6.0, 36))
    for bad in (['--temperature-schedule', 'step:1.0:30:0.001'],                      # not batched
                ['--pi-temperature', '1.0'],                                           # not batched
                ['--games-in-flight', '16', '--temperature-schedule', 'step:1.0:30'],
                ['--games-in-flight', '16', '--temperature-schedule', 'step:1.0:3.5:0.1'],
                ['--games-in-flight', '16', '--temperature-schedule', 'step:0:30:0.001'],
                ['--games-in-flight', '16', '--temperature-schedule', 'step:1:-1:0.001'],
                ['--games-in-flight', '16', '--temperature-schedule', 'step:1:36:0.001'],   # 37 entries for 36 cells
                ['--games-in-flight', '16', '--temperature-schedule', 'decay:1:-0.1:6'],
                ['--games-in-flight', '16', '--temperature-schedule', 'decay:1:0.1:nan'],
                ['--games-in-flight', '16', '--temperature-schedule', 'linear:1:0.1:6'],
                ['--games-in-flight', '16', '--pi-temperature', '0'],
                ['--games-in-flight', '16', '--pi-temperature', 'warm']):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
    # the pipeline refuses them outside the batched mode too, as it refuses the gate match
    for kw in (dict(temperature_schedule=('step', 1.0, 4, 0.001)), dict(pi_temperature=1.0)):
        with pytest.raises(ValueError, match='batched'):
            tool.TrainPipeline(selfplay_games_in_flight=0, **kw)
