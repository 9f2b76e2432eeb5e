"""Self-play resignation on the device (rz_root_values, rz_play_set_resign; BatchedSelfPlay.set_resign): the read-out is the
tree's own numbers in numpy fp64, a statistics-only rule changes no game, a resigned game is a prefix of the same game played out
(a game depends on (seed, game id) only), both loops agree, a captured move graph takes a new threshold, and the trainer's 'auto'
mode runs."""
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import REPO

pytestmark = pytest.mark.gpu

SEED = 13


def _net(kind):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(4)
    if kind == 'connect4':
        return PolicyValueNet(6, 7, 7).to('cuda:0'), dict(board=(6, 7), n_in_row=4, game='connect4', net_shape=(6, 7, 7))
    b = {'6x6': 6, '9x9': 9, '15x15': 15}[kind]
    return PolicyValueNet(b).to('cuda:0'), dict(board=b, n_in_row=4 if b == 6 else 5)


ROUTES = {
    'resident_6x6': ('6x6', dict(n_games=6, n_playout=40, lanes=1)),
    'two_launch_6x6': ('6x6', dict(n_games=6, n_playout=40, lanes=1, resident_search=False, use_graph=True, sims_per_graph=8)),
    'puct_6x6': ('6x6', dict(n_games=6, n_playout=40, lanes=1, score_mode='puct')),
    'connect4_compact': ('connect4', dict(n_games=6, n_playout=40, lanes=1)),
    'resident_15x15': ('15x15', dict(n_games=4, n_playout=24, lanes=1)),
}


def _sp(route, **extra):
    from rlzero_amd.selfplay import BatchedSelfPlay
    kind, kw = ROUTES[route]
    net, geo = _net(kind)
    return BatchedSelfPlay.for_network(net, device='cuda:0', temperature=1.0, seed=SEED, **geo, **dict(kw, **extra))


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _values_of_dump(dump):
    """{v_root, q_best} from eng.tree_dump in numpy fp64: the root and its visited children."""
    n, w = dump[()]
    v = -(np.float64(w) / np.float64(n)) if n > 0 else np.nan
    qs = [np.float64(cw) / np.float64(cn) for p, (cn, cw) in dump.items() if len(p) == 1 and cn > 0]
    return v, (max(qs) if qs else np.nan)


def _same_values(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(_bits(np.nan_to_num(got)), _bits(np.nan_to_num(want)))


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_root_values_bit_exact(route):
    sp = _sp(route)
    sp.run(range(len(sp.slot_game)), max_moves=3)   # (mid-game roots, kept subtrees)
    sp._simulate()
    assert route != 'resident_15x15' or (sp.lanes[0].evaluator.resident_ok(sp.lanes[0].eng)
                                         and sp.lanes[0].evaluator.resident_delta_ok(sp.lanes[0].eng))
    for lane in sp.lanes:
        with sp._on(lane):
            got = lane.eng.root_values()
        sp.torch.cuda.synchronize()
        for g in range(lane.eng.n_games):
            want = np.array(_values_of_dump(lane.eng.tree_dump(g)))
            assert _same_values(got[g], want), (route, g, got[g], want)
    for lane in sp.lanes:
        lane.eng.close()


def test_root_values_win_in_one():
    from rlzero_amd.engine import MCTSEngine, SyntheticEvaluator, int_to_bits
    eng = MCTSEngine(3, 3, n_games=2, n_playout=300, device='cuda:0')
    # X (player 0) on 0, 1; O on 3, 4; X to move wins on 2.  Game 1: an empty board, nothing searched yet
    stones = np.array([[int_to_bits(0b11), int_to_bits(0b11000)], [int_to_bits(0), int_to_bits(0)]], dtype=np.uint64)
    eng.set_roots(stones, [0, 0], [4, -1], reset_trees=True)
    vals = eng.root_values()
    assert np.isnan(vals).all()
    eng.simulate(SyntheticEvaluator('vlin'), 300)
    vals = eng.root_values()
    assert vals[0, 1] == 1.0 and np.isfinite(vals).all()
    for g in range(2):
        assert _same_values(vals[g], np.array(_values_of_dump(eng.tree_dump(g))))
    eng.close()


def _same_games(a, b, stats=True):
    assert [t.game_id for t in a] == [t.game_id for t in b]
    for x, y in zip(a, b):
        assert (x.winner, x.moves, x.resigned, x.no_resign) == (y.winner, y.moves, y.resigned, y.no_resign), x.game_id
        assert np.array_equal(np.asarray(x.pis).view(np.uint64), np.asarray(y.pis).view(np.uint64)), x.game_id
        assert np.float32(x.fp_margin).tobytes() == np.float32(y.fp_margin).tobytes(), x.game_id
        if stats:
            assert x.resign_stats.tobytes() == y.resign_stats.tobytes(), x.game_id


def _threshold(trajs):
    """A threshold between two logged statistics near their median, at least two float32 steps apart: the fp64 rule s < t and
    float32(s) < t then agree for every logged s."""
    s = np.unique(np.concatenate([t.resign_stats for t in trajs]))
    s = s[np.isfinite(s)]
    for i in range(len(s) // 2, len(s) - 1):
        if s[i + 1] > np.nextafter(np.nextafter(s[i], np.float32(2)), np.float32(2)):
            return (float(s[i]) + float(s[i + 1])) / 2
    raise AssertionError('no threshold')


def _check_prefix(base, got, t, frac, would):
    """base: the statistics-only run (every game played out); got: the same games under threshold t."""
    from rlzero_amd.selfplay import fp_margin, resign_uniform
    n_resigned, n_would = 0, 0
    for b, r in zip(base, got):
        assert b.game_id == r.game_id and not b.resigned
        calib = bool(resign_uniform(SEED, b.game_id) < frac)
        assert r.no_resign == calib, b.game_id
        below = np.nonzero(b.resign_stats < t)[0]
        if calib:
            assert not r.resigned and (r.moves, r.winner) == (b.moves, b.winner), b.game_id
            assert np.array_equal(np.asarray(r.pis).view(np.uint64), np.asarray(b.pis).view(np.uint64))
            assert r.resign_stats.tobytes() == b.resign_stats.tobytes()
            assert np.float32(r.fp_margin).tobytes() == fp_margin(b.resign_stats, b.winner).tobytes()
            n_would += below.size
        elif below.size == 0:
            assert not r.resigned and r.moves == b.moves and r.winner == b.winner
        else:
            k = int(below[0])
            n_resigned += 1
            assert r.resigned and r.moves == b.moves[:k] and r.winner == 1 - k % 2, b.game_id
            if k:
                assert np.array_equal(np.asarray(r.pis).view(np.uint64), np.asarray(b.pis)[:k].view(np.uint64))
            assert r.resign_stats.tobytes() == b.resign_stats[:k + 1].tobytes()
            assert np.isnan(r.fp_margin)
    assert would == n_would
    return n_resigned


@pytest.mark.parametrize('route', ['resident_6x6', 'connect4_compact', 'two_launch_6x6'])
def test_statistics_only_then_prefix(route):
    ids = list(range(20))
    plain = _sp(route).run_device(ids)
    sp = _sp(route, resign=(float('-inf'), 0.0))
    stats = sp.run_device(ids)
    _same_games(plain, stats, stats=False)
    assert plain[0].resign_stats is None and all(not t.resigned and not t.no_resign for t in stats)
    assert all(len(t.resign_stats) == len(t.moves) and np.isfinite(t.resign_stats).all() for t in stats)
    host = sp.run(ids)   # the host loop's float32(max(root_values())) == the logged word 7
    _same_games(stats, host)
    t, frac = _threshold(stats), 0.25
    sp.set_resign(t, frac)
    sp.resign_would = 0
    dev = sp.run_device(ids)
    assert _check_prefix(stats, dev, t, frac, sp.resign_would) >= 3
    sp.resign_would = 0
    _same_games(dev, sp.run(ids))
    assert _check_prefix(stats, dev, t, frac, sp.resign_would) >= 3
    for lane in sp.lanes:
        lane.eng.close()


@pytest.mark.parametrize('lanes', [1, 3])
def test_both_loops_agree_9x9(lanes):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    from rlzero_amd.selfplay import BatchedSelfPlay, calibrate_resign_threshold
    torch.manual_seed(3)
    net = PolicyValueNet(9).to('cuda:0')
    kw = dict(n_games=6, n_playout=32, lanes=lanes, use_graph=True, sims_per_graph=8, device='cuda:0', seed=SEED)
    ids = list(range(2, 16))
    sp = BatchedSelfPlay.for_network(net, 9, 5, resign=(float('-inf'), 1.0), **kw)
    stats = sp.run_device(ids)
    assert all(t.no_resign for t in stats)
    t = calibrate_resign_threshold(stats, 0.3)
    assert np.isfinite(t)
    sp.set_resign(_threshold(stats), 0.2)
    a = sp.run_device(ids)
    b = sp.run(ids, pipelined=lanes > 1)
    _same_games(a, b)
    assert any(x.resigned for x in a)
    for lane in sp.lanes:
        lane.eng.close()


def test_new_threshold_reaches_the_move_graph():
    ids = list(range(16))
    sp = _sp('resident_6x6', resign=(float('-inf'), 0.0))
    sp.device_attach()
    graph = sp.lanes[0].move_graph
    assert graph is not None
    stats = sp.run_device(ids)
    t = _threshold(stats)
    sp.set_resign(t, 0.0)
    assert sp.lanes[0].move_graph is graph   # no new capture
    sp.resign_would = 0
    got = sp.run_device(ids)
    assert sp.lanes[0].move_graph is graph
    assert _check_prefix(stats, got, t, 0.0, sp.resign_would) >= 3
    # off again: the same graph plays every game out
    sp.set_resign(None)
    off = sp.run_device(ids)
    _same_games(stats, off, stats=False)
    assert all(x.resign_stats is None for x in off)
    # an object attached WITHOUT a rule: the first rule captures the move graph again, and it is obeyed
    sp2 = _sp('resident_6x6')
    sp2.device_attach()
    g0 = sp2.lanes[0].move_graph
    sp2.set_resign(t, 0.0)
    assert sp2.lanes[0].move_graph is not g0 and sp2.lanes[0].eng.play_resign_on
    _same_games(got, sp2.run_device(ids))
    for lane in sp.lanes + sp2.lanes:
        lane.eng.close()


def test_resident_15x15_resigns():
    ids = list(range(8))
    sp = _sp('resident_15x15', resign=(float('-inf'), 0.0))
    assert sp.lanes[0].evaluator.resident_ok(sp.lanes[0].eng) and sp.lanes[0].evaluator.resident_delta_ok(sp.lanes[0].eng)
    stats = sp.run_device(ids)
    t = _threshold(stats)
    sp.set_resign(t, 0.25)
    sp.resign_would = 0
    got = sp.run_device(ids)
    assert _check_prefix(stats, got, t, 0.25, sp.resign_would) >= 1
    for lane in sp.lanes:
        lane.eng.close()


def test_trainer_auto_resign_smoke(tmp_path):
    cmd = [sys.executable, os.path.join(REPO, 'tools', 'train_alphazero.py'), '--board', '6', '--n-in-row', '4', '--playouts', '24',
           '--batches', '3', '--check-freq', '100', '--games-in-flight', '16', '--resign-threshold', 'auto', '--seed', '3']
    env = dict(os.environ, PYTHONPATH=REPO)
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('resign:')]
    assert len(lines) == 3, out.stdout[-2000:]
    first = float(lines[0].rsplit('next threshold', 1)[1])
    assert np.isfinite(first) and '0 of' in lines[0]
