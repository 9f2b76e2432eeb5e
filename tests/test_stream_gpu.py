"""Continuous self-play (BatchedSelfPlay.stream_start / stream_collect / stream_stop; rz_play_queue_ring, rz_play_queue_push): a
collection that does not stop the device at a round's end -- slots refill from a ring of game ids that the host tops up, the games
still running are continued by the next call, and weights and settings may change under them (epochs).

Pinned here: with constant weights every streamed game is bit for bit the game of the same id from run_device on a twin object
(moves, pi, winner; with the options on also the budget flags, the resignation fields and the root values), on the smallest ring
too and with stalls; a weight swap and a threshold change between collects give the same bits twice, the plies of the first epoch
equal the first weights' twin and the games of the second epoch the second's; the stream ends and starts again on one object; what
it refuses; and the trainer's two rounds with either buffer."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

LAYOUTS = {   # tests/test_device_moves.py's shapes: one lane that replays whole-move graphs, two lanes that do not
    'resident_1lane': dict(board=6, n_in_row=4, n_games=6, n_playout=40, lanes=1),
    'connect4_2lanes': dict(board=(6, 7), n_in_row=4, n_games=10, n_playout=50, game='connect4', net_shape=(6, 7, 7), lanes=2,
                            use_graph=True, sims_per_graph=8, resident_search=False),
}
OPTIONS = dict(playout_cap=(6, 0.5), root_values=True)   # (with them: resignation, set by the test, and a schedule)
SEED, TWIN_GAMES = 9, {'resident_1lane': 130, 'connect4_2lanes': 200}   # (more than five of the smallest rings, and the games behind them)
_nets, _twins = {}, {}


def _net(layout, seed):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    if (layout, seed) not in _nets:
        torch.manual_seed(seed)
        _nets[layout, seed] = (PolicyValueNet(6, 7, 7) if layout == 'connect4_2lanes' else PolicyValueNet(6)).to('cuda:0')
    return _nets[layout, seed]


def _sp(layout, net, **kw):
    from rlzero_amd.selfplay import BatchedSelfPlay
    return BatchedSelfPlay.for_network(net, device='cuda:0', temperature=1.0, seed=SEED, **dict(LAYOUTS[layout], **kw))


def _close(sp):
    for st in sp.check():
        assert st.reuse_dropped == 0
    for lane in sp.lanes:
        lane.evaluator.hip.check_flags()
        lane.eng.close()


def _twin(layout, seed=2):
    """{game id: Trajectory} of run_device on a twin object under the weights of ``seed``: computed once, left unchanged."""
    if (layout, seed) not in _twins:
        sp = _sp(layout, _net(layout, seed))
        _twins[layout, seed] = dict((t.game_id, t) for t in sp.run_device(range(TWIN_GAMES[layout])))
        _close(sp)
    return _twins[layout, seed]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _equal(got, want, plies=None, options=False):
    """A streamed game against the twin's game of its id, bit for bit (``plies``: the first plies only)."""
    k = len(want.moves) if plies is None else plies
    assert got.moves[:k] == want.moves[:k], got.game_id
    assert np.array_equal(_bits(got.pis[:k]), _bits(want.pis[:k])), got.game_id
    if plies is not None:
        return
    assert (got.winner, len(got.moves)) == (want.winner, len(want.moves)), got.game_id
    if options:
        assert (got.resigned, got.no_resign) == (want.resigned, want.no_resign), got.game_id
        for name in ('full', 'resign_stats', 'root_values'):
            a, b = getattr(got, name), getattr(want, name)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (got.game_id, name)
        assert np.float32(got.fp_margin).tobytes() == np.float32(want.fp_margin).tobytes(), got.game_id


def _same_runs(a, b):
    assert [t.game_id for t in a] == [t.game_id for t in b]
    for x, y in zip(a, b):
        _equal(x, y)
        assert x.epochs.tobytes() == y.epochs.tobytes(), x.game_id


def _gap_free(returned, running, first=0):
    ids = sorted([t.game_id for t in returned] + list(running))
    assert ids == list(range(first, first + len(ids))), ids


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_three_collects_equal_run_device(layout):
    """Constant weights, three collects of n = slots: every returned game is the twin's game of its id, every game is in epoch 0, a
    collect returns at least n games with the look-ahead of the stream unread, and the returned and the running ids are one range."""
    from rlzero_amd.selfplay import stream_lookahead
    twin, sp = _twin(layout), _sp(layout, _net(layout, 2))
    assert (layout == 'resident_1lane') == all(lane.eng._ask(lane.evaluator)[0].resident for lane in sp.lanes)
    sp.stream_start()
    assert (layout == 'resident_1lane') == all(lane.move_graph is not None for lane in sp.lanes)
    ahead = stream_lookahead(sp._copy_every, sp._depth)
    out = []
    for _ in range(3):
        got = sp.stream_collect(sp.n_slots)
        assert len(got) >= sp.n_slots
        assert all(sum(len(rows) for rows, _ in lane.inflight) + len(lane.uncopied) == ahead for lane in sp.lanes)
        out.extend(got)
    for t in out:
        _equal(t, twin[t.game_id])
        assert t.epochs.dtype == np.int32 and len(t.epochs) == len(t.moves) and not t.epochs.any()
    running = sp.stream_running_ids()
    assert running and not set(running) & set(t.game_id for t in out)
    _gap_free(out, running)
    assert sp.stream_stop() == len(running)
    _close(sp)


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_the_smallest_ring_wraps(layout):
    """The ring at the smallest capacity the top-up allows (the default), more than five capacities' worth of games through it;
    a smaller one is refused."""
    from rlzero_amd.selfplay import stream_topup
    twin = _twin(layout)
    sp = _sp(layout, _net(layout, 2))
    copy_every = 1   # (one row per read-back: the smallest top-up of the layout)
    cap = stream_topup(sp.n_slots, copy_every, 1)
    with pytest.raises(ValueError, match='stream_topup'):
        sp.stream_start(queue_capacity=cap - 1, copy_every=copy_every, depth=1)
    sp.stream_start(copy_every=copy_every, depth=1)
    assert sp._queue_ids.numel() == cap and all(lane.eng.play_queue_cap == cap for lane in sp.lanes)
    out = []
    while len(out) <= 5 * cap:
        out.extend(sp.stream_collect(sp.n_slots))
    assert len(out) > 5 * cap
    for t in out:
        _equal(t, twin[t.game_id])
    out.extend(sp.stream_stop(finish=True))
    _gap_free(out, [])
    _close(sp)


def _swap_run(layout, n_second):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    first, second = _net(layout, 2), _net(layout, 3)
    net = (PolicyValueNet(6, 7, 7) if layout == 'connect4_2lanes' else PolicyValueNet(6)).to('cuda:0')
    net.load_state_dict(first.state_dict())
    sp = _sp(layout, net)
    sp.stream_start()
    out = sp.stream_collect(sp.n_slots)
    with torch.no_grad():
        net.load_state_dict(second.state_dict())
    sp.refresh_weights()
    assert sp.stream_epoch == 1
    out.extend(sp.stream_collect(n_second))
    out.extend(sp.stream_stop(finish=True))
    _close(sp)
    return out


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_a_weight_swap_between_collects(layout):
    """Other weights after the first collect, the whole run twice: the same bits and epochs both times; a game wholly in epoch 0 is
    the first weights' twin's, one wholly in epoch 1 the second's, and a straddling game's epoch-0 plies are the first twin's."""
    n_second = 3 * LAYOUTS[layout]['n_games']
    a, b = _swap_run(layout, n_second), _swap_run(layout, n_second)
    _same_runs(a, b)
    _gap_free(a, [])
    old, new = _twin(layout, 2), _twin(layout, 3)
    kinds = {'old': 0, 'new': 0, 'straddling': 0}
    for t in a:
        assert (np.diff(t.epochs) >= 0).all() and set(t.epochs.tolist()) <= {0, 1}
        k = int((t.epochs == 0).sum())
        if k == len(t.moves):
            _equal(t, old[t.game_id])
            kinds['old'] += 1
        elif k == 0:
            _equal(t, new[t.game_id])
            kinds['new'] += 1
        else:
            _equal(t, old[t.game_id], plies=k)
            kinds['straddling'] += 1
    assert kinds['straddling'] >= 1 and kinds['new'] >= 1 and kinds['old'] >= 1, kinds


def _threshold(trajs):
    """A threshold between two logged statistics near their median, two float32 steps apart at least."""
    s = np.unique(np.concatenate([t.resign_stats for t in trajs]))
    s = s[np.isfinite(s)]
    for i in range(len(s) // 2, len(s) - 1):
        if s[i + 1] > np.nextafter(np.nextafter(s[i], np.float32(2)), np.float32(2)):
            return (float(s[i]) + float(s[i + 1])) / 2
    raise AssertionError('no threshold')


def _options_run(t_first, t_second, temps):
    sp = _sp('resident_1lane', _net('resident_1lane', 2), resign=(t_first, 0.25), temperature_schedule=temps, **OPTIONS)
    sp.stream_start()
    out = sp.stream_collect(2 * sp.n_slots)
    if t_second is not None:
        sp.set_resign(t_second, 0.25)
        assert sp.stream_epoch == 1
        out.extend(sp.stream_collect(2 * sp.n_slots))
    out.extend(sp.stream_stop(finish=True))
    _close(sp)
    return out


def test_options_together_and_a_threshold_change():
    """Resignation with a threshold that fires, a playout cap, a temperature schedule and root values at once: the streamed games
    are run_device's, every field; then another threshold between two collects -- verified under each row's own epoch (the reader
    raises otherwise), the same bits twice."""
    from rlzero_amd.selfplay import step_schedule
    temps = step_schedule(1.0, 4, 1e-3)
    stats = _sp('resident_1lane', _net('resident_1lane', 2), resign=(float('-inf'), 0.0), temperature_schedule=temps, **OPTIONS)
    t_fires = _threshold(stats.run_device(range(12)))
    _close(stats)
    twin_sp = _sp('resident_1lane', _net('resident_1lane', 2), resign=(t_fires, 0.25), temperature_schedule=temps, **OPTIONS)
    twin = dict((t.game_id, t) for t in twin_sp.run_device(range(TWIN_GAMES['resident_1lane'])))
    _close(twin_sp)
    assert any(t.resigned for t in twin.values()) and any(t.no_resign for t in twin.values())
    out = _options_run(t_fires, None, temps)
    assert any(t.resigned for t in out)
    for t in out:
        _equal(t, twin[t.game_id], options=True)
    a, b = _options_run(t_fires, t_fires - 0.1, temps), _options_run(t_fires, t_fires - 0.1, temps)
    _same_runs(a, b)
    assert any(len(set(t.epochs.tolist())) == 2 for t in a)
    for x, y in zip(a, b):
        assert (x.resigned, x.no_resign, x.full.tobytes(), x.root_values.tobytes()) == (y.resigned, y.no_resign, y.full.tobytes(), y.root_values.tobytes())


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_a_wide_stall_margin(layout):
    """stall_margin 0.08: the host decides roughly one draw in six, at a position of the stream that the log's content fixes."""
    twin, sp = _twin(layout), _sp(layout, _net(layout, 2))
    sp.stream_start(stall_margin=0.08)
    out = sp.stream_collect(2 * sp.n_slots)
    out.extend(sp.stream_stop(finish=True))
    assert sp.stalls_resolved > 0
    for t in out:
        _equal(t, twin[t.game_id])
    _gap_free(out, [])
    _close(sp)


def test_stop_run_device_and_start_again():
    """stream_stop(finish=True) returns exactly the running games; run_device works on the object afterwards, and a second stream
    -- from another first id -- as well."""
    layout = 'resident_1lane'
    twin, sp = _twin(layout), _sp(layout, _net(layout, 2))
    sp.stream_start()
    out = sp.stream_collect(sp.n_slots)
    running = sp.stream_running_ids()
    rest = sp.stream_stop(finish=True)
    assert sorted(t.game_id for t in rest) == running
    for t in out + rest:
        _equal(t, twin[t.game_id])
    again = sp.run_device(range(20, 32))
    assert [t.game_id for t in again] == list(range(20, 32))
    for t in again:
        _equal(t, twin[t.game_id])
    sp.stream_start(first_game_id=40)
    more = sp.stream_collect(sp.n_slots)
    more.extend(sp.stream_stop(finish=True))
    _gap_free(more, [], first=40)
    for t in more:
        _equal(t, twin[t.game_id])
        assert t.epochs is not None
    assert all(t.epochs is None for t in again)
    _close(sp)


def test_what_an_open_stream_refuses():
    from rlzero_amd._hip import HipError
    from rlzero_amd.engine import MCTSEngine, SyntheticEvaluator
    from rlzero_amd.selfplay import BatchedSelfPlay
    layout = 'resident_1lane'
    sp = _sp(layout, _net(layout, 2))
    with pytest.raises(ValueError, match='no stream is open'):
        sp.stream_collect(1)
    sp.stream_start()
    for call, word in ((lambda: sp.run(range(2)), 'run'), (lambda: sp.run_device(range(2)), 'run_device'),
                       (lambda: sp.device_queue(range(2)), 'device_queue'), (lambda: sp.stream_start(), 'stream_start'),
                       (lambda: sp.device_attach(), 'stream is open')):
        with pytest.raises(ValueError, match=word):
            call()
    with pytest.raises(ValueError, match='before stream_start'):   # (its whole-move graph was captured without a cap)
        sp.set_playout_cap(5, 0.5)
    with pytest.raises(ValueError, match='before stream_start'):
        sp.set_root_values(True)
    sp.lanes[0].eng.play_match_on = True   # (what play_set_match leaves behind)
    with pytest.raises(ValueError, match='match'):
        sp.stream_collect(1)
    sp.lanes[0].eng.play_match_on = False
    assert len(sp.stream_collect(1)) >= 1   # ... and the stream is as it was
    with pytest.raises(HipError, match='rz_play_queue_push'):   # (count > capacity: the library's argument error)
        sp.lanes[0].eng.play_queue_push(0, sp._queue_ids.numel() + 1)
    sp.stream_stop()
    _close(sp)
    eng = MCTSEngine(6, 4, n_games=4, n_playout=20, device='cuda:0', sims_in_flight=2)   # a route without the device move step
    k2 = BatchedSelfPlay(eng, SyntheticEvaluator('vlin'), seed=1)
    with pytest.raises(ValueError, match='no device move step'):
        k2.stream_start()
    eng.close()


def test_a_push_over_unclaimed_ids_is_an_error_of_the_engine():
    """The ring is full after stream_start's push: one more id would overwrite an unclaimed one -- nothing is written, check() reports it."""
    from rlzero_amd._hip import HipError
    layout = 'resident_1lane'
    sp = _sp(layout, _net(layout, 2))
    sp.stream_start()
    sp.torch.cuda.synchronize()
    ids, ctl = sp._queue_ids.cpu().numpy().copy(), sp._queue_ctl.cpu().numpy().copy()
    cap = ids.size
    assert cap - (ctl[1] - ctl[0]) < cap   # (ids wait unclaimed)
    sp.lanes[0].eng.play_queue_push(10 ** 6, cap)
    sp.torch.cuda.synchronize()
    assert np.array_equal(sp._queue_ids.cpu().numpy(), ids) and int(sp._queue_ctl.cpu()[1]) == ctl[1]
    with pytest.raises(HipError, match='queue of game ids full'):
        sp.check()
    for lane in sp.lanes:
        lane.eng.close()


def _trainer():
    spec = importlib.util.spec_from_file_location('train_alphazero_stream', os.path.join(REPO, 'tools', 'train_alphazero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('buffer', ['host', 'device'])
def test_the_trainer_for_two_rounds(buffer, capsys, monkeypatch, tmp_path):
    """Two rounds at 6x6 with the host buffer, and with the device buffer, a value mix and the calibrated threshold: each round
    consumes at least n games, games carry over from the first round to the second, the last round stops the stream."""
    monkeypatch.chdir(tmp_path)
    mod = _trainer()
    kw = dict(device_replay=True, value_mix=0.5, resign='auto') if buffer == 'device' else {}
    pipe = mod.TrainPipeline(board_size=6, n_in_row=4, n_playout=40, game_batch_num=2, check_freq=50, selfplay_games_in_flight=6,
                             seed=3, batch_size=16, continuous_selfplay=True, **kw)
    pipe.run()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('continuous self-play:')]
    assert len(lines) == 3 and 'stopped' in lines[2], lines
    finished = [int(ln.split()[2]) for ln in lines[:2]]
    stale = [int(ln.split()[5]) for ln in lines[:2]]
    assert min(finished) >= 6 and stale[0] == 0 and stale[1] > 0, lines   # (plies of round 2's games were searched in round 1)
    assert int(lines[2].split()[4]) > 0   # (games were running when the stream stopped)
    assert not pipe._batched._streaming and len(pipe.data_buffer) > 0
    assert pipe._next_game_id >= sum(finished)
