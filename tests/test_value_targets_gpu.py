"""Value targets from the search on the GPU: the move step's side ring of root values (rz_play_set_root_values, k_play_draw), the
replay buffer's q array and mixed targets (rz_replay_enable_values, rz_replay_add_values, rz_replay_set_value_mix,
k_replay_gather / k_replay_sample <.., true>), Reanalyse's value refresh (rz_replay_update_values, k_replay_update_q;
ReplayReanalyser(targets=)) and the trainer's options.  Every comparison is bit for bit:

* the ring against float32 of ``MCTSEngine.root_values()[:, 0]`` read just before the draw, and ``run`` against ``run_device``;
* the targets against ``replay.mixed_value_targets`` (numpy) and against the host route, ``training_samples(value_mix=)`` through the
  trainer's host ReplayBuffer, entry for entry;
* a refreshed q against float32 of the root values of an INDEPENDENT engine given the same roots through the host ``set_roots``.

Shapes: Gomoku 6 x 6 (four in a row, 8 slots, 16 playouts), Gomoku 11 x 11 (five in a row, 4 slots, 24 playouts, three moves: the
k_delta_res route's root records), Connect4 4 x 5 (8 slots, 16 playouts); buffers of 64 positions (40 for Reanalyse), so the ring wraps."""
import numpy as np
import pytest
from conftest import REPO  # noqa: F401  (puts the repository on sys.path)

import replay_cases as rc
import replay_connect4_cases as c4

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SEED, CAPACITY = 7, 64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _net(game, board, seed=1):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(seed)
    return PolicyValueNet(board[0], board[1], board[1]) if game == 'connect4' else PolicyValueNet(board)


GAMES = {'gomoku6': ('gomoku', 6, 4, 8, 16), 'gomoku11': ('gomoku', 11, 5, 4, 24), 'connect4': ('connect4', (4, 5), 3, 8, 16)}


def _sp(case, **extra):
    from rlzero_amd.selfplay import BatchedSelfPlay
    game, board, n_in_row, slots, playouts = GAMES[case]
    kw = dict(game='connect4', net_shape=(board[0], board[1], board[1])) if game == 'connect4' else {}
    kw.update(extra)
    return BatchedSelfPlay.for_network(_net(game, board), board, n_in_row, n_games=slots, n_playout=playouts, lanes=1, device=DEV,
                                       temperature=1.0, seed=SEED, **kw)


def _close(*sps):
    for sp in sps:
        for lane in sp.lanes:
            lane.eng.close()


_PLAYED = {}


def _played(case):
    """12 games of ``case`` played once by run_device with root values on, shared by the tests and left unchanged."""
    if case not in _PLAYED:
        sp = _sp(case, root_values=True)
        _PLAYED[case] = sp.run_device(list(range(12)))
        _close(sp)
    return _PLAYED[case]


# ----------------------------------------------------------------------------------------------- the move step
@pytest.mark.parametrize('case, moves', [('gomoku6', 40), ('gomoku11', 3), ('connect4', 24)])
def test_ring_row_is_the_root_value_before_the_draw(case, moves):
    """Eager moves (so that the host can read between the search and the draw): after each play_move the ring's row is float32 of
    root_values()[:, 0] for every slot that held a game -- stalled ones included, their root does not change -- and NaN for idle
    ones.  6 game ids for 8 (4) slots: some slots stay idle from the start, the others fall idle as their games end."""
    import torch
    sp = _sp(case, root_values=True)
    lane = sp.lanes[0]
    eng = lane.eng
    sp.device_attach(queue_capacity=16, move_graphs=False)
    assert eng.play_values_on and tuple(eng.play_values.shape) == (eng.play_log.shape[0], eng.n_games)
    assert eng.play_values.dtype == torch.float32 and lane.move_graph is None
    G = eng.n_games
    sp.device_queue(list(range(G - 2)))
    idle_rows = busy_rows = 0
    for _ in range(moves):
        if sp._lane_quiet(lane):
            break
        state = eng.play_state()[2]
        sp._simulate_lane(lane, host_counts=False)
        vals = eng.root_values()                      # (waits: the search is done, the draw not enqueued)
        row = eng.play_move()
        torch.cuda.synchronize()
        ring = eng.play_values[row].cpu().numpy()
        holds = state != 0
        assert np.isnan(ring[~holds]).all(), (row, ring, state)
        assert _same(ring[holds], vals[holds, 0].astype(np.float32)), (row, ring, vals[:, 0], state)
        assert not np.isnan(ring[state == 1]).any()
        idle_rows += int((~holds).sum())
        busy_rows += int(holds.sum())
        lane.uncopied.append(row)
        sp._read_back(lane)
        sp._harvest(lane, keep=0)
    assert idle_rows >= 2 and busy_rows >= G - 2
    sp.device_stop()
    eng.check()
    _close(sp)


def _spy_records(sp):
    """The log rows as read_rows consumes them -> {(game id, ply): the record's words, bytes} of the SEARCHED records (how many idle
    rows trail a run, and how often a stalled record repeats, depends on how far the host lags: those are not compared)."""
    from rlzero_amd._hip import PLAY_RUNNING, PLAY_SEARCHED
    seen, inner = {}, sp.read_rows

    def read_rows(rows, lo=0, values=None):
        for r, g in zip(*np.nonzero((rows[..., 4] & (PLAY_RUNNING | PLAY_SEARCHED)) == (PLAY_RUNNING | PLAY_SEARCHED))):
            rec = rows[r, g]
            gid = int(np.ascontiguousarray(rec[0:2]).view(np.int64)[0])
            seen[(gid, int(rec[2]))] = rec.tobytes()
        return inner(rows, lo, values=values)
    sp.read_rows = read_rows
    return seen


def _same_games(a, b, values=True):
    assert [t.game_id for t in a] == [t.game_id for t in b]
    for x, y in zip(a, b):
        assert (x.winner, x.moves, x.resigned) == (y.winner, y.moves, y.resigned), x.game_id
        assert np.array_equal(np.asarray(x.pis).view(np.uint64), np.asarray(y.pis).view(np.uint64)), x.game_id
        if values:
            assert x.root_values.dtype == np.float32 and len(x.root_values) == len(x.moves) == len(y.root_values), x.game_id
            assert _same(x.root_values, y.root_values), (x.game_id, x.root_values, y.root_values)
            assert not np.isnan(x.root_values).any()


@pytest.mark.parametrize('case', ['gomoku6', 'connect4'])
def test_both_loops_return_the_same_root_values(case):
    """run_device (whole-move graphs where the route has them) and run, the same game ids: equal games and equal root_values; and
    an object without the option plays the same games, every searched record of its log word for word the same, with no root_values."""
    ids = list(range(12))
    dev = _played(case)
    sp = _sp(case, root_values=True)
    host = sp.run(ids)
    _same_games(dev, host)
    with_ring = _spy_records(sp)
    again = sp.run_device(ids)
    _same_games(dev, again)
    if case == 'gomoku6':
        assert sp.lanes[0].move_graph is not None              # (the ring is captured in the whole-move graph: one replay per move)
    plain = _sp(case)
    without = _spy_records(plain)
    off = plain.run_device(ids)
    _same_games(dev, off, values=False)
    assert all(t.root_values is None for t in off) and plain.lanes[0].eng.play_values is None and not plain.lanes[0].eng.play_values_on
    assert len(with_ring) >= sum(len(t.moves) for t in dev) and with_ring == without   # every searched record, word for word
    assert all(t.root_values is None for t in plain.run(ids[:4]))
    # the option changed on an attached object: it attaches again, and off again
    plain.set_root_values(True)
    assert plain.lanes[0].eng.play_values_on
    _same_games(dev, plain.run_device(ids))
    plain.set_root_values(False)
    assert not plain.lanes[0].eng.play_values_on and all(t.root_values is None for t in plain.run_device(ids[:4]))
    _close(sp, plain)


def test_both_loops_agree_with_stalls_resignation_and_a_cap():
    """A stall margin wide enough that plies stall (the host decides them; their value is their searched record's), resignation
    and a playout cap on: run_device and run still return identical root_values, aligned with the moves of resigned games too."""
    ids = list(range(16))
    sp = _sp('gomoku6', root_values=True, resign=(-0.02, 0.25), playout_cap=(6, 0.5))
    sp.device_attach(stall_margin=0.2)
    dev = sp.run_device(ids)
    assert sp.stalls_resolved > 0
    host = sp.run(ids)
    _same_games(dev, host)
    for x, y in zip(dev, host):
        assert x.full.tolist() == y.full.tolist() and _same(x.resign_stats, y.resign_stats)
        assert len(x.resign_stats) == len(x.moves) + (1 if x.resigned else 0)
    print('stalls resolved %d, games resigned %d of %d' % (sp.stalls_resolved, sum(t.resigned for t in dev), len(dev)))
    _close(sp)


def test_the_eleven_row_route_logs_its_root_records():
    """11 x 11 (k_delta_res): three moves of both loops, the games cut short -- the values of the plies played agree."""
    sp = _sp('gomoku11', root_values=True)
    assert sp.lanes[0].eng._ask(sp.lanes[0].evaluator)[0].resident_delta
    ids = list(range(4))
    sp.device_attach(queue_capacity=8)
    lane = sp.lanes[0]
    sp.device_queue(ids)
    for _ in range(3):
        sp.play_move_device()
    sp.device_drain()
    got = sp.book.buf['q'][:, :3].copy()
    slot_game = sp.book.slot_game.copy()
    assert sorted(slot_game.tolist()) == ids and not np.isnan(got).any()
    sp.device_stop()
    sp.run(ids, max_moves=3)
    for s, gid in enumerate(slot_game):
        host_slot = int(np.nonzero(sp.slot_game == gid)[0][0])
        assert _same(got[s], np.asarray(sp.slot_values[host_slot], dtype=np.float32)), (gid, got[s], sp.slot_values[host_slot])
    lane.eng.check()
    _close(sp)


def test_the_ring_is_refused_after_the_first_move_and_during_a_match():
    import torch
    from rlzero_amd._hip import HipError
    from rlzero_amd.engine import MCTSEngine
    from rlzero_amd.match import opening_arrays, paired_openings
    t = torch
    eng = MCTSEngine(6, 4, n_games=4, n_playout=16, device=DEV, add_noise=False)
    q = (t.arange(4, dtype=t.int64, device=DEV), t.tensor([0, 4], dtype=t.int32, device=DEV))
    eng.play_attach(1, 1.0, q[0], q[1])
    ring = eng.play_set_root_values(True)
    assert eng.play_values_on and ring is eng.play_values and np.isnan(ring.cpu().numpy()).all()
    assert eng.play_set_root_values(False) is None and not eng.play_values_on
    eng.play_set_root_values(True)
    eng.play_refill()                                     # a move step is enqueued: the draws to come hold their ring
    with pytest.raises(HipError, match='rz_play_set_root_values'):
        eng.play_set_root_values(True)
    with pytest.raises(HipError, match='rz_play_set_root_values'):
        eng.play_set_root_values(False)
    arrays = opening_arrays(paired_openings(6, 4, 2, 2, seed=1), 6, 4)
    eng.play_attach(1, 1.0, q[0], q[1])                   # attached again: off, and a ring may be set -- but then no match
    assert not eng.play_values_on and eng.play_values is None
    eng.play_set_root_values(True)
    with pytest.raises(HipError, match='root values'):
        eng.play_set_match(arrays)
    eng.play_attach(1, 1.0, q[0], q[1])
    eng.play_set_match(arrays)
    with pytest.raises(HipError, match='a match is on'):
        eng.play_set_root_values(True)
    assert not eng.play_values_on
    t.cuda.synchronize()
    eng.check()
    eng.close()


# ----------------------------------------------------------------------------------------------- the buffer
def _replay(case, capacity=CAPACITY, **kw):
    from rlzero_amd.replay import DeviceReplay
    game, board = GAMES[case][:2]
    return DeviceReplay(board, capacity, device=DEV, seed=SEED, game=game, **kw)


def _host_entries(case, games, capacity, lam):
    """The host route: the trainer's ReplayBuffer fed training_samples(value_mix=lam) -> (states, pis, zs) float32 of every entry."""
    game, board = GAMES[case][:2]
    S = 2 if game == 'connect4' else 8
    buf = rc.trainer().ReplayBuffer(S * capacity, board, game=game)
    for t in games:
        buf.extend_samples(t.training_samples(value_mix=lam))
    return rc.host_entries(buf)


@pytest.mark.parametrize('case', ['gomoku6', 'connect4'])
def test_buffer_keeps_q_and_mixes_the_target(case):
    from rlzero_amd.replay import kept_root_values, mixed_value_targets, pack_positions, replay_indices
    game, board = GAMES[case][:2]
    games = _played(case)
    S = 2 if game == 'connect4' else 8
    kept = sum(len(t.moves) for t in games)
    assert kept > CAPACITY + 8                               # the ring wraps
    dr, plain = _replay(case, search_values=True), _replay(case)
    assert dr.search_values and not plain.search_values and dr.value_mix == 0.0
    for call in (games[:5], games[5:6], games[6:]):
        assert dr.add(call) == plain.add(call) == sum(len(t.moves) for t in call)
    count, cursor, cap = dr._state()
    assert (count, cap) == (CAPACITY, CAPACITY) and cursor % cap != 0
    # read: the records are pack_positions', q the kept plies' root values
    records = tuple(x[-CAPACITY:] for x in pack_positions(games, board, game=game))
    stones, meta, pi, q = dr.read(values=True)
    assert np.array_equal(stones, records[0]) and np.array_equal(meta, records[1]) and _same(pi, records[2])
    want_q = kept_root_values(games)[-CAPACITY:]
    assert _same(q, want_q) and not np.isnan(q).any()
    assert len(dr.read()) == 3 and len(plain.read()) == 3
    z = (((meta >> 10) & 3) - 1).astype(np.float32)
    everything = np.arange(S * CAPACITY)
    base = [x.cpu().numpy() for x in plain.gather(everything)]
    assert _same(base[2], np.repeat(z, S))
    # lam = 0: the kernels without q -- the bits of a buffer that never had values
    for a, b in zip([x.cpu().numpy() for x in dr.gather(everything)], base):
        assert _same(a, b)
    for a, b in zip(dr.sample(96, step=3), plain.sample(96, step=3)):
        assert _same(a.cpu().numpy(), b.cpu().numpy())
    for lam in (0.25, 1.0):
        dr.set_value_mix(lam)
        assert dr.value_mix == lam
        got = [x.cpu().numpy() for x in dr.gather(everything)]
        want_zs = np.repeat(mixed_value_targets(z, q, lam), S)                 # (the symmetries of a position share its q)
        assert _same(got[0], base[0]) and _same(got[1], base[1])
        assert _same(got[2], want_zs) and not _same(got[2], base[2])
        host = _host_entries(case, games, CAPACITY, lam)                       # the host route, entry for entry
        for g, h in zip(got, host):
            assert _same(g, h)
        drawn = replay_indices(SEED, 5, 96, S * CAPACITY)
        for s_, g_ in zip(dr.sample(96, step=5), dr.gather(drawn)):
            assert _same(s_.cpu().numpy(), g_.cpu().numpy())
        assert _same(dr.sample(96, step=5)[2].cpu().numpy(), want_zs[drawn])
        import torch
        on_device = dr.gather(torch.from_numpy(drawn).to(DEV))
        assert _same(on_device[2].cpu().numpy(), want_zs[drawn])
    if case == 'gomoku6':
        assert _same(got[2], np.repeat(q, S))                                  # lam = 1 on stored values: q itself
    dr.set_value_mix(0.0)
    assert _same(dr.gather(everything)[2].cpu().numpy(), base[2])
    dr.close()
    plain.close()


def test_buffer_under_a_cap_and_without_values():
    """Under a playout cap the kept plies are the full-budget ones -- their q, in order; a trajectory without root values stores NaN
    and its target stays z at every lam."""
    from rlzero_amd.replay import kept_root_values, mixed_value_targets
    games = _played('gomoku6')
    rs = np.random.RandomState(4)
    from rlzero_amd.selfplay import Trajectory
    capped = []
    for t in games[:6]:
        full = rs.rand(len(t.moves)) < 0.5
        capped.append(Trajectory(t.game_id, t.board_size, t.n_in_row, t.moves, t.pis, t.winner, full=full, root_values=t.root_values))
    bare = Trajectory(99, 6, 4, games[6].moves, games[6].pis, games[6].winner)
    assert bare.root_values is None
    dr = _replay('gomoku6', capacity=400, search_values=True)
    assert dr.add(capped + [bare]) == sum(int(t.full.sum()) for t in capped) + len(bare.moves)
    stones, meta, pi, q = dr.read(values=True)
    n_capped = len(q) - len(bare.moves)
    assert _same(q, kept_root_values(capped + [bare])) and _same(q[:n_capped], np.concatenate([t.root_values[t.full] for t in capped]))
    assert np.isnan(q[n_capped:]).all() and not np.isnan(q[:n_capped]).any()
    z = (((meta >> 10) & 3) - 1).astype(np.float32)
    for lam in (0.5, 1.0):
        dr.set_value_mix(lam)
        zs = dr.gather(np.arange(8 * len(q)))[2].cpu().numpy()
        assert _same(zs, np.repeat(mixed_value_targets(z, q, lam), 8))
        assert _same(zs[8 * n_capped:], np.repeat(z[n_capped:], 8))
        host = _host_entries('gomoku6', capped + [bare], 400, lam)
        assert _same(zs, host[2])
    dr.close()


def test_buffer_refusals():
    from rlzero_amd._hip import HipError
    games = _played('gomoku6')
    plain = _replay('gomoku6')
    for lam in (0.25, 1.0):
        with pytest.raises(ValueError, match='search values'):
            plain.set_value_mix(lam)
    plain.set_value_mix(0.0)
    assert plain.lib.rz_replay_set_value_mix(plain.handle, 0.5) != 0 and b'rz_replay_enable_values' in plain.lib.rz_last_error()
    with pytest.raises(ValueError):
        plain.read(values=True)
    plain.add(games[:1])
    with pytest.raises(ValueError, match='empty'):
        plain.enable_search_values()
    assert plain.lib.rz_replay_enable_values(plain.handle, plain._stream()) != 0
    assert not plain.search_values
    late = _replay('gomoku6')
    late.enable_search_values()
    late.enable_search_values()                              # (a second call: nothing happens)
    assert late.search_values
    for lam in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            late.set_value_mix(lam)
        assert late.lib.rz_replay_set_value_mix(late.handle, lam) != 0
    late.add(games[:2])
    late.set_value_mix(1.0)
    q = late.read(values=True)[3]
    assert _same(late.gather(np.arange(8 * len(q)))[2].cpu().numpy(), np.repeat(q, 8))
    with pytest.raises(HipError):
        late.read(first=0, n=len(q) + 1, values=True)
    plain.close()
    late.close()


# ----------------------------------------------------------------------------------------------- Reanalyse
R_CAPACITY, SLOTS, PLAYOUTS = 40, 8, 24


def _stored_games(game):
    """Games that complete no line (a stored position is never terminal), with random pi rows and random root values."""
    from rlzero_amd.selfplay import Trajectory
    if game == 'connect4':
        games = [c4.random_game((4, 5), 20, -1, seed=400 + g, game_id=g, n_in_row=3, avoid_lines=True) for g in range(3)]
    else:
        from test_replay_reanalyse_gpu import _game
        games = [_game(6, 4, 28, seed=600 + g, game_id=g) for g in range(2)]
    rs = np.random.RandomState(8)
    return [Trajectory(t.game_id, t.board_size, t.n_in_row, t.moves, t.pis, t.winner, game=game,
                       root_values=rs.uniform(-1.0, 1.0, size=len(t.moves)).astype(np.float32)) for t in games]


def _oracle(net, game, board, n_in_row, records):
    """An independent engine given every position of ``records`` through the host set_roots, eight at a time, the same playouts ->
    (reanalysed_pi of its visit counts float32 [n, A], float32 of its root values [n])."""
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    from rlzero_amd.replay import reanalysed_pi
    from test_replay_reanalyse_gpu import _roots_of_records
    stones, to_move, last = _roots_of_records(records[0], records[1])
    n = len(to_move)
    eng = MCTSEngine(board, n_in_row, n_games=SLOTS, n_playout=PLAYOUTS, device=DEV, add_noise=False, game=game)
    ev = HipNetEvaluator(net, (board[0], board[1], board[1]) if game == 'connect4' else board, DEV, max_boards=SLOTS)
    visits, values = [], []
    for a in range(0, n, SLOTS):
        m = min(SLOTS, n - a)
        s, t, l = np.zeros((SLOTS, 2, stones.shape[2]), np.uint64), np.zeros(SLOTS, np.int32), np.full(SLOTS, -1, np.int32)
        s[:m], t[:m], l[:m] = stones[a:a + m], to_move[a:a + m], last[a:a + m]
        eng.set_roots(s, t, l, reset_trees=True)
        eng.set_active((np.arange(SLOTS) < m).astype(np.uint8))
        eng.simulate(ev, PLAYOUTS)
        visits.append(eng.root_visits()[:m].copy())
        values.append(eng.root_values()[:m, 0].copy())
    eng.check()
    eng.close()
    ev.hip.close()
    pi, written = reanalysed_pi(np.concatenate(visits))
    q = np.concatenate(values)
    assert written.all() and not np.isnan(q).any()
    return pi, q.astype(np.float32)


def _holds(dr, records, pi, q, what):
    stones, meta, got_pi, got_q = dr.read(values=True)
    assert np.array_equal(stones, records[0]) and np.array_equal(meta, records[1]), what
    assert _same(got_pi, pi), (what, np.nonzero((_bits(got_pi) != _bits(pi)).any(axis=1))[0].tolist())
    assert _same(got_q, q), (what, np.nonzero(_bits(got_q) != _bits(q))[0].tolist(), got_q, q)


def _reanalyse_scenario(game):
    import torch
    from rlzero_amd._hip import HipError
    from rlzero_amd.replay import DeviceReplay, ReplayReanalyser
    board, n_in_row = ((4, 5), 3) if game == 'connect4' else (6, 4)
    games = _stored_games(game)
    kept = sum(len(t.moves) for t in games)
    dr = DeviceReplay(board, R_CAPACITY, device=DEV, seed=SEED, game=game, search_values=True)
    for t in games:
        dr.add([t])
    count, cursor, cap = dr._state()
    assert kept > R_CAPACITY and (count, cap) == (R_CAPACITY, R_CAPACITY) and cursor % cap != 0   # wrapped: slot != index
    records = dr.read(values=True)
    net = _net(game, board, seed=3)
    want_pi, want_q = _oracle(net, game, board, n_in_row, records)
    assert not (_bits(want_q) == _bits(records[3])).any()
    pi, q = records[2].copy(), records[3].copy()

    # targets='value': 13 host indices -- one full chunk and a padded one, position 5 once in each --: q only
    ra = ReplayReanalyser(net, dr, n_in_row, PLAYOUTS, slots=SLOTS, seed=SEED, targets='value')
    marks = []
    ra.timer = marks.append
    idx = np.array([R_CAPACITY - 1, 3, 17, 5, 30, 0, 22, 9, 12, 5, 35, 1, 28])
    assert ra.reanalyse(idx) == 13 and ra.positions_done == 13
    assert marks == ['start', 'positions'] + ['roots', 'search', 'update'] * 2
    ra.timer = None
    q[idx] = want_q[idx]
    _holds(dr, records, pi, q, 'value, host indices')
    # device indices; a bad one raises and nothing is refreshed
    on_device = np.array([2, 7, 33, 5])
    assert ra.reanalyse(torch.from_numpy(on_device).to(DEV)) == 4
    q[on_device] = want_q[on_device]
    _holds(dr, records, pi, q, 'value, device indices')
    with pytest.raises(HipError):
        ra.reanalyse(torch.tensor([4, R_CAPACITY, 6], dtype=torch.int64, device=DEV))
    _holds(dr, records, pi, q, 'a bad device index')
    # the mixed target of a refreshed position, all its symmetries
    dr.set_value_mix(1.0)
    S = dr.n_symmetries
    assert _same(dr.gather(S * 5 + np.arange(S))[2].cpu().numpy(), np.repeat(want_q[5], S))
    dr.set_value_mix(0.0)
    ra.check()
    ra.close()

    # targets='both': pi and q from the same search
    both = ReplayReanalyser(net, dr, n_in_row, PLAYOUTS, slots=SLOTS, seed=SEED, targets='both')
    idx2 = np.array([4, 11, 4, 20, 39, 6, 8, 10, 13, 14])
    assert both.reanalyse(idx2) == 10
    pi[idx2], q[idx2] = want_pi[idx2], want_q[idx2]
    _holds(dr, records, pi, q, 'both')
    # other weights: after refresh_weights() both targets follow them
    late = np.arange(R_CAPACITY - 8, R_CAPACITY)
    net.load_state_dict(_net(game, board, seed=53).state_dict())
    both.refresh_weights()
    assert both.reanalyse(late) == 8
    want_pi2, want_q2 = _oracle(net, game, board, n_in_row, records)
    pi[late], q[late] = want_pi2[late], want_q2[late]
    _holds(dr, records, pi, q, 'changed weights')
    assert (_bits(want_q2[late]) != _bits(want_q[late])).any()
    both.check()
    both.close()

    # targets='pi' (the default) leaves q alone
    only_pi = ReplayReanalyser(net, dr, n_in_row, PLAYOUTS, slots=SLOTS, seed=SEED)
    assert only_pi.targets == 'pi' and only_pi.reanalyse([15, 16]) == 2
    pi[[15, 16]] = want_pi2[[15, 16]]
    _holds(dr, records, pi, q, 'pi only')
    only_pi.close()

    # the ticket: an add between position_roots and update_values, and the result has no home
    where, _, _, _, ticket = dr.position_roots([1, 2], pad_to=SLOTS)
    values = torch.full((SLOTS, 2), 0.5, dtype=torch.float64, device=DEV)
    dr.add([games[0]])
    snap = dr.read(values=True)
    with pytest.raises(HipError, match='stale ticket'):
        dr.update_values(where, values, ticket)
    for a, b in zip(dr.read(values=True), snap):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # ... and with the current ticket only the named rows change; a NaN value and the padding write nothing
    where, _, _, _, ticket = dr.position_roots([1, 2, 4], pad_to=SLOTS)
    values[1, 0] = float('nan')
    values[2, 0] = -0.123456789
    values[:, 1] = 9.0                                     # (q_best: never read)
    dr.update_values(where, values, ticket)
    now = dr.read(values=True)
    for a, b in zip(now[:3], snap[:3]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    expect = snap[3].copy()
    expect[1], expect[4] = np.float32(0.5), np.float32(np.float64(-0.123456789))
    assert _same(now[3], expect)
    with pytest.raises(ValueError):
        dr.update_values(where, values.float(), ticket)
    with pytest.raises(ValueError):
        dr.update_values(where, values, ticket, n=SLOTS + 1)
    dr.close()


@pytest.mark.parametrize('game', ['gomoku', 'connect4'])
def test_reanalyse_refreshes_q_with_a_fresh_search(game):
    _reanalyse_scenario(game)


def test_reanalyse_values_on_a_side_stream():
    import torch
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        _reanalyse_scenario('gomoku')
    side.synchronize()


def test_reanalyser_refuses_value_targets_without_values():
    from rlzero_amd.replay import ReplayReanalyser
    dr = _replay('gomoku6')
    net = _net('gomoku', 6)
    for targets in ('value', 'both'):
        with pytest.raises(ValueError, match='search values'):
            ReplayReanalyser(net, dr, 4, 16, slots=SLOTS, targets=targets)
    with pytest.raises(ValueError):
        ReplayReanalyser(net, dr, 4, 16, slots=SLOTS, targets='z')
    import torch
    with pytest.raises(ValueError):
        dr.update_values(torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros((1, 2), dtype=torch.float64, device=DEV), 0)
    dr.close()


# ----------------------------------------------------------------------------------------------- the trainer, end to end
@pytest.mark.parametrize('extra', [['--value-mix', '0.5'],
                                   ['--device-replay', '--value-mix', '0.5', '--reanalyse', '8', '--reanalyse-slots', '8', '--reanalyse-targets', 'both'],
                                   ['--game', 'connect4', '--board', '4', '--board-width', '5', '--n-in-row', '3', '--device-replay', '--value-mix', '0.5',
                                    '--reanalyse', '8', '--reanalyse-slots', '8', '--reanalyse-targets', 'both']],
                         ids=['host-buffer', 'device-replay-gomoku', 'device-replay-connect4'])
def test_trainer_end_to_end(tmp_path, monkeypatch, capsys, extra):
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    args = ['--board', '6', '--n-in-row', '4'] if '--game' not in extra else []
    rc.trainer().main(args + ['--games-in-flight', '8', '--playouts', '16', '--batches', '2', '--check-freq', '100', '--seed', '1'] + extra)
    out = capsys.readouterr().out
    lines = [ln.split(':')[0] for ln in out.splitlines() if ln.startswith(('batch i:', 'kl:'))]
    assert lines == ['batch i', 'kl', 'batch i', 'kl'], out[-2000:]


def test_trainer_refuses_several_ranks(monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(ValueError, match='one rank'):
        rc.trainer().main(['--games-in-flight', '8', '--value-mix', '0.5', '--gpus', '2'])


def test_trainer_pipeline_keeps_and_refreshes_values():
    """TrainPipeline(value_mix=, reanalyse_targets='both'): self-play hands root values to the device buffer, the sampled targets
    are mixed_value_targets of what the buffer holds, and a refresh rewrites q."""
    from rlzero_amd.replay import mixed_value_targets, replay_indices
    tr = rc.trainer()
    pipe = tr.TrainPipeline(board_size=6, n_in_row=4, n_playout=16, selfplay_games_in_flight=8, seed=5, device_replay=True, value_mix=0.5,
                            reanalyse=8, reanalyse_slots=SLOTS, reanalyse_targets='both')
    dr = pipe.data_buffer
    assert dr.search_values and dr.value_mix == 0.5
    pipe.collect_selfplay_data(8)
    stones, meta, pi, q = dr.read(values=True)
    assert len(q) > 0 and not np.isnan(q).any()
    z = (((meta >> 10) & 3) - 1).astype(np.float32)
    drawn = replay_indices(dr.seed, 0, 32, len(dr))
    zs = dr.sample(32, step=0)[2].cpu().numpy()
    assert _same(zs, np.repeat(mixed_value_targets(z, q, 0.5), 8)[drawn])
    assert pipe.reanalyse_round() == 8 and pipe._reanalyser.targets == 'both'
    after = dr.read(values=True)
    assert np.array_equal(after[1], meta) and (_bits(after[3]) != _bits(q)).any()
    pipe._reanalyser.close()
    for lane in pipe._batched.lanes:
        lane.eng.close()
    dr.close()
    with pytest.raises(ValueError, match='value_mix'):
        tr.TrainPipeline(board_size=6, n_in_row=4, n_playout=16, selfplay_games_in_flight=8, seed=5, device_replay=True, reanalyse=8,
                         reanalyse_targets='value')
