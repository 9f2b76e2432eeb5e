"""Reanalyse for the AlphaZero device replay on the GPU (rz_replay_positions, rz_replay_update_pi; rlzero_amd.replay.ReplayReanalyser;
MCTSEngine.set_roots_device / root_visits_device): stored positions searched again, their pi rows rewritten in place.

The oracle is an INDEPENDENT ``MCTSEngine`` plus ``HipNetEvaluator`` -- other objects running the same search kernels -- given the same
roots through the host ``set_roots`` (formed from a ``read()`` of the records by a Python restatement of the record-to-root rule),
then ``simulate`` and ``root_visits``; its counts go through ``reanalysed_pi`` and equality is exact.  It is computed once per
network for all 40 positions and shared by the checks.  The buffer of 40 positions is filled past its capacity, so the ring has
wrapped and slot != index; the stored pi rows are random, so a refreshed row cannot equal an old one by accident; the games avoid
a line of n stones (a stored position is never terminal) and run long enough that the late positions have fewer legal cells than the
search has simulations -- there the visit counts depend on the values, which the weight-change check needs."""
import numpy as np
import pytest
from conftest import REPO  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CAPACITY, SLOTS, SEED = 40, 8, 11


def _game(board, n_in_row, plies, seed, game_id):
    """A legal game of up to ``plies`` seeded random moves, none of which completes a line, with random pi rows over the empty cells."""
    from rlzero_amd.games.gomoku.gomoku_env import _start_masks, has_line
    from rlzero_amd.selfplay import Trajectory
    rs = np.random.RandomState(seed)
    A = board * board
    masks, bits, moves = _start_masks(board, n_in_row), [0, 0], []
    for p in range(plies):
        taken = bits[0] | bits[1]
        safe = [int(c) for c in rs.permutation(A) if not (taken >> int(c)) & 1 and not has_line(bits[p & 1] | (1 << int(c)), masks, n_in_row)]
        if not safe:
            break
        moves.append(safe[0])
        bits[p & 1] |= 1 << safe[0]
    pis = np.zeros((len(moves), A))
    for p in range(len(moves)):
        empty = np.setdiff1d(np.arange(A), moves[:p])
        pis[p, empty] = rs.dirichlet(np.full(len(empty), 0.3))
    return Trajectory(game_id, board, n_in_row, moves, pis, -1)


def _net(board, seed):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(seed)
    return PolicyValueNet(board)


def _roots_of_records(stones, meta):
    """The record-to-root rule in numpy: stones by player, side to move, last move."""
    parity = (meta >> 9) & 1
    by_player = np.where(parity[:, None, None] == 0, stones, stones[:, ::-1, :])
    return np.ascontiguousarray(by_player), parity.astype(np.int32), ((meta & 511) - 1).astype(np.int32)


def _oracle_pi(net, board, n_in_row, playouts, records):
    """reanalysed_pi of the visit counts an independent engine finds for every position of ``records`` (a ``read()``), eight at a time
    through the host ``set_roots`` -> float32 [n, A]."""
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    from rlzero_amd.replay import reanalysed_pi
    stones, to_move, last = _roots_of_records(records[0], records[1])
    n = len(to_move)
    eng = MCTSEngine(board, n_in_row, n_games=SLOTS, n_playout=playouts, device=DEV, add_noise=False)
    ev = HipNetEvaluator(net, board, DEV, max_boards=SLOTS)
    out = []
    for a in range(0, n, SLOTS):
        m = min(SLOTS, n - a)
        s, t, l = np.zeros((SLOTS, 2, stones.shape[2]), np.uint64), np.zeros(SLOTS, np.int32), np.full(SLOTS, -1, np.int32)
        s[:m], t[:m], l[:m] = stones[a:a + m], to_move[a:a + m], last[a:a + m]
        eng.set_roots(s, t, l, reset_trees=True)
        eng.set_active((np.arange(SLOTS) < m).astype(np.uint8))
        eng.simulate(ev, playouts)
        out.append(eng.root_visits()[:m].copy())
    eng.check()
    eng.close()
    ev.hip.close()
    visits = np.concatenate(out)
    pi, written = reanalysed_pi(visits)
    assert written.all()
    return pi


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _holds(dr, records, expected_pi, what):
    """The buffer holds ``records``' stones and meta words bit for bit, and ``expected_pi``."""
    stones, meta, pi = dr.read()
    assert np.array_equal(stones, records[0]) and np.array_equal(meta, records[1]), what
    differ = np.nonzero((_bits(pi) != _bits(expected_pi)).any(axis=1))[0]
    assert differ.size == 0, (what, differ.tolist())


def _scenario(board, n_in_row, playouts, weights):
    import torch
    from rlzero_amd._hip import HipError
    from rlzero_amd.replay import DeviceReplay, ReplayReanalyser, replay_reanalyse_draws
    A = board * board
    plies = 28
    games = [_game(board, n_in_row, plies, seed=100 * board + g, game_id=g) for g in range(2)]
    assert [len(t.moves) for t in games] == [plies, plies]
    dr = DeviceReplay(board, CAPACITY, device=DEV, seed=SEED)
    dr.add(games[:1])
    dr.add(games[1:])
    count, cursor, cap = dr._state()
    assert (count, cap) == (CAPACITY, CAPACITY) and cursor % cap != 0 and dr.ticket == 2 * plies   # wrapped: position 0 is not in slot 0
    records = dr.read()
    net = _net(board, seed=board)
    want = _oracle_pi(net, board, n_in_row, playouts, records)
    assert not (_bits(want) == _bits(records[2])).all(axis=1).any()
    expected = records[2].copy()
    ra = ReplayReanalyser(net, dr, n_in_row, playouts, slots=SLOTS, seed=SEED)
    marks = []
    ra.timer = marks.append

    # 13 host indices: one full chunk and a padded one, position 5 once in each
    idx = np.array([39, 3, 17, 5, 30, 0, 22, 9, 12, 5, 35, 1, 28])
    assert ra.reanalyse(idx) == 13 and ra.positions_done == 13 and ra.sims_done == 13 * playouts
    assert marks == ['start', 'positions'] + ['roots', 'search', 'update'] * 2
    expected[idx] = want[idx]
    _holds(dr, records, expected, 'host indices')
    ra.check()

    # the eight symmetries of a refreshed position share the new row
    _, pis, _ = dr.gather(8 * 5 + np.arange(8))
    pis = pis.cpu().numpy()
    for k in range(8):
        assert np.array_equal(_bits(pis[k]), _bits(want[5][dr.src_pi[k]])), k

    # indices in a device tensor: the same result; one out of range raises and nothing is refreshed
    on_device = np.array([2, 7, 33, 5])
    assert ra.reanalyse(torch.from_numpy(on_device).to(DEV)) == 4
    expected[on_device] = want[on_device]
    _holds(dr, records, expected, 'device indices')
    for bad in ([4, CAPACITY, 6], [-1], [10, 11, 12, 13, 14, 15, 16, 18, 19, 2 ** 40]):
        with pytest.raises(HipError):
            ra.reanalyse(torch.tensor(bad, dtype=torch.int64, device=DEV))
        _holds(dr, records, expected, 'a bad device index')
    with pytest.raises(HipError):
        ra.reanalyse([0, CAPACITY])                                # (host indices: refused before the launch)
    _holds(dr, records, expected, 'a bad host index')

    # positions drawn on the device: exactly those the restatement names
    draws = replay_reanalyse_draws(SEED, 3, 10, CAPACITY)
    fresh = sorted(set(draws.tolist()) - set(idx.tolist()) - set(on_device.tolist()))
    assert fresh                                                   # (some of them were not refreshed before)
    assert ra.reanalyse_sample(10, step=3) == 10
    expected[draws] = want[draws]
    _holds(dr, records, expected, 'drawn positions')
    assert ra.step == 0 and ra.reanalyse_sample(3) == 3 and ra.step == 1   # the internal counter: refresh 0
    first = replay_reanalyse_draws(SEED, 0, 3, CAPACITY)
    expected[first] = want[first]
    _holds(dr, records, expected, 'the internal counter')

    # everything
    assert ra.reanalyse_all() == CAPACITY
    _holds(dr, records, want, 'all positions')

    if weights:
        # the network changes in place: a refresh after refresh_weights() is the oracle's on the changed module, and differs
        late = np.arange(CAPACITY - 8, CAPACITY)                   # the last plies of the second game: 16 .. 9 empty cells
        if playouts > A - (plies - 8):
            states = torch.from_numpy(np.asarray(games[1].states()[plies - 8:], dtype=np.float32))
            with torch.no_grad():
                _, v_old = net(states)
                net.val_fc2.weight.mul_(-8.0)                       # the value head's last layer: every value's pre-activation turns over
                _, v_new = net(states)
            assert float((v_new - v_old).abs().max()) > 0.05       # (far above a tie of two children's W / N)
        ra.refresh_weights()
        assert ra.reanalyse(late) == 8
        want2 = _oracle_pi(net, board, n_in_row, playouts, records)
        expected = want.copy()
        expected[late] = want2[late]
        _holds(dr, records, expected, 'changed weights')
        assert (_bits(want2[late]) != _bits(want[late])).any()

    # the ticket: an add between positions and update_pi, and the result has no home
    where, _, _, _, ticket = dr.position_roots([1, 2], pad_to=SLOTS)
    assert ticket == dr.ticket and where.shape == (SLOTS, ) and (where[2:] == -1).all().item() and (where[:2] >= 0).all().item()
    visits = torch.ones((SLOTS, A), dtype=torch.int32, device=DEV)
    dr.add([_game(board, n_in_row, 3, seed=5, game_id=9)])
    assert dr.ticket == ticket + 3
    snap = dr.read()
    with pytest.raises(HipError, match='stale ticket'):
        dr.update_pi(where, visits, ticket)
    for a, b in zip(dr.read(), snap):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # ... and with the current ticket only the named rows change, a row of zero counts and the padding write nothing
    where, _, _, _, ticket = dr.position_roots([1, 2, 4], pad_to=SLOTS)
    visits[1] = 0
    visits[2, :3] = torch.tensor([-7, 3, 1], dtype=torch.int32)
    dr.update_pi(where, visits, ticket)
    now = dr.read()
    assert np.array_equal(now[0], snap[0]) and np.array_equal(now[1], snap[1])
    rows = np.array([1, 4])
    uniform = np.full(A, np.float32(1.0 / A))
    spiked = uniform.copy()
    spiked[:3] = [0.0, np.float32(3.0 / (A + 1)), np.float32(1.0 / (A + 1))]
    spiked[3:] = np.float32(1.0 / (A + 1))
    assert np.array_equal(_bits(now[2][1]), _bits(uniform)) and np.array_equal(_bits(now[2][4]), _bits(spiked))
    others = np.setdiff1d(np.arange(CAPACITY), rows)
    assert np.array_equal(_bits(now[2][others]), _bits(snap[2][others]))
    with pytest.raises(ValueError):
        dr.update_pi(where, visits[:, :A - 1].contiguous(), ticket)
    with pytest.raises(ValueError):
        dr.update_pi(where, visits, ticket, n=SLOTS + 1)
    ra.check()
    ra.close()
    dr.close()


@pytest.mark.parametrize('board, n_in_row, playouts, weights', [(6, 4, 24, True), (11, 5, 24, False), (16, 5, 16, False)])
def test_reanalyse_is_a_fresh_search_of_the_stored_position(board, n_in_row, playouts, weights):
    """6 x 6 (the resident k_trunk_split route; the late positions have fewer empty cells than simulations, so the weight change
    shows), 11 x 11 and 16 x 16 (k_delta_res; four mask words, last moves up to cell 255)."""
    _scenario(board, n_in_row, playouts, weights)


def test_the_whole_sequence_on_a_side_stream():
    """Everything above ordered on a side stream, with the default stream idle: no launch or copy leans on the default stream."""
    import torch
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        _scenario(6, 4, 24, True)
    side.synchronize()


def test_engine_device_roots_are_the_host_roots():
    """set_roots_device / root_visits_device against set_roots / root_visits on a second engine: the same counts; wrong tensors are
    refused before anything is launched."""
    import torch
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    from rlzero_amd.replay import pack_positions
    board, n_in_row, playouts = 6, 4, 24
    game = _game(board, n_in_row, 28, seed=3, game_id=0)
    records = pack_positions([game], board)
    stones, to_move, last = _roots_of_records(records[0][-SLOTS:], records[1][-SLOTS:])
    net = _net(board, seed=2)
    got = []
    for on_device in (False, True):
        eng = MCTSEngine(board, n_in_row, n_games=SLOTS, n_playout=playouts, device=DEV, add_noise=False)
        ev = HipNetEvaluator(net, board, DEV, max_boards=SLOTS)
        if on_device:
            d = [torch.from_numpy(stones.view(np.int64)).to(DEV), torch.from_numpy(to_move).to(DEV), torch.from_numpy(last).to(DEV)]
            for bad in ((d[0][:4], d[1], d[2]), (d[0], d[1].long(), d[2]), (d[0].cpu(), d[1], d[2]), (d[0], d[1], d[2][::2])):
                with pytest.raises(ValueError):
                    eng.set_roots_device(*bad)
            epoch = eng.roots_epoch
            eng.set_roots_device(*d, reset_trees=True)
            assert eng.roots_epoch == epoch + 1
            eng.simulate(ev, playouts)
            vis = eng.root_visits_device()
            assert vis.is_cuda and vis.dtype == torch.int32 and tuple(vis.shape) == (SLOTS, board * board)
            got.append(vis.cpu().numpy().copy())
            roots = eng.get_roots()
            assert np.array_equal(roots[0], stones) and np.array_equal(roots[1], to_move) and np.array_equal(roots[2], last)
        else:
            eng.set_roots(stones, to_move, last, reset_trees=True)
            eng.simulate(ev, playouts)
            got.append(eng.root_visits().copy())
        eng.check()
        eng.close()
        ev.hip.close()
    assert np.array_equal(got[0], got[1]) and (got[0].sum(axis=1) > 0).all()


def test_the_trainer_refreshes_before_its_updates():
    """TrainPipeline(reanalyse=N): off until asked, then ``reanalyse_round`` -- what ``run`` calls on rank 0 between a round's
    collection and its updates -- refreshes exactly the drawn positions of the pipeline's device buffer with the agent's network."""
    import replay_cases as rc
    from rlzero_amd.replay import replay_reanalyse_draws
    tr = rc.trainer()
    board, n_in_row, playouts = 6, 4, 16
    pipe = tr.TrainPipeline(board_size=board, n_in_row=n_in_row, n_playout=playouts, selfplay_games_in_flight=16, seed=5, device_replay=True,
                            reanalyse=6, reanalyse_slots=SLOTS)
    assert pipe._reanalyser is None and pipe.reanalyse_playouts == playouts and pipe.reanalyse_round() == 0   # (an empty buffer: nothing yet)
    dr = pipe.data_buffer
    dr.add([_game(board, n_in_row, 28, seed=70 + g, game_id=g) for g in range(2)])
    before = dr.read()
    assert pipe.reanalyse_round() == 6 and pipe._reanalyser.positions_done == 6
    after = dr.read()
    drawn = replay_reanalyse_draws(pipe.selfplay_seed, 0, 6, dr.positions)
    changed = np.nonzero((_bits(after[2]) != _bits(before[2])).any(axis=1))[0]
    assert sorted(set(drawn.tolist())) == changed.tolist()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    want = _oracle_pi(pipe.alphazero_agent.policy_value_net, board, n_in_row, playouts, before)
    assert np.array_equal(_bits(after[2][changed]), _bits(want[changed]))
    pipe.reanalyse = 'all'
    assert pipe.reanalyse_round() == dr.positions
    assert np.array_equal(_bits(dr.read()[2]), _bits(want))
    pipe._reanalyser.close()
    dr.close()
