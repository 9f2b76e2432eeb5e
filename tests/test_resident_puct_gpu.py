"""The resident search under PUCT (rz_net_search_resident_puct; HipNetEvaluator.resident_puct, an opt-in route): one launch per search
on boards of up to 10 rows and columns, one game per CU.

(a) against the three-launch PUCT step (trunk -> FC GEMM -> k_tree_step_raw) of a twin engine and evaluator with the same weights, roots
    and noise seeds: every record of every game's arena -- N, W, child blocks, prior blocks, every stored prior -- the tree dumps, root
    visits, root priors and root statistics, bit for bit, one board per way k_trunk_split covers a board (trunk_class);
(b) against the oracle's PUCT search fed, leaf by leaf, what a one-game probe of the DEFAULT route computes for that position;
(c) whole games: run and run_device (whole-move hipGraphs) with the switch on play the games of the same calls with it off;
(d) the refusals of the new entry point, and those that must stay: rz_net_search_resident, set_playouts, the cap, matches.

The nets are sharpened (act_fc1.weight x 20) so that the priors shape the search, and the tests assert that they do.  Every test builds
its evaluator with resident_puct=True: on a tree without the route each fails at that attribute, the constructor or the entry point."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
C_PUCT = 3.0
# name: (game, board, n_in_row, simulations, openings of game 0 / 1 / 2 as moves played from the empty board -- equal lengths; game 0's
# leaves a win in one for the player to move (terminal leaves at depth 1 and, where the opponent can answer, 2), none is finished)
CASES = {
    'ttt3': ('gomoku', 3, 3, 40, ([0, 3, 1, 4], [4, 0, 8, 2], [0, 4, 8, 1])),
    'connect4': ('connect4', (6, 7), 4, 80, ([0, 1, 0, 1, 0, 1], [3, 3, 2, 4, 2, 4], [3, 2, 3, 4, 0, 6])),
    'gomoku9': ('gomoku', 9, 5, 120, ([0, 9, 1, 10, 2, 11, 3, 12], [40, 41, 31, 32, 49, 50, 22, 13], [40, 30, 41, 31, 50, 20, 60, 61])),
    'gomoku10': ('gomoku', 10, 5, 120, ([0, 10, 1, 11, 2, 12, 3, 13], [44, 45, 54, 55, 34, 35, 64, 24], [44, 33, 45, 34, 56, 22, 67, 68])),
    'gomoku6': ('gomoku', 6, 4, 80, ([0, 6, 1, 7, 2, 8], [14, 15, 20, 21, 8, 9], [14, 21, 15, 20, 9, 28])),
}


@pytest.fixture(scope='module', autouse=True)
def _stream_pool_left_as_found():
    """torch hands out its pooled streams in a cycle, and which of the few hardware queues a stream sits on decides how the lanes of
    a LATER test overlap (tests/test_trace.py measures exactly that).  This module draws streams -- the side stream, warm_graph's --
    so it puts the cycle back where it found it: the tests behind it get the streams they get without it."""
    import torch
    cycle, seen = [], set()
    while True:   # one whole cycle and one more: the draw that repeats is cycle[0] again
        handle = torch.cuda.Stream(device=DEV).cuda_stream
        if handle in seen:
            break
        seen.add(handle)
        cycle.append(handle)
    assert handle == cycle[0]
    yield
    for _ in range(2 * len(cycle)):   # until the stream BEFORE cycle[0] has been drawn: the next draw is cycle[0], as it was
        if torch.cuda.Stream(device=DEV).cuda_stream == cycle[-1]:
            break
    else:
        raise AssertionError('the stream pool did not come round')


def _shape(case):
    game, board = CASES[case][:2]
    return (board[0], board[1]) if game == 'connect4' else (board, board)


def _trunk_ms(rows, cols):
    """rz_net.hip's trunk_class: how k_trunk_split covers a board -- 4: one N-tile, 2: two, 3: three tiles of 3 rows, 1: four, 0: more."""
    tile_rows = min(32 // cols, 16)
    tiles = -(-rows // tile_rows)
    return 4 if tiles <= 1 else 2 if tiles <= 2 else 3 if (tiles == 3 and tile_rows == 3) else 1 if tiles <= 4 else 0


# one board per class of TN = 1 (6 x 6 shares Connect4's: it is searched in (b) and (c))
CLASS_BOARDS = ['ttt3', 'connect4', 'gomoku9', 'gomoku10']


def test_the_boards_cover_every_class_of_one_tile_per_wave():
    assert sorted(_trunk_ms(*_shape(c)) for c in CLASS_BOARDS) == [1, 2, 3, 4]
    assert _trunk_ms(*_shape('gomoku6')) == _trunk_ms(*_shape('connect4'))


def _net(case, seed=4):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    rows, cols = _shape(case)
    torch.manual_seed(seed)
    net = PolicyValueNet(rows, cols, cols) if CASES[case][0] == 'connect4' else PolicyValueNet(rows)
    with torch.no_grad():   # away from the near-uniform initial policy
        net.act_fc1.weight.mul_(20.0)
    return net


def _engine(case, n_games, **kw):
    from rlzero_amd.engine import MCTSEngine
    game, board, n_in_row, sims = CASES[case][:4]
    kw.setdefault('n_playout', sims)
    kw.setdefault('score_mode', 'puct')
    kw.setdefault('c_puct', C_PUCT)
    return MCTSEngine(board, n_in_row, n_games=n_games, game=game, device=DEV, **kw)


def _evaluator(case, net, resident_puct, max_boards=8):
    from rlzero_amd.engine import HipNetEvaluator
    rows, cols = _shape(case)
    acts = cols if CASES[case][0] == 'connect4' else rows * cols
    ev = HipNetEvaluator(net, (rows, cols, acts), DEV, max_boards=max_boards)
    ev.resident_puct = resident_puct
    return ev


def _twins(case, net, **kw):
    """-> [(engine, evaluator)] x 2: the resident PUCT route first, the three-launch step second; three games, the middle one idle."""
    out = []
    for resident in (True, False):
        ev = _evaluator(case, net, resident)
        eng = _engine(case, 3, **kw)
        assert ev.resident_ok(eng) is resident and not ev.deferred_ok(eng) and (not resident or ev.resident_per_cu(eng) == 1)
        out.append((eng, ev))
    return out


def _open(eng, case, crafted):
    eng.reset_games()
    if crafted:
        openings = CASES[case][4]
        for ply in range(len(openings[0])):
            moves = np.array([o[ply] for o in openings], dtype=np.int32)
            eng.advance(moves)   # (nothing searched yet: a fresh root each time)
            _, ended = eng.step(moves)
            assert not ended.any()
    eng.set_noise_keys()
    eng.set_active([1, 0, 1])


def _snapshot(eng):
    rn, rw = eng.root_stats()
    snap = {'visits': eng.root_visits().copy(), 'priors': eng.root_priors().view(np.uint32).copy(), 'root_n': rn.copy(),
            'root_w': rw.view(np.uint64).copy()}
    for g in range(eng.n_games):
        ar = eng.arena(g)
        for k, v in ar.items():   # EVERY record and prior of the arena, visited or not
            snap['arena%d.%s' % (g, k)] = np.asarray(v).copy().view(np.uint8) if isinstance(v, np.ndarray) else np.float32(v).view(np.uint32)
        snap['tree%d' % g] = {p: (n, float(w).hex()) for p, (n, w) in eng.tree_dump(g).items()}
    return snap


def _assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            assert a[k] == b[k], (tag, k)
        else:
            assert np.array_equal(a[k], b[k]), (tag, k)


def _legal_root_visits(eng, g):
    stones, _, _ = eng.get_roots()
    from rlzero_amd.engine import bits_to_int
    occ = bits_to_int(stones[g, 0]) | bits_to_int(stones[g, 1])
    visits = eng.root_visits()[g]
    return [int(visits[a]) for a in eng.legal_actions(occ)]


def _assert_priors_shape_the_search(eng, games=(0, 2)):
    for g in games:
        v = _legal_root_visits(eng, g)
        assert max(v) > 3 * max(1, min(v)), (g, v)


def _close(pairs):
    for eng, ev in pairs:
        eng.check()
        ev.hip.check_flags()
        eng.close()
        ev.hip.close()


# ------------------------------------------------------------------------------------------------ (a) the three-launch step
@pytest.mark.parametrize('case', CLASS_BOARDS)
@pytest.mark.parametrize('crafted', [False, True])
def test_one_search_equals_the_three_launch_step(case, crafted):
    """Fresh roots, and crafted ones (game 0: a win in one for the mover -- terminal leaves within two plies): one search."""
    sims = CASES[case][3]
    pairs = _twins(case, _net(case))
    snaps = []
    for eng, ev in pairs:
        _open(eng, case, crafted)
        eng.simulate(ev, sims)
        snaps.append(_snapshot(eng))
    _assert_same(snaps[0], snaps[1], (case, crafted))
    res = pairs[0][0]
    assert (snaps[0]['root_n'][[0, 2]] == sims).all() and snaps[0]['root_n'][1] == 0   # (the idle game was not searched)
    if not crafted:
        _assert_priors_shape_the_search(res)
    else:
        terminal = [p for p, (n, _) in snaps[0]['tree0'].items() if len(p) in (1, 2) and n > 0 and p not in
                    {q[:len(p)] for q in snaps[0]['tree0'] if len(q) > len(p)}]
        assert terminal   # (leaves at depth 1 or 2 that were visited and never expanded further)
    _close(pairs)


@pytest.mark.parametrize('case', CLASS_BOARDS)
@pytest.mark.parametrize('noise', [False, True])
def test_four_moves_with_tree_reuse(case, noise):
    """Four moves, update_with_move between the searches; with Dirichlet noise the kept subtrees' priors and the counters the later
    expansions draw with must go on alike -- a counter that differed would move every later prior."""
    sims = CASES[case][3]
    pairs = _twins(case, _net(case), add_noise=noise, noise_seed=4)
    records = []
    for eng, ev in pairs:
        _open(eng, case, False)
        rec = []
        for move in range(4):
            eng.simulate(ev, sims)
            rec.append(_snapshot(eng))
            best = rec[-1]['visits'].argmax(axis=1).astype(np.int32)
            keep = np.where([1, 0, 1], best, -2).astype(np.int32)
            eng.advance(keep)
            _, ended = eng.step(np.where([1, 0, 1], best, -1).astype(np.int32))
            if ended.any():
                break
        records.append(rec)
    assert len(records[0]) == len(records[1]) >= 3
    for move, (x, y) in enumerate(zip(*records)):
        _assert_same(x, y, (case, noise, move))
    if noise:   # the noise is in the stored priors (a twin without it stores others)
        plain = _twins(case, _net(case))
        _open(plain[0][0], case, False)
        plain[0][0].simulate(plain[0][1], sims)
        assert not np.array_equal(plain[0][0].root_priors().view(np.uint32), records[0][0]['priors'])
        _close(plain)
    _close(pairs)


@pytest.mark.parametrize('case', CLASS_BOARDS)
def test_a_search_in_two_launches(case):
    """n1 + n2 simulations: the second launch continues (select_first false, its first leaf from rz_select_step before it)."""
    from rlzero_amd._hip import check
    sims = CASES[case][3]
    n1 = sims // 3
    (eng, ev), (eng3, ev3) = pairs = _twins(case, _net(case))
    _open(eng, case, True)
    eng.sim_chunk(ev, n1)
    check(eng.lib.rz_select_step(eng.handle, None, eng.stream()), 'rz_select_step')
    ev.search_resident(eng, sims - n1, False)
    _open(eng3, case, True)
    eng3.simulate(ev3, sims)
    _assert_same(_snapshot(eng), _snapshot(eng3), case)
    _close(pairs)


@pytest.mark.parametrize('case', CLASS_BOARDS)
def test_after_a_weight_reload_and_on_a_side_stream(case):
    """refresh() with changed weights moves both routes alike (and moves them); then the resident search on a stream of its own."""
    import torch
    sims = CASES[case][3]
    net = _net(case)
    pairs = _twins(case, net)
    before = []
    for eng, ev in pairs:
        _open(eng, case, False)
        eng.simulate(ev, sims)
        before.append(_snapshot(eng))
    _assert_same(before[0], before[1], (case, 'before'))
    with torch.no_grad():
        net.conv2.weight.mul_(1.25)
        net.act_fc1.bias.add_(0.5 * torch.randn_like(net.act_fc1.bias))
    side = torch.cuda.Stream(device=DEV)
    after = []
    for i, (eng, ev) in enumerate(pairs):
        ev.refresh()
        _open(eng, case, False)
        if i == 0:
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                eng.simulate(ev, sims)
            side.synchronize()
        else:
            eng.simulate(ev, sims)
        after.append(_snapshot(eng))
    _assert_same(after[0], after[1], (case, 'after'))
    assert not np.array_equal(after[0]['priors'], before[0]['priors'])
    _close(pairs)


# ------------------------------------------------------------------------------------------------ (b) the oracle
@pytest.mark.parametrize('case', ['gomoku6', 'connect4'])
def test_against_the_oracle_fed_by_a_one_game_probe(case):
    """RefSearch(score_mode='puct') fed, leaf by leaf, the priors and value a one-game probe on the DEFAULT route (uct_ref engine,
    three-launch step: nothing of the resident PUCT kernel) computes for that position."""
    from oracle.connect4_ref import RefConnect4
    from oracle.gomoku_ref import RefGomoku
    from oracle.mcts_ref import RefSearch, tree_dump
    from rlzero_amd.engine import int_to_bits
    game, board, n_in_row, sims, openings = CASES[case]
    net = _net(case).to(DEV)
    probe_ev = _evaluator(case, net, False)
    probe_ev.deferred_priors = False
    probe = _engine(case, 1, n_playout=2, score_mode='uct_ref', c_puct=5.0)

    def set_roots(eng, envs):
        stones = np.array([[int_to_bits(e.bitboards()[0]), int_to_bits(e.bitboards()[1])] for e in envs], dtype=np.uint64)
        eng.set_roots(stones, [e.current_player() for e in envs], [getattr(e, 'last_cell', e.last_move) for e in envs], reset_trees=True)

    def pvf(env):
        set_roots(probe, [env])
        probe.sim_chunk(probe_ev, 1)
        pri = probe.root_priors()[0]
        _, rw = probe.root_stats()
        return [(a, pri[a]) for a in env.leagel_actions()], -float(rw[0])

    pre = openings[2][:2]
    env = RefConnect4.from_moves(pre) if game == 'connect4' else RefGomoku.from_moves(board, n_in_row, pre)
    empty = RefConnect4() if game == 'connect4' else RefGomoku(board, n_in_row)
    ev = _evaluator(case, net, True)
    eng = _engine(case, 3)
    assert ev.resident_ok(eng)
    set_roots(eng, [env, empty, env])
    eng.simulate(ev, sims)
    eng.check()
    s = RefSearch(pvf, sims, C_PUCT, score_mode='puct')
    acts, _ = s.simulate(env, 1.0)
    want = {p: (n, float(w).hex()) for p, (n, w) in tree_dump(s.root).items()}
    for g in (0, 2):
        visits, pri = eng.root_visits()[g], eng.root_priors()[g]
        assert [int(visits[a]) for a in acts] == [k.n for k in s.root.kids]
        assert [float(pri[a]) for a in acts] == [float(k.p) for k in s.root.kids]
        assert {p: (n, float(w).hex()) for p, (n, w) in eng.tree_dump(g).items()} == want
    assert max(k.n for k in s.root.kids) > 3 * max(1, min(k.n for k in s.root.kids))   # the priors shape the search
    eng.close()
    probe.close()
    ev.hip.close()
    probe_ev.hip.close()


# ------------------------------------------------------------------------------------------------ (c) whole games
def _selfplay(case, resident_puct, **extra):
    from rlzero_amd.selfplay import BatchedSelfPlay
    game, board, n_in_row = CASES[case][:3]
    kw = dict(game='connect4', net_shape=(board[0], board[1], board[1])) if game == 'connect4' else {}
    kw.update(extra)
    return BatchedSelfPlay.for_network(_net(case), board, n_in_row, n_games=6, n_playout=40, c_puct=C_PUCT, lanes=1, device=DEV,
                                       temperature=1.0, seed=11, score_mode='puct', resident_puct=resident_puct, **kw)


def _same_games(a, b, tag):
    assert [t.game_id for t in a] == [t.game_id for t in b], tag
    for x, y in zip(a, b):
        assert (x.winner, list(x.moves)) == (y.winner, list(y.moves)), (tag, x.game_id)
        assert np.array_equal(np.asarray(x.pis).view(np.uint64), np.asarray(y.pis).view(np.uint64)), (tag, x.game_id)


@pytest.mark.parametrize('case', ['connect4', 'gomoku6'])
def test_selfplay_plays_the_games_of_the_three_launch_step(case):
    """12 games in 6 slots, Dirichlet noise on: run and run_device with the switch on against the same calls with it off; the
    device loop replays one whole-move hipGraph per move; a stalled slot changes nothing."""
    ids = list(range(12))
    off = _selfplay(case, False)
    want_host, want_dev = off.run(ids), off.run_device(ids)
    assert not off.lanes[0].evaluator.resident_ok(off.lanes[0].eng) and off.lanes[0].move_graph is None
    on = _selfplay(case, True)
    lane = on.lanes[0]
    assert lane.evaluator.resident_puct and lane.evaluator.resident_ok(lane.eng)
    _same_games(on.run(ids), want_host, (case, 'run'))
    sims0 = on.sims_done
    _same_games(on.run_device(ids), want_dev, (case, 'run_device'))
    assert lane.move_graph is not None and lane.eng._def_pending == 0
    assert on.sims_done - sims0 == 40 * sum(len(t.moves) for t in want_dev)
    _same_games(want_host, want_dev, (case, 'loops'))
    on.device_attach(queue_capacity=len(ids), stall_margin=0.2)
    _same_games(on.run_device(ids), want_dev, (case, 'stalls'))
    assert on.stalls_resolved > 0 and lane.move_graph is not None
    for sp in (on, off):
        sp.check()
        for ln in sp.lanes:
            ln.eng.close()


def test_one_game_player_passes_the_switch_through():
    """AlphaZeroPlayer(score_mode='puct', resident_puct=True): the one-game engine searches resident, with the move probabilities of the
    three-launch player over four moves with tree reuse; a board the route cannot serve is a ValueError at the first search."""
    from rlzero_amd.games.gomoku.gomoku_env import GomokuEnv
    from rlzero_amd.mcts import AlphaZeroPlayer
    seen = {}
    for resident in (True, False):
        agent = _agent(6)
        player = AlphaZeroPlayer(agent.policy_value_fn, n_playout=40, c_puct=C_PUCT, score_mode='puct', resident_puct=resident)
        env = GomokuEnv(6, 4)
        env.reset()
        rec = []
        for _ in range(4):
            acts, probs = player.mcts.simulate(env, 1.0)
            move = int(acts[int(np.argmax(probs))])
            rec.append((tuple(int(a) for a in acts), np.asarray(probs, dtype=np.float64).tobytes(), move))
            env.step(move)
            player.mcts.update_with_move(move)
        ev, eng = player.mcts._evaluator, player.mcts._engine
        assert ev.resident_puct is resident and ev.resident_ok(eng) is resident
        seen[resident] = rec
        eng.close()
    assert seen[True] == seen[False]
    agent = _agent(11)
    player = AlphaZeroPlayer(agent.policy_value_fn, n_playout=8, score_mode='puct', resident_puct=True)
    env = GomokuEnv(11, 5)
    env.reset()
    with pytest.raises(ValueError, match='resident_puct=True cannot be served: a board of 11 x 11'):
        player.get_action(env)


def _agent(board):
    import torch
    from rlzero_amd.games.gomoku.alphazero_agent import AlphaZeroAgent
    torch.manual_seed(2)
    agent = AlphaZeroAgent(board, device=DEV)
    with torch.no_grad():
        agent.policy_value_net.act_fc1.weight.mul_(20.0)
    return agent


# ------------------------------------------------------------------------------------------------ (d) refusals
def _refused(ev, eng, words, n_sims=4):
    from rlzero_amd._hip import HipError
    with pytest.raises(HipError) as err:
        ev.hip.search_resident_puct(eng, n_sims, True)
    assert 'rz_net_search_resident_puct' in str(err.value) and words in str(err.value), str(err.value)


def test_the_entry_point_refuses_what_it_cannot_serve():
    import torch
    from rlzero_amd._hip import HipError, check
    net = _net('gomoku6')
    ev = _evaluator('gomoku6', net, True, max_boards=2)
    n_cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    # the engine: not PUCT; more than one simulation in flight
    for kw, words in ((dict(score_mode='uct_ref'), 'RZ_SCORE_PUCT and one simulation in flight'),
                      (dict(sims_in_flight=2), 'RZ_SCORE_PUCT and one simulation in flight')):
        eng = _engine('gomoku6', 2, **kw)
        eng.reset_games()
        r = ev.route(eng)
        assert not r.resident or r.deferred   # (uct_ref keeps the resident search of the deferred route: rz_net_search_resident's)
        _refused(ev, eng, words)
        eng.close()
    eng = _engine('gomoku6', 2)
    eng.reset_games()
    _refused(ev, eng, 'n_sims must be positive', n_sims=0)
    # the net: no split-f16 trunk; the f32 FC GEMM
    ev.hip.set_algo('direct')
    assert not ev.resident_ok(eng)
    _refused(ev, eng, 'RZ_NET_SPLIT_F16 trunk')
    ev.hip.set_algo('split_f16')
    ev.hip.set_heads_algo('f32')
    assert not ev.resident_ok(eng)
    _refused(ev, eng, 'RZ_NET_HEADS_F32')
    ev.hip.set_heads_algo('auto')
    assert ev.resident_ok(eng)
    # more games than reserved: the library's own check (the Python wrapper reserves before it calls)
    eng3 = _engine('gomoku6', 3)
    eng3.reset_games()
    assert ev.hip.max_boards == 2
    with pytest.raises(HipError, match='more games than rz_net_reserve'):
        check(ev.hip.lib.rz_net_search_resident_puct(ev.hip.handle, eng3.handle, 4, 1, ev.hip._stream()), 'rz_net_search_resident_puct')
    eng3.close()
    # another board than the net's
    eng9 = _engine('gomoku9', 2)
    eng9.reset_games()
    assert not ev.resident_ok(eng9)
    _refused(ev, eng9, 'disagree on the board')
    eng9.close()
    # more games than CUs
    big = _engine('gomoku6', n_cus + 1, n_playout=4)
    big.reset_games()
    assert not ev.resident_ok(big)
    _refused(ev, big, 'one per CU')
    big.close()
    # rz_net_search_resident keeps refusing PUCT, whatever the switch says
    with pytest.raises(HipError, match='rz_net_search_resident failed'):
        ev.hip.search_resident(eng, 4, True)
    # ... and nothing above has touched the engine's tree or left an error behind
    eng.simulate(ev, 20)
    assert (eng.root_stats()[0] == 20).all()
    eng.check()
    eng.close()
    ev.hip.close()
    # a board of 11 rows
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    ev11 = HipNetEvaluator(PolicyValueNet(11), 11, DEV, max_boards=2)
    ev11.resident_puct = True
    eng11 = MCTSEngine(11, 5, n_games=2, n_playout=8, score_mode='puct', device=DEV)
    eng11.reset_games()
    assert not ev11.resident_ok(eng11)
    _refused(ev11, eng11, 'up to 10 x 10')
    eng11.simulate(ev11, 8)   # (the switch on an evaluator the route cannot serve: the three-launch step, as route() says)
    eng11.check()
    eng11.close()
    ev11.hip.close()


def test_what_stays_refused_under_puct():
    """The default evaluator has no resident PUCT search; per-game simulation counts, the playout cap and matches keep refusing the rule,
    with the switch on too."""
    from rlzero_amd._hip import HipError
    net = _net('gomoku6')
    eng = _engine('gomoku6', 2)
    default = _evaluator('gomoku6', net, False)
    assert default.resident_ok(eng) is False and type(default).resident_puct is False
    default.hip.close()
    with pytest.raises(ValueError, match='uct_ref'):
        eng.set_playouts(np.array([4, 8], dtype=np.int32))
    eng.close()
    sp = _selfplay('gomoku6', True, add_noise=False)
    with pytest.raises(ValueError, match='playout cap'):
        sp.set_playout_cap(10, 0.5)
    sp.device_attach(queue_capacity=8)
    lane_eng = sp.lanes[0].eng
    with pytest.raises(ValueError, match='playout cap'):
        lane_eng.play_set_cap(10, 0.5)
    from rlzero_amd.engine import WORDS
    with pytest.raises(HipError, match='matches need the resident search'):
        lane_eng.play_set_match((np.zeros((1, 2, WORDS), np.uint64), [0], [-1]))
    lane_eng.close()
    from rlzero_amd.selfplay import BatchedSelfPlay
    with pytest.raises(ValueError, match='resident_puct=True cannot be served'):
        BatchedSelfPlay.for_network(_net('gomoku6'), 6, 4, n_games=6, n_playout=8, lanes=1, device=DEV, score_mode='uct_ref', resident_puct=True)
