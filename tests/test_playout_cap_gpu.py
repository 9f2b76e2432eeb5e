"""Playout cap randomization on the device (rz_set_playouts, rz_play_set_cap; MCTSEngine.set_playouts, BatchedSelfPlay.set_playout_cap):
a game searched with its own simulation count ends with the tree of a uniform search of that count -- bit for bit, in all three
resident kernels, and the oracle's --, the workgroup order changes nothing, the device's partition is stable, both self-play loops
play the same games with the same budget flags, p_full = 1 is the game without a cap, a captured move graph takes new values, and
the trainer's option runs."""
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import REPO

import test_production_routes as tpr   # (its helpers: roots from oracle positions, the probe that feeds the oracle the device's values)
from oracle.connect4_ref import RefConnect4
from oracle.gomoku_ref import RefGomoku
from oracle.mcts_ref import RefSearch, tree_dump

pytestmark = pytest.mark.gpu

SEED = 13
PATTERN = [1, 2, 3, 7, 12]

KERNELS = {   # id -> (game, shape, n_in_row, receptive-field trunk)
    'k_delta_res_15x15': ('gomoku', 15, 5, True),
    'k_trunk_rows_res_15x15': ('gomoku', 15, 5, False),
    'k_trunk_split_res_6x6': ('gomoku', 6, 4, True),
    'k_trunk_split_res_connect4': ('connect4', (6, 7), 4, True),
}


def _net(game, shape):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(4)
    if game == 'connect4':
        return PolicyValueNet(6, 7, 7).to('cuda:0'), (6, 7, 7)
    return PolicyValueNet(shape).to('cuda:0'), shape


def _roots(game, shape, n_row, count, seed):
    """``count`` distinct positions of two to five stones."""
    rs, envs, seen = np.random.RandomState(seed), [], set()
    while len(envs) < count:
        if game == 'connect4':
            env = RefConnect4.from_moves(rs.randint(0, shape[1], size=rs.randint(2, 6)).tolist(), shape[0], shape[1], n_row)
        else:
            env = RefGomoku.from_moves(shape, n_row, rs.permutation(shape * shape)[:rs.randint(2, 6)].tolist())
        key = (env.bitboards(), env.current_player())
        if key not in seen and not env.game_end_winner()[0]:
            seen.add(key)
            envs.append(env)
    return envs


def _engine(game, shape, n_row, n_games, n_playout, net, net_shape, delta=True):
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
    ev = HipNetEvaluator(net, net_shape, 'cuda:0', max_boards=n_games)
    ev.delta_trunk = delta
    eng = MCTSEngine(shape, n_row, n_games=n_games, n_playout=n_playout, device='cuda:0', game=game, add_noise=False)
    assert ev.resident_ok(eng)
    return eng, ev


def _state(eng, g):
    """What a search leaves of game g: the visited nodes' N and W (fp64 bits) and the arena's priors."""
    a = eng.arena(g)
    # the children counts of the records IN USE, breadth first from the root: a node's child vector grows 4, 8, 16 ... and its
    # records beyond the visited ones (NV) are capacity that holds whatever an earlier search of the arena left there
    used, at = [0], 0
    while at < len(used):
        s = used[at]
        at += 1
        if a['FC'][s] >= 0:
            used.extend(range(int(a['FC'][s]), int(a['FC'][s]) + int(a['NV'][s])))
    return tpr._hex_tree(eng.tree_dump(g)), a['PRI'].tobytes(), [(s, int(a['K'][s]), int(a['PB'][s]) if a['K'][s] else -1) for s in used]


def _close(*things):
    for x in things:
        getattr(x, 'hip', x).close()


@pytest.mark.parametrize('kernel', sorted(KERNELS))
def test_per_game_counts_are_the_uniform_search(kernel):
    game, shape, n_row, delta = KERNELS[kernel]
    net, net_shape = _net(game, shape)
    G, n_playout = 40, 12
    eng, ev = _engine(game, shape, n_row, G, n_playout, net, net_shape, delta)
    ref, ev_ref = _engine(game, shape, n_row, G, n_playout, net, net_shape, delta)
    is_delta = kernel.startswith('k_delta_res')
    assert ev.resident_delta_ok(eng) == is_delta
    assert ev.route(eng).compact_resident == kernel.startswith('k_trunk_split')
    starts = _roots(game, shape, n_row, G, seed=5)
    c1 = np.array([PATTERN[g % 5] for g in range(G)])
    c2 = np.array([PATTERN[(g + 2) % 5] for g in range(G)])

    def search(counts):
        ev.hip.delta_stats(reset=True) if is_delta else None
        eng.set_playouts(counts)
        eng.simulate(ev)                       # (n_playout: the launch's maximum)
        eng.set_playouts(None)
        visits = eng.root_visits()
        got = [_state(eng, g) for g in range(G)]
        st = eng.check()
        ev.hip.check_flags()
        assert st.reuse_dropped == 0
        if is_delta:
            stats = ev.hip.delta_stats()
            assert stats['delta'] + stats['no_base'] == int(counts.sum()), stats
        return visits, got

    tpr._set_roots(eng, starts)
    visits1, got1 = search(c1)
    assert [int(v.sum()) for v in visits1] == [c - 1 for c in c1]   # (the first simulation expands the root)
    # a real move: the most visited child (a game searched once has no visited child: its first legal action)
    moves = np.array([int(np.argmax(v)) if v.sum() else starts[g].leagel_actions()[0] for g, v in enumerate(visits1)], dtype=np.int32)
    eng.advance(moves)
    eng.step(moves)
    visits2, got2 = search(c2)

    # the reference: the same roots searched UNIFORMLY through today's path, one run per count
    for k, c in enumerate(PATTERN):
        mine = [g for g in range(G) if g % 5 == k]
        tpr._set_roots(ref, starts)
        ref.simulate(ev_ref, n_sims=c)
        want_visits = ref.root_visits()
        for g in mine:
            assert np.array_equal(want_visits[g], visits1[g]), (kernel, 'search 1', g, c)
            assert _state(ref, g) == got1[g], (kernel, 'search 1', g, c)
        ref.advance(moves)
        ref.step(moves)
        ref.simulate(ev_ref, n_sims=PATTERN[(k + 2) % 5])
        want_visits = ref.root_visits()
        for g in mine:
            assert np.array_equal(want_visits[g], visits2[g]), (kernel, 'search 2', g, c)
            assert _state(ref, g) == got2[g], (kernel, 'search 2', g, c)
        assert ref.check().reuse_dropped == 0
    _close(eng, ref, ev, ev_ref)


def test_counts_against_the_oracle():
    net, net_shape = _net('gomoku', 6)
    counts = np.array([1, 5, 9, 20, 20, 3])
    eng, ev = _engine('gomoku', 6, 4, 6, 20, net, net_shape)
    probe = tpr._Probe(net, 'gomoku', 6, 4)
    starts = tpr._start_positions('gomoku', 6, 4, 6, seed=3)
    tpr._set_roots(eng, starts)
    eng.set_playouts(counts)
    eng.simulate(ev)
    for g, start in enumerate(starts):
        oracle = RefSearch(probe, int(counts[g]), 5)
        oracle.simulate(start.clone(), 1.0)
        assert tpr._hex_tree(eng.tree_dump(g)) == tpr._hex_tree(tree_dump(oracle.root)), g
    assert eng.check().reuse_dropped == 0
    probe.close()
    _close(eng, ev)


def test_order_changes_nothing():
    net, net_shape = _net('gomoku', 15)
    G = 16
    eng, ev = _engine('gomoku', 15, 5, G, 12, net, net_shape)
    assert ev.resident_delta_ok(eng)
    starts = _roots('gomoku', 15, 5, G, seed=9)
    counts = np.random.RandomState(1).randint(1, 13, size=G)
    seen = []
    for how in (dict(longest_first=False), dict(order=np.arange(G)[::-1]), dict(longest_first=True)):
        tpr._set_roots(eng, starts)
        eng.set_playouts(counts, **how)
        got_counts, got_order, source = eng.playouts()
        assert source == 'host' and got_counts.tolist() == counts.tolist()
        if 'order' in how:
            assert got_order.tolist() == list(range(G))[::-1]
        elif how['longest_first']:
            assert got_order.tolist() == np.argsort(-counts, kind='stable').tolist()
        else:
            assert got_order is None
        eng.simulate(ev)
        seen.append(([_state(eng, g) for g in range(G)], eng.root_visits().tolist()))
        assert eng.check().reuse_dropped == 0
    assert seen[0] == seen[1] == seen[2]
    assert [sum(v) for v in seen[0][1]] == [c - 1 for c in counts]
    eng.set_playouts(None)
    assert eng.playouts() == (None, None, None)
    _close(eng, ev)


@pytest.mark.parametrize('G', [70, 300])
def test_device_partition_is_stable(G):
    """k_play_order read back: random full / fast / inactive slots, more than one wave (70) and more than one chunk of 256 (300)."""
    import torch
    from rlzero_amd.engine import MCTSEngine
    n_playout, n_fast, p_full = 8, 2, 0.4
    eng = MCTSEngine(3, 3, n_games=G, n_playout=n_playout, device='cuda:0')
    ids = np.random.RandomState(G).permutation(4 * G)[:(2 * G) // 3]   # a third of the slots stays idle: whichever lose the race
    queue = torch.from_numpy(ids.astype(np.int64)).to('cuda:0')
    ctl = torch.tensor([0, len(ids)], dtype=torch.int32, device='cuda:0')
    eng.play_attach(SEED, 1.0, queue, ctl)
    eng.play_refill()
    eng.play_set_cap(n_fast, p_full)
    counts, order, source = eng.playouts()
    gids, plies, state, _ = eng.play_state()
    from rlzero_amd.selfplay import cap_uniform
    running = state == 1
    assert source == 'device' and running.sum() == len(ids) and sorted(gids[running].tolist()) == sorted(ids.tolist())
    full = cap_uniform(SEED, np.maximum(gids, 0), plies) < p_full
    assert counts[running].tolist() == np.where(full, n_playout, n_fast)[running].tolist()
    cls = np.where(~running, 2, np.where(counts >= n_playout, 0, 1))
    assert set(cls.tolist()) == {0, 1, 2}
    assert sorted(order.tolist()) == list(range(G))                                   # a permutation
    assert order.tolist() == sorted(range(G), key=lambda g: (cls[g], g))              # full, fast, inactive; stable within each
    eng.close()


# ----------------------------------------------------------------------------------------------- self-play under a cap
def _sp(board, n_games, n_playout, **extra):
    from rlzero_amd.selfplay import BatchedSelfPlay
    net, _ = _net('gomoku', board)
    return BatchedSelfPlay.for_network(net, board, 4 if board == 6 else 5, n_games=n_games, n_playout=n_playout, lanes=1, device='cuda:0',
                                       temperature=1.0, seed=SEED, **extra)


def _spy(sp):
    """Records of the device loop as _harvest consumes them -> {(game id, ply): (flags, N(root))} of the searched ones."""
    from rlzero_amd import playlog
    from rlzero_amd._hip import PLAY_SEARCHED
    seen, inner = {}, sp._harvest

    def harvest(lane, keep):
        before = [r for rows, _ in lane.inflight for r in rows]
        out = inner(lane, keep)
        left = set(r for rows, _ in lane.inflight for r in rows)
        for r in before:
            if r in left:
                continue
            d = playlog.running(lane.host_np[r][None])[1]
            for i in np.nonzero(d.flags & PLAY_SEARCHED)[0]:
                seen[(int(d.game[i]), int(d.ply[i]))] = (int(d.flags[i]), int(d.root_n[i]))
        return out
    sp._harvest = harvest
    return seen


def _root_n(board, n_row, count):
    """N(root) after ``count`` simulations from the empty board, by the oracle (values do not enter a visit count)."""
    oracle = RefSearch(lambda env: ([(a, 1.0 / len(env.leagel_actions())) for a in env.leagel_actions()], 0.0), count, 5)
    oracle.simulate(RefGomoku(board, n_row), 1.0)
    return tree_dump(oracle.root)[()][0]


def _check_flags(trajs, seen, cap, board, n_row, n_playout):
    from rlzero_amd._hip import PLAY_FULL
    from rlzero_amd.selfplay import cap_uniform
    n_fast, p_full = cap
    want_n = {True: _root_n(board, n_row, n_playout), False: _root_n(board, n_row, n_fast)}
    at_ply0 = set()
    for t in trajs:
        want = cap_uniform(SEED, t.game_id, np.arange(len(t.full))) < p_full
        assert t.full.tolist() == want.tolist() and len(t.full) == len(t.moves), t.game_id
        for ply in range(len(t.moves)):
            flags, _ = seen[(t.game_id, ply)]
            assert bool(flags & PLAY_FULL) == bool(want[ply]), (t.game_id, ply)
        assert seen[(t.game_id, 0)][1] == want_n[bool(want[0])], (t.game_id, seen[(t.game_id, 0)], want_n)
        at_ply0.add(bool(want[0]))
    assert at_ply0 == {True, False}   # both budgets occur on a known root


def _same_games(a, b, full=True):
    assert [t.game_id for t in a] == [t.game_id for t in b]
    for x, y in zip(a, b):
        assert (x.winner, x.moves) == (y.winner, y.moves), x.game_id
        assert np.array_equal(np.asarray(x.pis).view(np.uint64), np.asarray(y.pis).view(np.uint64)), x.game_id
        if full:
            assert x.full.tolist() == y.full.tolist(), x.game_id


@pytest.mark.parametrize('board,slots,games,n_playout,cap', [(9, 6, 14, 32, (6, 0.4)), (15, 4, 8, 24, (5, 0.5))])
def test_both_loops_agree(board, slots, games, n_playout, cap):
    sp = _sp(board, slots, n_playout, playout_cap=cap)
    assert all(lane.eng._ask(lane.evaluator)[0].resident for lane in sp.lanes)
    seen = _spy(sp)
    ids = list(range(games))
    dev = sp.run_device(ids)
    assert sp.lanes[0].eng.play_cap_on
    _check_flags(dev, seen, cap, board, 5, n_playout)
    host = sp.run(ids)
    _same_games(dev, host)
    plies = sum(len(t.moves) for t in dev)
    assert sum(len(t.training_samples()) for t in dev) == sum(int(t.full.sum()) for t in dev) < plies
    again = sp.run_device(ids)   # (the host loop's counts do not linger)
    _same_games(dev, again)
    for lane in sp.lanes:
        lane.eng.close()


def test_p_full_one_is_the_uncapped_game():
    ids = list(range(12))
    plain = _sp(6, 6, 40).run_device(ids)
    sp = _sp(6, 6, 40, playout_cap=(3, 1.0))
    got = sp.run_device(ids)
    _same_games(plain, got, full=False)
    assert all(t.full is None for t in plain) and all(t.full.all() and len(t.full) == len(t.moves) for t in got)
    _same_games(got, sp.run(ids))
    for lane in sp.lanes:
        lane.eng.close()


def test_new_cap_reaches_the_move_graph():
    ids = list(range(16))
    plain = _sp(6, 6, 40).run_device(ids)
    sp = _sp(6, 6, 40, playout_cap=(5, 0.5))
    seen = _spy(sp)
    sp.device_attach()
    graph = sp.lanes[0].move_graph
    assert graph is not None and sp.lanes[0].eng.play_cap_on
    first = sp.run_device(ids)
    _check_flags(first, seen, (5, 0.5), 6, 4, 40)
    seen.clear()
    sp.set_playout_cap(9, 0.3)
    assert sp.lanes[0].move_graph is graph   # no new capture
    got = sp.run_device(ids)
    assert sp.lanes[0].move_graph is graph
    _check_flags(got, seen, (9, 0.3), 6, 4, 40)
    assert [t.moves for t in got] != [t.moves for t in first]
    # off again: the same graph plays the games without a cap
    sp.set_playout_cap(None)
    off = sp.run_device(ids)
    assert sp.lanes[0].move_graph is graph
    _same_games(plain, off, full=False)
    assert all(t.full is None for t in off)
    # an object attached WITHOUT a cap: the first cap captures the move graph again, and it is obeyed
    sp2 = _sp(6, 6, 40)
    sp2.device_attach()
    g0 = sp2.lanes[0].move_graph
    assert g0 is not None and not sp2.lanes[0].eng.play_cap_on
    sp2.set_playout_cap(9, 0.3)
    assert sp2.lanes[0].move_graph is not g0 and sp2.lanes[0].eng.play_cap_on
    _same_games(got, sp2.run_device(ids))
    for lane in sp.lanes + sp2.lanes:
        lane.eng.close()


def test_refusals_on_the_device():
    from rlzero_amd.engine import MCTSEngine, SyntheticEvaluator
    puct = MCTSEngine(6, 4, n_games=2, n_playout=8, device='cuda:0', score_mode='puct')
    with pytest.raises(ValueError):
        puct.set_playouts([1, 2])
    rc = puct.lib.rz_set_playouts(puct.handle, puct.moves.data_ptr(), None, None)   # the library itself: RZ_ERR_ARG with a message
    assert rc != 0 and b'resident' in puct.lib.rz_last_error()
    puct.close()
    eng = MCTSEngine(6, 4, n_games=2, n_playout=8, device='cuda:0')
    for bad in ([1], [0, 3], [1.5, 2.0]):
        with pytest.raises(ValueError):
            eng.set_playouts(bad)
    eng.set_playouts([1, 2])
    with pytest.raises(ValueError, match='resident'):   # an evaluator without a resident search
        eng.simulate(SyntheticEvaluator('v0'), 4)
    head = eng.lib.rz_expand_backup(eng.handle, eng.logp.data_ptr(), eng.value.data_ptr(), None)
    assert head != 0 and b'resident' in eng.lib.rz_last_error()
    eng.set_playouts(None)
    eng.simulate(SyntheticEvaluator('v0'), 4)
    eng.close()


def test_trainer_playout_cap_smoke(tmp_path):
    cmd = [sys.executable, os.path.join(REPO, 'tools', 'train_alphazero.py'), '--board', '6', '--n-in-row', '4', '--playouts', '24',
           '--batches', '2', '--check-freq', '100', '--games-in-flight', '16', '--playout-cap', '6:0.5', '--seed', '3']
    env = dict(os.environ, PYTHONPATH=REPO)
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('playout cap:')]
    assert len(lines) == 2, out.stdout[-2000:]
    full, plies = int(lines[0].split()[2]), int(lines[0].split()[4])
    assert 0 < full < plies
