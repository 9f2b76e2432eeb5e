"""Network-vs-network matches, the host's side (rlzero_amd/match.py): openings, pair and seat arithmetic, the pair's uniform, the
score -- and a match played on the CPU by the oracle's play_game from an opening, the device-free twin of tests/test_match_gpu.py."""
import math

import numpy as np
import pytest

from oracle import evaluators as ev
from oracle.gomoku_ref import RefGomoku
from oracle.mcts_ref import RefPlayer, play_game
from rlzero_amd import match as M
from rlzero_amd.selfplay import draw_move, move_uniform


def test_paired_openings_are_distinct_legal_positions_with_player_0_to_move():
    opens = M.paired_openings(6, 4, 12, 4, seed=3)
    assert opens == M.paired_openings(6, 4, 12, 4, seed=3)          # reproducible from the seed
    assert opens != M.paired_openings(6, 4, 12, 4, seed=4)
    keys = set()
    for moves in opens:
        assert len(moves) == 4 and len(set(moves)) == 4 and all(0 <= m < 36 for m in moves)   # legal: distinct empty cells
        env = RefGomoku.from_moves(6, 4, moves)
        assert not env.game_end_winner()[0] and env.current_player() == 0
        keys.add(env.bitboards() + (env.last_move, ))
    assert len(keys) == 12
    stones, to_move, last = M.opening_arrays(opens, 6, 4)
    assert stones.shape[0] == 12 and (to_move == 0).all() and [int(x) for x in last] == [m[-1] for m in opens]
    for i, moves in enumerate(opens):
        b0, b1 = RefGomoku.from_moves(6, 4, moves).bitboards()
        assert int(stones[i, 0, 0]) == b0 and int(stones[i, 1, 0]) == b1 and not stones[i, :, 1:].any()


def test_paired_openings_refuse_what_they_cannot_give():
    with pytest.raises(ValueError):
        M.paired_openings(6, 4, 2, 3, seed=0)        # odd: player 1 would be to move
    with pytest.raises(ValueError):
        M.paired_openings(6, 4, 2, 0, seed=0)        # one empty board, two asked for
    with pytest.raises(ValueError):
        M.paired_openings((6, 7), 4, 2, 2, seed=0, game='connect4')
    assert M.paired_openings(6, 4, 1, 0, seed=0) == [[]]
    with pytest.raises(ValueError):
        M.opening_arrays([[0, 1, 6, 2, 12, 3, 18]], 6, 4)   # player 0 has four in a column: terminal


def test_seats_and_pairs():
    gids = np.arange(10)
    assert M.pair_of(gids).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert M.opening_of(gids, 3).tolist() == [0, 0, 1, 1, 2, 2, 0, 0, 1, 1]
    assert M.seat_of(gids, M.NET_A).tolist() == [0, 1] * 5 and M.seat_of(gids, M.NET_B).tolist() == [1, 0] * 5
    # A moves iff (player 0 to move) == (even game): with player 0 to move after the opening, A opens the even game, B the odd one
    assert M.net_to_move(gids, np.zeros(10, int)).tolist() == [M.NET_A, M.NET_B] * 5
    assert M.net_to_move(gids, np.ones(10, int)).tolist() == [M.NET_B, M.NET_A] * 5
    for g in range(6):
        for tm in (0, 1):
            assert (int(M.net_to_move(g, tm)) == M.NET_A) == (int(M.seat_of(g, M.NET_A)) == tm)


def test_match_uniform_is_the_pairs_second_draw():
    gids, plies = np.array([0, 1, 2, 3, 6, 7, 1 << 33, (1 << 33) + 1]), np.array([0, 0, 5, 5, 9, 9, 2, 2])
    u = M.match_uniform(11, gids, plies)
    assert np.array_equal(u, move_uniform(11, gids >> 1, 2 * plies + 1))
    assert np.array_equal(u[0::2], u[1::2]) and len(set(u[0::2].tolist())) == 4     # shared within a pair, apart between pairs
    assert float(M.match_uniform(11, 5, 3)) == float(move_uniform(11, 2, 7))
    assert float(M.match_uniform(11, 5, 3)) != float(move_uniform(11, 5, 3))


def _result(gid, winner):
    return M.MatchResult(gid, 0, [], [0], winner, [np.zeros(1, np.int32)])


def test_score_counts_points_seats_and_pairs():
    # pair 0: A wins both (player 0 of game 0, player 1 of game 1); pair 1: A wins as first mover, loses as second; pair 2: two ties;
    # pair 3: a tie and a loss; pair 4: only its even game (an unfinished pair is no pair outcome)
    res = [_result(0, 0), _result(1, 1), _result(2, 0), _result(3, 0), _result(4, -1), _result(5, -1), _result(6, -1), _result(7, 0), _result(8, 1)]
    assert [r.points_a for r in res] == [1, 1, 1, 0, 0.5, 0.5, 0.5, 0, 0]
    s = M.score(res)
    assert (s['games'], s['a_wins'], s['b_wins'], s['ties'], s['a_points']) == (9, 3, 3, 3, 4.5)
    assert s['a_score'] == 0.5 and s['elo_diff'] == 0.0 and not s['elo_clipped']
    assert s['a_score_moving_first'] == (1 + 1 + 0.5 + 0.5 + 0) / 5 and s['a_score_moving_second'] == (1 + 0 + 0.5 + 0) / 4
    assert s['pairs'] == {'2-0': 1, '1.5-0.5': 0, '1-1': 1, 'tie-tie': 1, '0.5-1.5': 1, '0-2': 0}
    assert M.BatchedMatch.score(res) == s


def test_score_clips_a_shut_out():
    wins = [_result(g, g & 1) for g in range(8)]              # A: player 0 of the even games, player 1 of the odd ones
    s = M.score(wins)
    assert s['a_score'] == 1.0 and s['pairs']['2-0'] == 4 and s['elo_clipped']
    assert s['elo_diff'] == pytest.approx(-400 * math.log10(1 / (1 - 0.5 / 8) - 1)) and math.isfinite(s['elo_diff'])
    lost = M.score([_result(g, 1 - (g & 1)) for g in range(8)])
    assert lost['a_score'] == 0.0 and lost['pairs']['0-2'] == 4 and lost['elo_clipped'] and lost['elo_diff'] == -s['elo_diff']
    assert M.elo_from_score(0.75, 100) == (pytest.approx(400 * math.log10(3)), False)


# ------------------------------------------------------------------------- a match on the CPU
class _FromOpening(RefGomoku):
    """play_game resets its environment: this one resets to the opening."""

    def __init__(self, board, n_row, opening):
        self._opening = list(opening)
        RefGomoku.__init__(self, board, n_row)

    def reset(self, start_player_idx=0):
        RefGomoku.reset(self, start_player_idx)
        for m in self._opening:
            self.step(m)
        self._n_open = len(self.order)


class _Choice(object):
    """RefPlayer.choice on the match's uniforms: get_action draws twice per move, the second with the pair's uniform of the ply
    (counted from the opening); what it saw is kept, for the arbiter's expression."""

    def __init__(self, seed, gid, env):
        self.seed, self.gid, self.env, self.calls, self.seen = seed, gid, env, 0, []

    def __call__(self, acts, probs):
        ply = len(self.env.order) - self.env._n_open
        second = self.calls % 2 == 1
        self.calls += 1
        u = float(M.match_uniform(self.seed, self.gid, ply)) if second else float(move_uniform(self.seed, self.gid >> 1, 2 * ply))
        if second:
            self.seen.append((ply, tuple(acts), np.asarray(probs)))
        return draw_move(np.asarray(acts), np.asarray(probs, dtype=np.float64), u)


def _cpu_match(fn_a, fn_b, n_pairs, openings, seed, board=6, n_row=4, n_playout=24):
    out = []
    for gid in range(2 * n_pairs):
        k = int(M.opening_of(gid, len(openings)))
        env = _FromOpening(board, n_row, openings[k])
        players = {}
        for net, fn in ((M.NET_A, fn_a), (M.NET_B, fn_b)):
            players[int(M.seat_of(gid, net))] = RefPlayer(fn, n_playout=n_playout, c_puct=5, choice=_Choice(seed, gid, env))
        winner, moves = play_game(env, players[0], players[1])
        assert len(moves) == len(env.order) - len(openings[k])   # (play_game lists the moves after its reset: after the opening)
        # who drew which ply: the network whose turn it was (net_to_move on the side to move before the ply)
        for seat, p in players.items():
            for ply, acts, probs in p.choice.seen:
                assert ply % 2 == seat       # (player 0 moves the even plies from an opening with player 0 to move)
                net = M.NET_A if seat == int(M.seat_of(gid, M.NET_A)) else M.NET_B
                assert int(M.net_to_move(gid, ply % 2)) == net
                assert moves[ply] == draw_move(np.asarray(acts), probs, float(M.match_uniform(seed, gid, ply)))
        assert sum(len(p.choice.seen) for p in players.values()) == len(moves)
        out.append(M.MatchResult(gid, k, openings[k], moves, winner, [np.zeros(1, np.int32)] * len(moves)))
    return out


@pytest.fixture(scope='module')
def openings():
    return M.paired_openings(6, 4, 2, 2, seed=5)


def test_cpu_match_of_a_network_against_itself_is_one_half(openings):
    res = _cpu_match(ev.vlin, ev.vlin, 3, openings, seed=7)
    for a, b in zip(res[0::2], res[1::2]):
        assert a.pair == b.pair and a.opening == b.opening and a.moves == b.moves and a.winner == b.winner
        assert a.points_a + b.points_a == 1.0
    s = M.score(res)
    assert s['a_score'] == 0.5 and s['pairs']['2-0'] == s['pairs']['0-2'] == s['pairs']['1.5-0.5'] == s['pairs']['0.5-1.5'] == 0


def test_cpu_match_of_two_evaluators_from_openings(openings):
    res = _cpu_match(ev.vlin, ev.v0, 3, openings, seed=7)
    assert [r.game_id for r in res] == list(range(6)) and [r.opening for r in res] == [0, 0, 1, 1, 0, 0]
    for r in res:
        env = RefGomoku.from_moves(6, 4, r.opening_moves + r.moves)          # the moves are a legal game from the opening, to its end
        assert env.game_end_winner() == (True, r.winner)
        assert not RefGomoku.from_moves(6, 4, r.opening_moves + r.moves[:-1]).game_end_winner()[0]
        assert (r.seat_a, r.seat_b) == ((0, 1) if r.game_id % 2 == 0 else (1, 0))
    # the two games of a pair differ in who searches which side: with two different evaluators they are not the same game
    assert any(a.moves != b.moves for a, b in zip(res[0::2], res[1::2]))
    # pairs 0 and 2 share opening 0 but not their uniforms
    assert res[0].opening_moves == res[4].opening_moves
    s = M.score(res)
    assert s['games'] == 6 and s['a_wins'] + s['b_wins'] + s['ties'] == 6 and sum(s['pairs'].values()) == 3
    assert s['a_points'] == sum(r.points_a for r in res)
    # swapping the networks mirrors the score: B's games are A's with the seats exchanged within each pair
    swapped = _cpu_match(ev.v0, ev.vlin, 3, openings, seed=7)
    for r, q in zip(res, swapped):
        assert q.game_id == r.game_id and swapped[r.game_id ^ 1].moves == r.moves and swapped[r.game_id ^ 1].winner == r.winner
    assert M.score(swapped)['a_points'] == 6 - s['a_points']


# ------------------------------------------------------------------------- the command lines
def _tool(name):
    import importlib.util
    import os
    from conftest import REPO
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(REPO, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_match_tool_arguments():
    tool = _tool('match')
    args = tool.parse_args(['a.th', 'b.th', '--board', '15', '--n-in-row', '5', '--playouts', '800', '--pairs', '256', '--openings', '64',
                            '--opening-plies', '4', '--seed', '3'])
    assert (args.ckpt_a, args.ckpt_b, args.board, args.n_in_row, args.playouts, args.pairs, args.openings, args.opening_plies, args.seed) == \
        ('a.th', 'b.th', 15, 5, 800, 256, 64, 4, 3)
    for bad in (['--opening-plies', '3'], ['--pairs', '0'], ['--openings', '0']):
        with pytest.raises(SystemExit):
            tool.parse_args(['a.th', 'b.th'] + bad)


def test_trainer_gate_option_is_a_batched_mode_option():
    tool = _tool('train_alphazero')
    assert tool.parse_args([]).gate_against is None
    assert tool.parse_args(['--games-in-flight', '8', '--gate-against', 'old.model']).gate_against == 'old.model'
    with pytest.raises(SystemExit):
        tool.parse_args(['--gate-against', 'old.model'])
    with pytest.raises(ValueError):
        tool.TrainPipeline(gate_against='old.model')


def test_load_checkpoint_reads_a_file_and_a_save_model_directory(tmp_path):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(1)
    net = PolicyValueNet(6)
    (tmp_path / 'ckpt').mkdir()
    torch.save(net.state_dict(), str(tmp_path / 'ckpt' / 'model.th'))
    torch.save(net.state_dict(), str(tmp_path / 'plain.th'))
    for path in (tmp_path / 'ckpt', tmp_path / 'plain.th'):
        got = M.load_checkpoint(str(path), 6, device='cpu')
        assert all(torch.equal(a, b) for a, b in zip(got.state_dict().values(), net.state_dict().values()))
