"""The prologue of a receptive-field leaf (rz_delta.h, delta_passes): ranks and totals of the five cell sets come out of every wave's
ballots over the whole board, and the base's records are fetched once, straight into the registers they are stored from.  Which cell
goes into which tile and record slot is all that may change, so the counters and the trees of the resident search (k_delta_res) must
equal the two-launch step's (k_trunk_delta, the same leaves) and the full-board kernel's, bit for bit."""
import numpy as np
import pytest

from oracle.gomoku_ref import RefGomoku

pytestmark = pytest.mark.gpu

STATS = ('delta', 'no_base', 'cells', 'tiles3', 'tiles2')


def _roots(B, n, count, seed):
    """Random non-terminal positions of up to half a board."""
    rs = np.random.RandomState(seed)
    envs = []
    while len(envs) < count:
        e = RefGomoku(B, n)
        for m in rs.permutation(B * B)[:rs.randint(0, B * B // 2)]:
            e.step(int(m))
            if e.game_end_winner()[0]:
                break
        if not e.game_end_winner()[0]:
            envs.append(e)
    return envs


def _late_roots(B, n, count, seed):
    """Nearly full boards without a line: stones in runs of two along rows and diagonals, alternating down columns
    (cell (y, x) black when (x + 2 y) mod 4 < 2), 6 .. 9 cells left empty and the colours balanced (black to move or white)."""
    rs = np.random.RandomState(seed)
    envs = []
    for i in range(count):
        empty = set(rs.choice(B * B, 6 + i % 4, replace=False).tolist())
        black = [c for c in range(B * B) if c not in empty and (c % B + 2 * (c // B)) % 4 < 2]
        white = [c for c in range(B * B) if c not in empty and (c % B + 2 * (c // B)) % 4 >= 2]
        while not 0 <= len(black) - len(white) <= 1:
            big = black if len(black) > len(white) else white
            big.pop(rs.randint(len(big)))
        rs.shuffle(black)
        rs.shuffle(white)
        moves = [m for pair in zip(black, white) for m in pair] + black[len(white):]
        e = RefGomoku.from_moves(B, n, moves)
        assert not e.game_end_winner()[0]
        envs.append(e)
    return envs


def _net(B, seed):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(seed)
    return PolicyValueNet(B)


def _search(net, envs, sims, resident=True, delta=True):
    """One search from `envs` -> (root visits, whole trees, delta counters of the search)."""
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine, int_to_bits
    B = envs[0].board_size
    evaluator = HipNetEvaluator(net, B, 'cuda:0', max_boards=len(envs))
    evaluator.resident_search = resident
    evaluator.delta_trunk = delta
    eng = MCTSEngine(B, 5, n_games=len(envs), n_playout=sims, device='cuda:0', add_noise=True, noise_seed=3)
    assert evaluator.resident_ok(eng) == resident and evaluator.deferred_ok(eng) and evaluator.delta_ok(eng) == delta
    stones = np.array([[int_to_bits(e.bitboards()[0]), int_to_bits(e.bitboards()[1])] for e in envs], dtype=np.uint64)
    eng.set_roots(stones, [e.current_player() for e in envs], [e.last_move for e in envs], reset_trees=True)
    eng.set_noise_keys()
    evaluator.hip.delta_stats(reset=True)
    eng.simulate(evaluator, sims, use_graph=False)
    st = evaluator.hip.delta_stats()
    visits = eng.root_visits().copy()
    trees = [eng.tree_dump(g) for g in range(len(envs))]
    eng.check()
    eng.close()
    evaluator.hip.close()
    return visits, trees, {k: st[k] for k in STATS}


def test_resident_prologue_counts_equal_the_two_launch_step():
    """One seeded 15 x 15 search of 64 games: the resident search selects the same leaves as the two-launch step, so the leaves
    against a base, without one, the changed cells and the conv2 / conv3 tiles are the same numbers -- and the trees the same bits."""
    net = _net(15, 11)
    envs = _roots(15, 5, 64, seed=5)
    v_res, t_res, s_res = _search(net, envs, 96, resident=True)
    v_two, t_two, s_two = _search(net, envs, 96, resident=False)
    assert s_res['delta'] + s_res['no_base'] == 64 * 96, s_res
    assert s_res['delta'] > 0 and s_res['tiles3'] > 0 and s_res['tiles2'] > 0, s_res
    assert s_res == s_two
    assert np.array_equal(v_res, v_two)
    assert t_res == t_two


def test_deep_late_game_roots_take_the_passes_without_a_base():
    """Nearly full boards (6 .. 12 empty cells): a 120-simulation tree goes deeper than four changed cells, so leaves take the four
    passes without a base (no_base > 0) beside leaves against it; the trees equal the full-board kernel's bit for bit."""
    net = _net(15, 12)
    envs = _late_roots(15, 5, 16, seed=20)
    v_res, t_res, s_res = _search(net, envs, 120, resident=True)
    assert s_res['no_base'] > 0 and s_res['delta'] > 0, s_res
    v_full, t_full, _ = _search(net, envs, 120, resident=True, delta=False)
    assert np.array_equal(v_res, v_full)
    assert t_res == t_full
