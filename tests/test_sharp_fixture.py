"""The g9 fixtures (boards of 11, 15 and 16 rows on sharp_weights: values that steer a search) against the oracle, on the CPU.

The fixtures are the reference's own runs (tests/golden/gen_golden.py g9).  Here: the restatement (oracle/) on the same weights rebuilds
every recorded search bit for bit and plays the shortest game ply for ply, and the fixture itself meets the conditions it was chosen
by -- so that the device tests of tests/test_sharp_net_rows.py, which read their tolerances from it, compare what they claim to."""
import numpy as np
import pytest
import sharp_fixture as sf

from oracle import evaluators as ev
from oracle.gomoku_ref import RefGomoku
from oracle.mcts_ref import RefPlayer, RefSearch, inverse_cdf_choice, tree_dump


@pytest.mark.parametrize('B', sf.BOARDS)
def test_the_oracle_rebuilds_every_sharp_search_bit_for_bit(B):
    """Leaf paths and f32 values of every simulation, the root record and the whole tree dump (N and the bits of W)."""
    import torch
    torch.set_num_threads(1)
    w = sf.weights(B)
    for rec in sf.search(B)['cases']:
        s = RefSearch(ev.NetEvaluator(w, B), rec['n_playout'], rec['c_puct'])
        s.leaf_log = []
        with torch.no_grad():
            acts, probs = s.simulate(RefGomoku.from_moves(B, rec['n'], rec['pre']), temperature=rec['T'])
        assert [list(p) for p, _ in s.leaf_log] == [p for p, _ in rec['leaves']], rec['name']
        terminal = set(rec['terminal'])   # (a terminal leaf's backup is +-1 / 0: the log holds that, the fixture the net's output)
        assert [float(v).hex() for i, (_, v) in enumerate(s.leaf_log) if i not in terminal] == \
            [v for i, (_, v) in enumerate(rec['leaves']) if i not in terminal], rec['name']
        assert list(acts) == rec['acts'] and [k.n for k in s.root.kids] == rec['N']
        assert [float(k.w).hex() for k in s.root.kids] == rec['W']
        assert np.max(np.abs(np.asarray(probs) - np.array([float.fromhex(p) for p in rec['pi']]))) <= 1e-12
        assert {p: (n, float(x).hex()) for p, (n, x) in tree_dump(s.root).items()} == {tuple(p): (n, x) for p, n, x in rec['tree']}, rec['name']


def test_the_oracle_plays_the_shortest_sharp_game_ply_for_ply():
    import torch
    torch.set_num_threads(1)
    game = min(sf.games(), key=lambda g: (len(g['plies']), g['seed']))
    B = game['B']
    player = RefPlayer(ev.NetEvaluator(sf.weights(B), B), n_playout=game['n_playout'], c_puct=game['c_puct'], is_selfplay=True,
                       choice=inverse_cdf_choice(float.fromhex(p['u']) for p in game['plies']))
    env = RefGomoku(B, game['n'])
    env.reset()
    for ply in game['plies']:
        with torch.no_grad():
            acts, probs = player.mcts.simulate(env, game['T'])
        assert list(acts) == ply['acts'] and [kid.n for kid in player.mcts.root.kids] == ply['N']
        move = player.choice(acts, probs)
        assert int(move) == ply['move']
        player.mcts.update_with_move(move)
        env.step(move)
    if game['winner'] is not None:
        assert env.game_end_winner() == (True, game['winner'])


@pytest.mark.parametrize('B', sf.BOARDS)
def test_the_sharp_fixture_meets_the_conditions_it_was_chosen_by(B):
    """Values that matter (std >= 0.2 in fp64 over every position and leaf the fixture holds, at most 5 % behind a saturated tanh, a
    mean spread of the log-probabilities >= 3); tolerances E = 4 e_value <= 2e-6 and E_lp = 4 e_logp <= 2e-5; enough cases whose tree
    does not hang on a rounding (the reference's N at every node under values moved by +-E with four sign patterns, and in fp64)."""
    import torch
    head = sf.search(B)
    w = sf.weights(B)
    pos = sf.net(B)
    # the positions: the recorded f32 outputs are the restatement's, and the statistics are those stored
    planes = [pos['planes']]
    for rec in head['cases']:
        root, states = RefGomoku.from_moves(B, rec['n'], rec['pre']), []
        for path, _ in rec['leaves']:
            env = root.clone()
            for m in path:
                env.step(m)
            states.append(env.current_state())
        planes.append(np.array(states, dtype=np.float32))
    planes = np.concatenate(planes)
    assert len(planes) == head['stats']['n_positions']
    with torch.no_grad():
        lp64, v64 = ev.net_forward(w, planes, torch.float64)
        lp32, v32 = ev.net_forward(w, pos['planes'])
    v64, lp64 = v64.numpy().reshape(-1), lp64.numpy()
    assert v64.std() >= 0.2 and abs(v64.std() - head['stats']['value_std']) < 1e-9
    assert (np.abs(v64) > 0.99).mean() <= 0.05
    assert (lp64.max(axis=1) - lp64.min(axis=1)).mean() >= 3.0
    E, E_lp = sf.tolerances(B)
    assert head['margin'] == 4 and 0 < E <= sf.E_VALUE_MAX and 0 < E_lp <= sf.E_LOGP_MAX
    # (the restatement in f32, all 24 in one batch: another summation order than the reference's batch-1 calls, each within e of fp64)
    assert np.max(np.abs(v32.numpy().reshape(-1) - pos['value'])) <= E / 2 and np.max(np.abs(lp32.numpy() - pos['log_probs'])) <= E_lp / 2
    assert np.max(np.abs(v64[:24] - pos['value'])) <= E / 4 and np.max(np.abs(lp64[:24] - pos['log_probs'])) <= E_lp / 4
    # the 24 positions: the kinds the issue names
    stones = pos['planes'][:, :2].sum(axis=(1, 2, 3))
    assert len(stones) == 24 and stones[0] == 0 and stones[1] == 1 and (B * B - stones <= 12).sum() >= 2
    last = [m[-1] for m in pos['moves'][2:6]]
    assert [(c // B == 0, c // B == B - 1, c % B == 0, c % B == B - 1)[i] for i, c in enumerate(last)] == [True] * 4
    # the searches
    names = [c['name'] for c in head['cases']]
    assert {'empty', 'edge', 'near_win'} <= set(names) and (B == 11 or 'late' in names)
    assert sum(1 for c in head['cases'] if c['robust']) >= 3
    by_name = {c['name']: c for c in head['cases']}
    assert by_name['near_win']['terminal'], 'the near-win root must meet terminal leaves'
    if B == 15:
        assert by_name['late']['robust']
    if B != 11:
        assert 10 <= B * B - len(by_name['late']['pre']) <= 14 and by_name['late']['max_depth'] >= 3
    sims = {11: 150, 15: 400, 16: 300}[B]
    assert all(c['n_playout'] == sims and len(c['leaves']) == sims for c in head['cases'])


def test_the_sharp_games_have_enough_plies_no_rounding_decides():
    gs = sf.games()
    assert sorted((g['B'], g['n_playout']) for g in gs) == [(11, 150), (11, 150), (15, 300), (15, 300)]
    for g in gs:
        assert g['robust_plies'] >= 8 and g['robust_plies'] <= len(g['plies'])
        assert (g['winner'] is not None) if g['B'] == 11 else len(g['plies']) == 12
