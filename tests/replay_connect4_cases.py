"""Helpers of the Connect4 replay tests (test_replay_connect4_host.py, test_replay_connect4_gpu.py): seeded random LEGAL games as
Trajectory objects -- columns, with pi rows over the columns that are not full -- and the trainer's host ReplayBuffer they are
compared with."""
import numpy as np

import replay_cases as rc

BOARDS = [(6, 7, 4), (4, 5, 3), (9, 8, 4), (4, 16, 4)]   # rows, cols, n_in_row: the default; a small one; 72 cells (two mask words); the widest


def random_columns(rows, cols, plies, rs, avoid_lines=0):
    """``plies`` legal drops in seeded random order (fewer if ``avoid_lines`` = n_in_row > 0 leaves no drop that completes no line)."""
    from rlzero_amd.games.connect4.connect4_env import _start_masks
    from rlzero_amd.games.gomoku.gomoku_env import has_line
    masks = _start_masks(rows, cols, avoid_lines) if avoid_lines else None
    height, bits, moves = [0] * cols, [0, 0], []
    for p in range(plies):
        for column in rs.permutation(cols):
            column = int(column)
            if height[column] >= rows:
                continue
            bit = 1 << (height[column] * cols + column)
            if masks is not None and has_line(bits[p & 1] | bit, masks, avoid_lines):
                continue
            moves.append(column)
            bits[p & 1] |= bit
            height[column] += 1
            break
        else:
            break
    return moves


def random_pis(rows, cols, moves, rs, dtype=np.float64):
    """Dirichlet rows over the columns that are not full before every ply."""
    height, pis = [0] * cols, np.zeros((len(moves), cols))
    for p, column in enumerate(moves):
        open_ = [c for c in range(cols) if height[c] < rows]
        pis[p, open_] = rs.dirichlet(np.full(len(open_), 0.3))
        height[column] += 1
    return pis.astype(dtype)


def random_game(board, plies, winner, seed, game_id=0, full=None, pi_dtype=np.float64, n_in_row=4, avoid_lines=False):
    """A legal Connect4 game of ``plies`` drops on ``board`` = (rows, cols)."""
    from rlzero_amd.selfplay import Trajectory
    rows, cols = board
    rs = np.random.RandomState(seed)
    moves = random_columns(rows, cols, plies, rs, n_in_row if avoid_lines else 0)
    assert avoid_lines or len(moves) == plies
    return Trajectory(game_id, (rows, cols), n_in_row, moves, random_pis(rows, cols, moves, rs, pi_dtype), winner, game='connect4', full=full)


def column_filler(board, seed, game_id=0, n_in_row=4):
    """A game that fills column 0 to the top first (the two players alternate in it), then drops at random until the board is full."""
    from rlzero_amd.selfplay import Trajectory
    rows, cols = board
    rs = np.random.RandomState(seed)
    moves, height = [0] * rows, [rows] + [0] * (cols - 1)
    while len(moves) < rows * cols:
        column = int(rs.choice([c for c in range(cols) if height[c] < rows]))
        moves.append(column)
        height[column] += 1
    return Trajectory(game_id, (rows, cols), n_in_row, moves, random_pis(rows, cols, moves, rs), -1, game='connect4')


def host_buffer(trajectories, capacity, board):
    """ReplayBuffer(2 * capacity, board, game='connect4') fed every game's training_samples(): what
    DeviceReplay(board, capacity, game='connect4') must hold."""
    buf = rc.trainer().ReplayBuffer(2 * capacity, board, game='connect4')
    for t in trajectories:
        buf.extend_samples(t.training_samples())
    return buf
