"""Helpers of the replay-buffer tests (test_replay_host.py, test_replay_gpu.py): the trainer script as a module, seeded random legal
games as Trajectory objects and the host ReplayBuffer they are compared with."""
import importlib.util
import os

import numpy as np
from conftest import REPO

_TRAINER = None


def trainer():
    """tools/train_alphazero.py as a module (ReplayBuffer, TrainPipeline, parse_args)."""
    global _TRAINER
    if _TRAINER is None:
        spec = importlib.util.spec_from_file_location('train_alphazero_replay', os.path.join(REPO, 'tools', 'train_alphazero.py'))
        _TRAINER = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_TRAINER)
    return _TRAINER


def random_game(board, plies, winner, seed, game_id=0, full=None, pi_dtype=np.float64):
    """A legal game of ``plies`` distinct cells in seeded random order, with Dirichlet pi rows over the cells still empty."""
    from rlzero_amd.selfplay import Trajectory
    rs = np.random.RandomState(seed)
    A = board * board
    moves = rs.permutation(A)[:plies]
    pis = np.zeros((plies, A))
    for p in range(plies):
        empty = np.setdiff1d(np.arange(A), moves[:p])
        pis[p, empty] = rs.dirichlet(np.full(len(empty), 0.3))
    return Trajectory(game_id, board, min(board, 5), moves.tolist(), pis.astype(pi_dtype), winner, full=full)


def host_buffer(trajectories, capacity, board):
    """ReplayBuffer(8 * capacity, board) fed every game's training_samples(): what DeviceReplay(board, capacity) must hold."""
    buf = trainer().ReplayBuffer(8 * capacity, board)
    for t in trajectories:
        buf.extend_samples(t.training_samples())
    return buf


def host_entries(buf, indices=None):
    """(states float32 [n,4,B,B], pis float32 [n,A], zs float32 [n]) of the host buffer's entries (all of them by default)."""
    indices = range(len(buf)) if indices is None else indices
    rows = [buf[int(i)] for i in indices]
    return (np.array([r[0] for r in rows], dtype=np.float32), np.array([r[1] for r in rows], dtype=np.float32),
            np.array([r[2] for r in rows], dtype=np.float32))
