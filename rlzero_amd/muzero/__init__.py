"""MuZero on MI355X (BASELINE.json configs[4]: learned dynamics on CartPole-v1, 50 simulations per move,
recurrent unroll K = 5).  The reference names MuZero but ships none (README.md:3,
rlzero/algorithms/rl_args.py:21-24), so this package is build-defined: the published algorithm
(arXiv:1911.08265v2) with the search tree in hand-written HIP kernels (csrc/rz_muzero.hip, C ABI rz_mz_*),
the small MLPs of the learned model and the learner on PyTorch-ROCm (opt-in: the learner step in HIP as well, learner.py)."""
from .acrobot import AcrobotBatch, acrobot_initial_states
from .agent import MuZeroAgent
from .cartpole import CartPoleBatch
from .learner import MuZeroFusedLearner
from .network import MuZeroNet, inverse_value_transform, value_transform
from .reanalyse import MuZeroReanalyser, mz_reanalyse_draws
from .replay import MuZeroDeviceReplay, mz_prioritized_draws, mz_priority_weights, mz_replay_draws
from .selfplay import MuZeroSelfPlay, ReplayBuffer
from .tree import MuZeroTree

__all__ = ['MuZeroAgent', 'CartPoleBatch', 'MuZeroNet', 'MuZeroSelfPlay', 'ReplayBuffer', 'MuZeroTree', 'MuZeroDeviceReplay', 'mz_replay_draws',
           'MuZeroReanalyser', 'mz_reanalyse_draws', 'mz_priority_weights', 'mz_prioritized_draws', 'MuZeroFusedLearner', 'AcrobotBatch', 'acrobot_initial_states',
           'value_transform', 'inverse_value_transform']
