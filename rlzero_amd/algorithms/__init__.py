"""Trainer API of the AlphaZero path.

In the reference the AlphaZero trainer is the ``TrainPipeline`` class inside the script
tools/train_alphazero.py:17-190 (``rlzero/algorithms`` only holds the unrelated DMC / CFR
code).  The batched, multi-GPU self-play collector that replaces its sequential
``collect_selfplay_data`` loop is ``rlzero_amd.selfplay``; it is re-exported here under the
name BASELINE.json uses, with the lock-step counterpart of ``policy_evaluate``'s games
(``rlzero_amd.evaluate``), the network-vs-network matches (``rlzero_amd.match``) and the replay buffer in device memory
with its reanalyser (``rlzero_amd.replay``).
"""
from ..evaluate import BatchedEvaluation, DuelResult
from ..match import BatchedMatch, MatchResult, paired_openings
from ..replay import (DeviceReplay, ReplayReanalyser, reanalysed_pi, replay_index, replay_indices, replay_reanalyse_draws,
                      symmetry_tables)
from ..selfplay import (BatchedSelfPlay, Trajectory, broadcast_weights, calibrate_resign_threshold, gather_trajectories,
                        shard_game_ids)

__all__ = ['BatchedSelfPlay', 'BatchedEvaluation', 'BatchedMatch', 'MatchResult', 'paired_openings', 'DuelResult', 'Trajectory', 'gather_trajectories', 'shard_game_ids', 'broadcast_weights',
           'calibrate_resign_threshold', 'DeviceReplay', 'symmetry_tables', 'replay_index', 'replay_indices', 'ReplayReanalyser', 'replay_reanalyse_draws',
           'reanalysed_pi']
