#!/usr/bin/env python3
"""AlphaZero training loop for Gomoku -- this repository's twin of the reference script
tools/train_alphazero.py (same import lines :11-14, attribute names :21-57, method names
``get_equi_data / collect_selfplay_data / policy_update / policy_evaluate / run`` and stdout
lines :124-136,161,170), running on the MI355X engine.

Two ways to collect self-play data:
  * ``selfplay_games_in_flight == 0`` (default): the reference's flow -- one game at a time
    through ``GameControl.start_self_play`` and ``AlphaZeroPlayer`` (search on the GPU);
  * ``selfplay_games_in_flight  > 0``: that many games in lock-step per collection round and GPU
    (``rlzero_amd.selfplay.BatchedSelfPlay``), the mode the hardware is built for; ``policy_evaluate``'s games then
    run in lock-step as well (``rlzero_amd.evaluate.BatchedEvaluation``), and ``--gate-against CKPT`` adds, at every
    ``check_freq``, the score of a match from paired openings against that checkpoint (``rlzero_amd.match``: reported next to
    the pure-MCTS win ratio, nothing is decided on it).

Several GPUs (``python tools/train_alphazero.py --gpus N ...`` starts one process per GPU itself, or run it under
``torch.distributed.run``): the games of a collection round are dealt to the ranks by id (game g -> rank g mod N, no
collective inside the search), ONE gather brings the finished trajectories to rank 0, which alone keeps the replay buffer
and runs ``policy_update`` / ``policy_evaluate`` / the checkpoints (train_alphazero.py:81-137,164-190), then ONE broadcast
hands every rank the new weights for its next round.  A game's trajectory depends on (seed, game id) only, so the data --
and with them the losses -- are those of the single-process run on the same ids.

Reference quirks kept on purpose: ``lr_multiplier`` is adapted but never
applied and ``learn_rate`` is never passed to the agent (D-7); ``policy_evaluate`` counts
``win_cnt[1]`` as wins although player ids are 0/1 (D-6); ``get_equi_data`` rotates the planes
by +i*90 degrees and pi by -i*90 degrees for odd i (D-9).

``--game connect4`` (build-defined: the reference has no Connect4) trains on a ``--board`` x ``--board-width`` board (6 x 7, four in
a row) in the batched mode only: self-play, the evaluation games, either replay buffer and Reanalyse take the game; the reference
flow, ``--gate-against`` and several ranks are refused.  Its augmentation is the left-right mirror alone -- entry 2 j + k of a
buffer is sample j as played (k = 0) or with every plane ``[:, :, ::-1]`` and ``pi[::-1]`` (k = 1) --: gravity breaks the rotations.
"""
from __future__ import print_function

import os
import random
import sys
from collections import defaultdict, deque
from collections.abc import Sequence

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from rlzero.games.gomoku import GameControl, GomokuEnv
from rlzero.games.gomoku.alphazero_agent import AlphaZeroAgent
from rlzero.mcts.alphazero_mcts import AlphaZeroPlayer
from rlzero.mcts.rollout_mcts import RolloutPlayer


def _symmetries(planes, pi_grid):
    """The 8 (state, pi) pairs the reference generates for one sample, in its order: for
    i = 1..4 the pair rotated by i quarter turns, then its left-right mirror.  The policy goes
    through the reference's flipud / rot90 / flipud sandwich (train_alphazero.py:65-78)."""
    out = []
    upside_down = np.flipud(pi_grid)
    for quarter_turns in (1, 2, 3, 4):
        turned = np.array([np.rot90(plane, quarter_turns) for plane in planes])
        pi_turned = np.rot90(upside_down, quarter_turns)
        out.append((turned, np.flipud(pi_turned).flatten()))
        mirrored = np.array([np.fliplr(plane) for plane in turned])
        out.append((mirrored, np.flipud(np.fliplr(pi_turned)).flatten()))
    return out


class ReplayBuffer(Sequence):
    """The reference's ``deque(maxlen=buffer_size)`` of augmented samples (train_alphazero.py:32, 59-79, 88-90) with the 8 symmetries
    formed WHEN A SAMPLE IS READ instead of when a game arrives: entry 8 j + k is symmetry k of the j-th sample ever added, in
    get_equi_data's order and with its numpy operations -- value for value what ``deque.extend(get_equi_data(play_data))`` would
    hold (tests/test_train_script.py) -- but a collection round of 512 games (52 k positions, 420 k entries) costs the host a list
    append per game where forming every symmetry up front cost more than the round's self-play on the GPU, and a mini-batch reads 32.
    Sequence protocol (len, index, iteration: what ``random.sample`` and the tests use), ``maxlen``, ``extend`` (ready-made
    entries: the reference flow), ``extend_samples`` (a game's un-augmented samples).
    ``game='connect4'`` (``board_size``: (rows, cols)): TWO symmetries, entry 2 j + k -- k = 0 the sample as played, k = 1 its
    left-right mirror, every plane ``[:, :, ::-1]`` and ``pi[::-1]``."""

    def __init__(self, maxlen, board_size, game='gomoku'):
        self.maxlen, self.game = int(maxlen), game
        self.size = tuple(int(v) for v in board_size) if game == 'connect4' else int(board_size)
        self.n_symmetries = 2 if game == 'connect4' else 8
        self._blocks = deque()   # ('raw', [entries]) or ('game', states [P,4,B,B], pi grids [P,B,B], z [P])
        self._counts = deque()   # entries each block contributes
        self._skip = 0           # entries of the FIRST block that have fallen out (maxlen)
        self._len = 0

    def __len__(self):
        return self._len

    def _trim(self):
        over = self._len - self.maxlen
        while over > 0:
            left = self._counts[0] - self._skip
            if over >= left:
                self._blocks.popleft()
                self._counts.popleft()
                self._skip = 0
                self._len -= left
                over -= left
            else:
                self._skip += over
                self._len -= over
                over = 0

    def extend(self, entries):
        entries = list(entries)
        if entries:
            self._blocks.append(('raw', entries))
            self._counts.append(len(entries))
            self._len += len(entries)
            self._trim()

    def extend_samples(self, play_data):
        """A game's (state, mcts_prob, z) samples, un-augmented: 8 entries each (Connect4: 2), formed on access."""
        play_data = list(play_data)
        if not play_data:
            return
        states = np.stack([np.asarray(s_) for s_, _, _ in play_data])
        if self.game == 'connect4':
            grids = np.stack([np.asarray(p_).reshape(self.size[1]) for _, p_, _ in play_data])   # (a pi row: one value per column)
        else:
            grids = np.stack([np.asarray(p_).reshape(self.size, self.size) for _, p_, _ in play_data])
        self._blocks.append(('game', states, grids, [w for _, _, w in play_data]))
        self._counts.append(self.n_symmetries * len(play_data))
        self._len += self.n_symmetries * len(play_data)
        self._trim()

    def _entry(self, block, i):
        if block[0] == 'raw':
            return block[1][i]
        _, states, grids, zs = block
        if self.game == 'connect4':
            j, k = divmod(i, 2)
            if k == 1:   # the left-right mirror
                return np.ascontiguousarray(states[j][:, :, ::-1]), np.ascontiguousarray(grids[j][::-1]), zs[j]
            return states[j], grids[j], zs[j]
        j, k = divmod(i, 8)
        quarter_turns, mirrored = k // 2 + 1, k % 2 == 1
        turned = np.rot90(states[j:j + 1], quarter_turns, axes=(2, 3))            # get_equi_data's operations on a stack of one
        pi_turned = np.rot90(grids[j:j + 1, ::-1, :], quarter_turns, axes=(1, 2))
        if mirrored:
            return (np.ascontiguousarray(turned[:, :, :, ::-1])[0], np.ascontiguousarray(pi_turned[:, :, ::-1][:, ::-1, :]).reshape(1, -1)[0], zs[j])
        return np.ascontiguousarray(turned)[0], np.ascontiguousarray(pi_turned[:, ::-1, :]).reshape(1, -1)[0], zs[j]

    def __getitem__(self, index):
        if isinstance(index, slice):
            return [self[i] for i in range(*index.indices(self._len))]
        if index < 0:
            index += self._len
        if not 0 <= index < self._len:
            raise IndexError('ReplayBuffer index out of range')
        index += self._skip
        for block, count in zip(self._blocks, self._counts):
            if index < count:
                return self._entry(block, index)
            index -= count
        raise IndexError('ReplayBuffer index out of range')

    def __iter__(self):
        first = True
        for block, count in zip(self._blocks, self._counts):
            for i in range(self._skip if first else 0, count):
                yield self._entry(block, i)
            first = False


class TrainPipeline:

    def __init__(self, board_size=6, n_in_row=4, n_playout=400, game_batch_num=64, check_freq=50,
                 selfplay_games_in_flight=0, buffer_size=None, seed=None, resign='off', resign_disabled_frac=0.1,
                 resign_fp_target=0.05, playout_cap=None, gate_against=None, batch_size=32, updates_per_round=1,
                 device_replay=False, temperature_schedule=None, pi_temperature=None, reanalyse=None, reanalyse_slots=512,
                 reanalyse_playouts=None, game='gomoku', board_width=None, value_mix=0.0, reanalyse_targets='pi',
                 continuous_selfplay=False, score_mode='uct_ref', resident_puct=False, forced_playouts=None):
        """``buffer_size``: length of the replay deque.  None = the reference's 1000 (train_alphazero.py:32) in the
        reference flow; in the batched mode (``selfplay_games_in_flight > 0``) None sizes it to hold ONE collection
        round (games in flight x board cells x 8 symmetries) -- a documented deviation: with the reference's 1000 a
        256-game round (~200 k augmented samples) would keep its last 1000 samples and drop > 99 % of what the GPU
        produced.  Pass 1000 to get the reference's number in either mode.  ``seed``: of the batched mode's move draws
        (uniforms keyed (seed, game id, ply)); None = drawn on rank 0.  Under a launcher (RANK / WORLD_SIZE set, or an
        initialised process group) the pipeline is one of the ranks: see the module docstring.
        ``resign``: self-play resignation (BatchedSelfPlay.set_resign; batched mode only, an opt-in extension): 'off', a threshold,
        or 'auto' -- the first round all calibration games with threshold -inf (statistics only), then after every round rank 0
        sets the threshold from the calibration games of the last rounds (selfplay.calibrate_resign_threshold, at most
        ``resign_fp_target`` false positives) and hands it to every rank.  ``resign_disabled_frac``: the calibration games.
        ``playout_cap``: None or (n_fast, p_full) -- playout cap randomization (BatchedSelfPlay.set_playout_cap; batched mode only, an
        opt-in extension): the replay buffer takes the plies searched with the full budget (Trajectory.training_samples).
        ``gate_against``: None or a checkpoint (batched mode only): at every ``check_freq`` the current network plays a match from
        paired openings against it (rlzero_amd.match) and the score is printed next to the pure-MCTS win ratio; nothing is decided
        on it.
        ``batch_size`` / ``updates_per_round``: entries per mini-batch and ``policy_update`` calls per collection round (the
        reference's 32 and 1, train_alphazero.py:33,130-131), for either buffer.  ``device_replay`` (batched mode on a GPU only, an
        opt-in extension): rank 0's ``data_buffer`` is a ``rlzero_amd.replay.DeviceReplay`` -- the finished games go to device
        memory from their move lists, a mini-batch is one launch (``sample``: drawn on the device WITH replacement, keyed (seed,
        update)), and the KL / explained variances of ``policy_update`` are computed on the device.
        ``temperature_schedule``: None or what --temperature-schedule parses to, ('step', t_early, n_plies, t_late) or ('decay',
        t_start, t_end, halflife) -- a per-ply move temperature (BatchedSelfPlay.set_temperature_schedule; batched mode only, an
        opt-in extension); ``pi_temperature``: None (the stored pi at the ply's T, the reference's rule) or the T of the stored pi.
        ``reanalyse`` (needs ``device_replay``, an opt-in extension): None / 0 = off -- nothing is allocated or launched --, N or
        'all': before every round's updates rank 0 searches N drawn positions of the buffer (or all of them) again with the
        current network and rewrites their pi rows (rlzero_amd.replay.ReplayReanalyser: the visit distribution at T = 1, z and
        the boards untouched); ``reanalyse_slots`` positions per search batch, ``reanalyse_playouts`` simulations each (None:
        ``n_playout``).
        ``game``: 'gomoku' or 'connect4' -- Connect4 on ``board_size`` rows x ``board_width`` columns (default 7), an action is a
        column; batched mode on one rank only, without a gate match (the reference flow's GameControl and rlzero_amd.match are
        Gomoku's); both replay buffers hold its two symmetries (ReplayBuffer).
        ``value_mix`` = lam in [0, 1] (batched mode on one rank, either buffer, both games; an opt-in extension): 0 = off -- nothing
        is allocated, launched or stored differently --; lam > 0: self-play keeps the root value q of every search
        (BatchedSelfPlay.set_root_values) and the learner's value target is (1 - lam) z + lam q (rlzero_amd.replay.mixed_value_targets:
        DeviceReplay.set_value_mix, or Trajectory.training_samples(value_mix=) into the host buffer).  ValueError with several
        ranks: the ranks' payload carries no root values.  ``reanalyse_targets``: 'pi' (default), 'value' or 'both' -- what a refresh
        rewrites (ReplayReanalyser(targets=)); 'value' / 'both' need ``value_mix`` > 0, whose buffer keeps q.
        ``continuous_selfplay`` (batched mode on one rank with the move step on the device; an opt-in extension -- NOT the reference's
        loop, which collects and then updates): self-play is ONE stream (BatchedSelfPlay.stream_start) that the rounds do not stop.  A
        round is ``stream_collect(n)`` behind ``refresh_weights()``: it ends when n more games have finished, and the games still
        running go on under the next round's weights (Trajectory.epochs tells which plies) instead of idling their slots' neighbours.
        The replay buffer receives the games in FINISHING order, not in game-id order.  The last round of ``run`` stops the stream and
        prints the games it drops.  ValueError with several ranks, with RZ_TRAIN_HOST_MOVES=1 and in the reference flow.
        ``score_mode`` (batched mode; governs SELF-PLAY only -- evaluation games and the gate match keep their engines): 'uct_ref'
        (default, the reference's rule) or 'puct', the rule that reads the policy head; ``resident_puct``: its one-launch resident
        search (BatchedSelfPlay.for_network(resident_puct=True): boards of up to 10 rows); ``forced_playouts``: None or k > 0 --
        forced playouts and policy target pruning (BatchedSelfPlay.set_forced_playouts: the stored pis come from the pruned counts).
        ValueError: 'puct' with a playout cap, Reanalyse or continuous self-play (all three are uct_ref's today), resident_puct or
        forced_playouts without 'puct'.  Several ranks are served: the payload they gather carries the pis as they are."""
        check_puct_options(score_mode, resident_puct, forced_playouts, selfplay_games_in_flight, playout_cap, reanalyse, continuous_selfplay)
        self.score_mode, self.resident_puct = score_mode, bool(resident_puct)
        self.forced_playouts = None if forced_playouts is None else float(forced_playouts)
        if game not in ('gomoku', 'connect4'):
            raise ValueError('game %r: gomoku or connect4' % (game, ))
        self.game_kind = game
        if game == 'connect4':
            if selfplay_games_in_flight <= 0:
                raise ValueError('Connect4 is a batched-mode game: selfplay_games_in_flight must be > 0')
            if gate_against is not None:
                raise ValueError('the gate match is a Gomoku option: rlzero_amd.match plays no Connect4')
            self.rows, self.cols = int(board_size), int(7 if board_width is None else board_width)
            board_size = (self.rows, self.cols)
        else:
            if board_width is not None and int(board_width) != int(board_size):
                raise ValueError('a Gomoku board is square: board_width %r with board_size %r' % (board_width, board_size))
            self.rows = self.cols = board_size
        self.n_cells, self.n_symmetries = self.rows * self.cols, 2 if game == 'connect4' else 8
        if (temperature_schedule is not None or pi_temperature is not None) and selfplay_games_in_flight <= 0:
            raise ValueError('the temperature schedule is a batched self-play option: selfplay_games_in_flight must be > 0')
        self.temperature_schedule = None if temperature_schedule is None else temperature_table(temperature_schedule, self.n_cells)
        self.pi_temperature = None if pi_temperature is None else float(pi_temperature)
        if device_replay and selfplay_games_in_flight <= 0:
            raise ValueError('the device replay buffer is a batched-mode option: selfplay_games_in_flight must be > 0')
        if int(batch_size) < 1 or int(updates_per_round) < 1:
            raise ValueError('batch_size and updates_per_round must be >= 1')
        self.device_replay, self.updates_per_round, self._updates = bool(device_replay), int(updates_per_round), 0
        self.reanalyse = reanalyse if reanalyse == 'all' else (int(reanalyse) if reanalyse else None)
        if self.reanalyse is not None and not device_replay:
            raise ValueError('reanalyse needs --device-replay: it refreshes the pi rows of the device replay buffer')
        if self.reanalyse is not None and self.reanalyse != 'all' and self.reanalyse < 0:
            raise ValueError('reanalyse: a number of positions >= 0 or "all"')
        self.reanalyse_slots = int(reanalyse_slots)
        self.reanalyse_playouts = int(n_playout if reanalyse_playouts is None else reanalyse_playouts)
        if self.reanalyse is not None and (self.reanalyse_slots < 1 or self.reanalyse_playouts < 1):
            raise ValueError('reanalyse_slots and reanalyse_playouts must be >= 1')
        self._reanalyser = None
        self.value_mix = float(value_mix)
        if not 0.0 <= self.value_mix <= 1.0:
            raise ValueError('value_mix %r not in [0, 1]' % (value_mix, ))
        if self.value_mix > 0.0 and selfplay_games_in_flight <= 0:
            raise ValueError('the value mix is a batched self-play option: selfplay_games_in_flight must be > 0')
        if reanalyse_targets not in ('pi', 'value', 'both'):
            raise ValueError('reanalyse_targets %r: pi, value or both' % (reanalyse_targets, ))
        if reanalyse_targets != 'pi' and not self.value_mix > 0.0:
            raise ValueError('reanalyse_targets %r refreshes the stored root values: it needs value_mix > 0' % (reanalyse_targets, ))
        self.reanalyse_targets = reanalyse_targets
        if gate_against is not None and selfplay_games_in_flight <= 0:
            raise ValueError('the gate match is a batched-mode option: selfplay_games_in_flight must be > 0')
        self.gate_against, self._gate, self._gate_rounds = gate_against, None, 0
        if playout_cap is not None and selfplay_games_in_flight <= 0:
            raise ValueError('the playout cap is a batched self-play option: selfplay_games_in_flight must be > 0')
        self.playout_cap = None if playout_cap is None else (int(playout_cap[0]), float(playout_cap[1]))
        if resign != 'off' and selfplay_games_in_flight <= 0:
            raise ValueError('resignation is a batched self-play option: selfplay_games_in_flight must be > 0')
        self.rank, self.world = self._init_ranks()
        self.continuous_selfplay = bool(continuous_selfplay)
        if self.continuous_selfplay:
            if selfplay_games_in_flight <= 0:
                raise ValueError('continuous self-play is a batched-mode option: selfplay_games_in_flight must be > 0')
            if self.world > 1:
                raise ValueError('continuous self-play runs on one rank: a stream of games is not sharded (%d ranks)' % self.world)
            if os.environ.get('RZ_TRAIN_HOST_MOVES') == '1':
                raise ValueError('continuous self-play needs the move step on the device (RZ_TRAIN_HOST_MOVES=1 is the host-driven loop)')
        self._final_round = False
        if self.world > 1 and self.value_mix > 0.0:
            raise ValueError('the value mix runs on one rank: the payload the ranks gather carries no root values (%d ranks)' % self.world)
        if self.world > 1 and game == 'connect4':
            raise ValueError('Connect4 trains on one rank: several ranks are a Gomoku option')
        if self.world > 1 and selfplay_games_in_flight <= 0:
            raise ValueError('several ranks share a collection round: selfplay_games_in_flight must be > 0 (games per GPU)')
        self.resign_mode = resign if resign in ('off', 'auto') else float(resign)
        self.resign_disabled_frac, self.resign_fp_target = float(resign_disabled_frac), float(resign_fp_target)
        self.resign_threshold = None if resign == 'off' else float('-inf') if resign == 'auto' else float(resign)
        self._resign_history = []   # calibration games of the last rounds (rank 0, 'auto')
        # board and game
        self.board_size = board_size
        self.n_in_row = n_in_row
        if game == 'connect4':   # (no GameControl: the reference flow is Gomoku's)
            from rlzero_amd.games.connect4.connect4_env import Connect4Env
            self.board, self.game = Connect4Env(self.rows, self.cols, self.n_in_row), None
        else:
            self.board = GomokuEnv(board_size=self.board_size, n_in_row=self.n_in_row)
            self.game = GameControl(self.board)
        # training hyper-parameters (train_alphazero.py:26-41)
        self.learn_rate = 2e-3
        self.lr_multiplier = 1.0
        self.temperature = 1.0
        self.n_playout = n_playout
        self.c_puct = 5
        if buffer_size is None:
            buffer_size = 1000 if selfplay_games_in_flight <= 0 else \
                max(1000, selfplay_games_in_flight * self.world * self.n_cells * self.n_symmetries)
        self.buffer_size = int(buffer_size)
        self.batch_size = int(batch_size)
        # (the reference's deque of augmented samples, the symmetries formed on access: ReplayBuffer)
        self.data_buffer = ReplayBuffer(self.buffer_size, self.board_size, game=game)
        self.play_batch_size = 1
        self.epochs = 5
        self.kl_targ = 0.02
        self.check_freq = check_freq
        self.game_batch_num = game_batch_num
        self.best_win_ratio = 0.0
        self.device = self._pick_device()
        if self.device_replay:
            if self.device.type != 'cuda':
                raise ValueError('the device replay buffer needs a GPU (this process runs on %s)' % (self.device, ))
            if self.rank == 0:   # (rank 0 holds the buffer, as with the host one; sized like the batched mode's default: one round)
                from rlzero_amd.replay import DeviceReplay
                self.data_buffer = DeviceReplay(self.board_size, max(1, self.buffer_size // self.n_symmetries), device=str(self.device), game=game,
                                                search_values=self.value_mix > 0.0)
                self.data_buffer.set_value_mix(self.value_mix)
        self.pure_mcts_playout_num = 100
        self.selfplay_games_in_flight = selfplay_games_in_flight
        if game == 'connect4':
            self.alphazero_agent = AlphaZeroAgent(self.rows, device=self.device, board_width=self.cols, n_actions=self.cols)
        else:
            self.alphazero_agent = AlphaZeroAgent(self.board_size, device=self.device)
        self.mcts_player = AlphaZeroPlayer(self.alphazero_agent.policy_value_fn, n_playout=self.n_playout,
                                           c_puct=self.c_puct, is_selfplay=True)
        self._batched = None
        self._duel, self._duel_key, self._evaluations = None, None, 0
        self._next_game_id = 0
        self._trace_rounds = 0
        self.selfplay_seed = self._agree_on(random.getrandbits(31) if seed is None else int(seed))
        if self.device_replay and self.rank == 0:
            self.data_buffer.seed = self.selfplay_seed   # (the sampler's stream: keyed (seed, update, entry))
        if self.world > 1:   # every rank starts from rank 0's weights
            from rlzero.algorithms import broadcast_weights
            broadcast_weights(self.alphazero_agent.policy_value_net, src=0)

    # ------------------------------------------------------------------ ranks
    @staticmethod
    def _init_ranks():
        """-> (rank, world).  One process per GPU; the process group is RCCL (backend nccl) on GPUs, gloo on the CPU or when
        RZ_DIST_BACKEND says so (two ranks on one GPU: RCCL refuses that)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
        world = int(os.environ.get('WORLD_SIZE', '1'))
        if world <= 1:
            return 0, 1
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        backend = os.environ.get('RZ_DIST_BACKEND', 'nccl' if torch.cuda.is_available() else 'gloo')
        if backend == 'nccl':
            local = 0 if os.environ.get('RZ_DIST_SINGLE_DEVICE') == '1' else int(os.environ.get('LOCAL_RANK', '0'))
            torch.cuda.set_device(local)
            dist.init_process_group('nccl', device_id=torch.device('cuda', local))
        else:
            dist.init_process_group(backend)
        return dist.get_rank(), dist.get_world_size()

    def _pick_device(self):
        if not torch.cuda.is_available():
            return torch.device('cpu')
        if self.world == 1:
            return torch.device('cuda')
        local = 0 if os.environ.get('RZ_DIST_SINGLE_DEVICE') == '1' else int(os.environ.get('LOCAL_RANK', str(self.rank)))
        torch.cuda.set_device(local)
        return torch.device('cuda', local)

    def _agree_on(self, value):
        """rank 0's ``value`` (an int) on every rank."""
        if self.world == 1:
            return value
        import torch.distributed as dist
        on_gpu = dist.get_backend() == 'nccl'
        t = torch.tensor([value], dtype=torch.int64, device=self.device if on_gpu else 'cpu')
        dist.broadcast(t, src=0)
        return int(t.item())

    # ------------------------------------------------------------------ data
    def get_equi_data(self, play_data):
        """8-fold augmentation: [(state, mcts_prob, winner_z), ...] -> 8x as many, in the reference's order (per sample: for
        i = 1..4 the pair rotated by i quarter turns, then its left-right mirror; train_alphazero.py:59-79).  A game's samples are
        turned together -- numpy's rot90 / flip on the stacked arrays, the per-sample results of `_symmetries` (which
        tests/golden/g5_equi.npz pins) as views of them: a 256-game round is 200 k samples, and one numpy call per plane and
        sample was most of what the trainer's collection round cost the host."""
        play_data = list(play_data)
        if not play_data:
            return []
        if getattr(self, 'game_kind', 'gomoku') == 'connect4':   # two symmetries: the sample as played, then its left-right mirror
            extend_data = []
            for state, mcts_prob, winner in play_data:
                state, mcts_prob = np.asarray(state), np.asarray(mcts_prob)
                extend_data.append((state, mcts_prob, winner))
                extend_data.append((np.ascontiguousarray(state[:, :, ::-1]), np.ascontiguousarray(mcts_prob[::-1]), winner))
            return extend_data
        size = self.board_size
        states = np.stack([np.asarray(s_) for s_, _, _ in play_data])                                   # [P, 4, B, B]
        grids = np.stack([np.asarray(p_).reshape(size, size) for _, p_, _ in play_data])                # [P, B, B]
        upside_down = grids[:, ::-1, :]                                                                 # np.flipud per sample
        out_s, out_p = [], []
        for quarter_turns in (1, 2, 3, 4):
            turned = np.rot90(states, quarter_turns, axes=(2, 3))
            pi_turned = np.rot90(upside_down, quarter_turns, axes=(1, 2))
            out_s.append(np.ascontiguousarray(turned))
            out_p.append(np.ascontiguousarray(pi_turned[:, ::-1, :]).reshape(len(play_data), -1))      # flipud, flatten
            out_s.append(np.ascontiguousarray(turned[:, :, :, ::-1]))                                    # fliplr of every plane
            out_p.append(np.ascontiguousarray(pi_turned[:, :, ::-1][:, ::-1, :]).reshape(len(play_data), -1))   # flipud(fliplr)
        extend_data = []
        for j, (_, _, winner) in enumerate(play_data):
            for k in range(8):
                extend_data.append((out_s[k][j], out_p[k][j], winner))
        return extend_data

    def _play_games(self, game_ids, on_finished=None):
        """The trajectories of ``game_ids`` (this rank's share of a round), games in lock-step on this rank's GPU.  ``on_finished``: see
        BatchedSelfPlay.run_device (one rank, the move step on the device: the round's samples are formed while the GPU plays on)."""
        self._selfplay()
        self._batched.refresh_weights()   # (every lane's evaluator: the learner has stepped / new weights have arrived)
        self._set_resign()
        # the move step on the device (rz_play_*: the host reads the games from a log behind the GPU); RZ_TRAIN_HOST_MOVES=1: the
        # host-driven loop -- the same trajectories either way (tests/test_device_moves.py)
        if os.environ.get('RZ_TRAIN_HOST_MOVES') == '1':
            trajs = self._batched.run(game_ids) if len(game_ids) else []
            if on_finished is not None and trajs:
                on_finished(trajs)
        else:
            trajs = self._batched.run_device(game_ids, on_finished=on_finished) if len(game_ids) else []
        if os.environ.get('RZ_TRAIN_TRACE'):
            self._trace_round(trajs)
        return trajs

    def _selfplay(self):
        """The rank's BatchedSelfPlay, built on first use."""
        from rlzero.algorithms import BatchedSelfPlay
        if self._batched is None:
            # one to four lanes of games, whichever fills the GPU better (selfplay.plan_lanes)
            self._batched = BatchedSelfPlay.for_network(
                self.alphazero_agent.policy_value_net, self.board_size, self.n_in_row,
                n_games=self.selfplay_games_in_flight, n_playout=self.n_playout, c_puct=self.c_puct,
                device=str(self.device), temperature=self.temperature, seed=self.selfplay_seed, playout_cap=self.playout_cap,
                temperature_schedule=self.temperature_schedule, pi_temperature=self.pi_temperature,
                root_values=self.value_mix > 0.0, **self._puct_kw(), **self._game_kw())
        return self._batched

    def _set_resign(self):
        if self.resign_mode != 'off':
            # 'auto' before its first calibration: threshold -inf and every game a calibration game (statistics only)
            first = self.resign_mode == 'auto' and not self._resign_history and self.resign_threshold == float('-inf')
            self._batched.set_resign(self.resign_threshold, 1.0 if first else self.resign_disabled_frac)

    def _collect_continuous(self, n_games, consume):
        """One round of continuous self-play: the stream's next ``n_games`` finished games (at least), under the weights and the
        resignation threshold handed over at its start -- a new epoch of the stream; games that started in an earlier round finish
        here, games this round starts may finish in a later one.  ``consume`` takes every game's tuple in FINISHING order while the
        GPU plays on.  The last round of run() stops the stream.  -> [] (every game was consumed)."""
        sp = self._selfplay()
        sp.refresh_weights()
        self._set_resign()
        if not sp._streaming:   # (the first round: the options above are in force when the move step is attached)
            sp.stream_start(first_game_id=self._next_game_id)
        epoch = sp.stream_epoch
        trajs = sp.stream_collect(n_games, on_finished=lambda done: [consume(self._tuple(t)) for t in done])
        self._next_game_id = max([self._next_game_id] + [t.game_id + 1 for t in trajs])
        self._resign_round(trajs)
        self._cap_round(trajs)
        plies = sum(len(t.moves) for t in trajs)
        stale = sum(int((t.epochs < epoch).sum()) for t in trajs)
        print('continuous self-play: {} games finished, {} of {} plies searched in an earlier epoch ({:.3f})'.format(
            len(trajs), stale, plies, stale / max(plies, 1)), flush=True)
        if os.environ.get('RZ_TRAIN_TRACE'):
            self._trace_round(trajs)
        if self._final_round:
            print('continuous self-play: stream stopped, {} running games dropped'.format(sp.stream_stop()), flush=True)
        return []

    def _puct_kw(self):
        """The selection rule of self-play (for_network's keywords; nothing under the default rule)."""
        if self.score_mode != 'puct':
            return {}
        return dict(score_mode='puct', resident_puct=self.resident_puct, forced_playouts=self.forced_playouts)

    def _game_kw(self):
        """What BatchedSelfPlay.for_network / BatchedEvaluation.for_network take beyond Gomoku's defaults."""
        return dict(game='connect4', net_shape=(self.rows, self.cols, self.cols)) if self.game_kind == 'connect4' else {}

    def _trace_round(self, trajs):
        """RZ_TRAIN_TRACE=<directory>: one JSON line per collection round and rank -- a digest of the torch parameters, a digest
        of what every lane's HIP evaluator answers on a fixed batch of positions (i.e. of the weights it was handed), and the
        round's games.  What the multi-rank tests compare: every rank must search with the weights rank 0 learned."""
        import hashlib
        import json
        net = self.alphazero_agent.policy_value_net
        digest = hashlib.sha1()
        for p in net.parameters():
            digest.update(p.detach().cpu().numpy().tobytes())
        rng = np.random.RandomState(7)
        obs = torch.from_numpy((rng.rand(8, 4, self.rows, self.cols) < 0.3).astype(np.float32)).to(self.device)
        answers = []
        for lane in self._batched.lanes:
            with torch.cuda.stream(lane.stream):
                if getattr(lane.evaluator.hip, 'algo', 'split_f16') == 'split_f16_fp8':
                    answers.append('position-fed-only')   # (the opt-in FP8 mode takes no float planes: nothing to digest here)
                    continue
                logp, value = lane.evaluator.hip.forward(obs)
            lane.stream.synchronize()
            answers.append(hashlib.sha1(logp.cpu().numpy().tobytes() + value.cpu().numpy().tobytes()).hexdigest())
        rec = {'rank': self.rank, 'round': self._trace_rounds, 'params': digest.hexdigest(), 'lanes': answers,
               'games': {str(t.game_id): t.moves for t in trajs}}
        self._trace_rounds += 1
        with open(os.path.join(os.environ['RZ_TRAIN_TRACE'], 'rank%d.jsonl' % self.rank), 'a') as f:
            f.write(json.dumps(rec) + '\n')

    def _tuple(self, t):
        """start_self_play's tuple of a trajectory; under a playout cap with the full-budget plies only.  With the device replay
        buffer the trajectory itself: its positions are formed on the device from the move list (DeviceReplay.add)."""
        if self.device_replay:
            return t
        if self.value_mix > 0.0:   # (the mixed value target in z's place; under a cap the full-budget plies, as below)
            return t.winner, t.training_samples(value_mix=self.value_mix)
        return t.as_reference_tuple() if self.playout_cap is None else (t.winner, t.training_samples())

    def _cap_round(self, trajs):
        """After a collection round under a playout cap (``trajs``: None off rank 0): the share of plies searched with the full budget."""
        if self.playout_cap is None or trajs is None:
            return
        plies = sum(len(t.moves) for t in trajs)
        full = sum(int(t.full[:len(t.moves)].sum()) for t in trajs)
        print('playout cap: {} of {} plies searched with the full budget ({:.3f}); n_fast {}, p_full {}'.format(
            full, plies, full / max(plies, 1), *self.playout_cap), flush=True)

    def _collect_batched(self, n_games, consume=None):
        """One collection round: ``n_games`` games in all, game g played by rank g mod world (selfplay.shard_game_ids),
        one gather to rank 0 (pi as float32: what the learner consumes).  -> start_self_play's tuples on rank 0, in game
        id order; [] on the other ranks.  ``consume`` (one rank): called with every game's tuple IN GAME-ID ORDER as soon as the game
        and all games before it have ended -- while the GPU plays the others --; the tuples it took are not returned."""
        from rlzero.algorithms import gather_trajectories
        ids = range(self._next_game_id, self._next_game_id + n_games)
        self._next_game_id += n_games
        if self.world > 1:
            local = self._play_games([g for g in ids if g % self.world == self.rank])
            merged = gather_trajectories(local, self.board_size, self.n_in_row, dst=0, pi_dtype=np.float32)
            self._resign_round(merged)
            self._cap_round(merged)
            return [self._tuple(t) for t in merged] if merged is not None else []
        # one rank: every finished game becomes start_self_play's tuple (planes from its move list) WHILE the others are played --
        # behind an idle GPU that was a tenth of a round; the round's order stays the game ids'
        ready, cursor = {}, [ids.start]

        def take(trajs):
            for t in trajs:
                ready[t.game_id] = self._tuple(t)
            while consume is not None and cursor[0] in ready:   # (the replay buffer's order is the reference's: game by game)
                consume(ready.pop(cursor[0]))
                cursor[0] += 1
        local = self._play_games(list(ids), on_finished=take)
        self._resign_round(local)
        self._cap_round(local)
        self._forced_round(local)
        rest = [t for t in sorted(local, key=lambda t: t.game_id) if t.game_id >= cursor[0] or consume is None]
        return [ready[t.game_id] if t.game_id in ready else self._tuple(t) for t in rest]

    def _forced_round(self, trajs):
        """After a collection round under forced playouts (one rank: the gathered payload carries no raw counts): what policy target
        pruning took out of the round's targets."""
        if self.forced_playouts is None or not trajs or any(t.raw_visits is None for t in trajs):
            return
        raw = np.concatenate([t.raw_visits for t in trajs], axis=0)
        pis = np.concatenate([np.asarray(t.pis) for t in trajs], axis=0)
        print('forced playouts: k {:g}, {} plies, {} of {} visited root children without weight in the pruned target'.format(
            self.forced_playouts, len(raw), int(((raw > 0) & (pis < 1e-9)).sum()), int((raw > 0).sum())), flush=True)

    RESIGN_ROUNDS = 4   # 'auto': rounds of calibration games the threshold is set from

    def _resign_round(self, trajs):
        """After a collection round (``trajs``: every rank's games on rank 0, None elsewhere): rank 0 prints the round's
        resignations, the calibration games' false-positive rate at the threshold played and -- 'auto' -- sets the next threshold,
        which every rank takes."""
        if self.resign_mode == 'off':
            return
        from rlzero.algorithms import calibrate_resign_threshold
        if trajs is not None:
            calib = [t for t in trajs if t.no_resign]
            played = self.resign_threshold
            fp = np.mean([t.fp_margin < played for t in calib]) if calib else float('nan')
            if self.resign_mode == 'auto':
                self._resign_history = (self._resign_history + [calib])[-self.RESIGN_ROUNDS:]
                self.resign_threshold = calibrate_resign_threshold([t for r in self._resign_history for t in r], self.resign_fp_target)
            print('resign: {} of {} games resigned, calibration false positives {:.3f} of {} at threshold {:.4f}; next threshold {:.4f}'.format(
                sum(t.resigned for t in trajs), len(trajs), fp, len(calib), played, self.resign_threshold), flush=True)
        if self.world > 1 and self.resign_mode == 'auto':   # rank 0's threshold on every rank
            import torch.distributed as dist
            on_gpu = dist.get_backend() == 'nccl'
            t = torch.tensor([self.resign_threshold], dtype=torch.float64, device=self.device if on_gpu else 'cpu')
            dist.broadcast(t, src=0)
            self.resign_threshold = float(t.item())
            self._resign_history = self._resign_history or [[]]   # (past the first round on every rank)

    def collect_selfplay_data(self, n_games=1):
        """collect self-play data for training."""
        pending = []   # (device replay: the round's games, one DeviceReplay.add for all of them)

        def consume(game):
            if self.device_replay:
                plies = len(game.moves)
                self.episode_len = plies if game.full is None else int(game.full[:plies].sum())
                pending.append(game)
                return
            winner, play_data = game
            play_data = list(play_data)
            self.episode_len = len(play_data)
            if os.environ.get('RZ_TRAIN_EAGER_SYMMETRIES') == '1':   # (the eight symmetries of every sample up front, as before round 6)
                self.data_buffer.extend(self.get_equi_data(play_data))
            else:
                self.data_buffer.extend_samples(play_data)
        if self.continuous_selfplay:
            games = self._collect_continuous(max(n_games, self.selfplay_games_in_flight), consume)
        elif self.selfplay_games_in_flight > 0:
            games = self._collect_batched(max(n_games, self.selfplay_games_in_flight * self.world), consume=consume)
        else:
            games = [self.game.start_self_play(self.mcts_player, temperature=self.temperature)
                     for _ in range(n_games)]
        for game in games:
            consume(game)
        if pending:
            self.data_buffer.add(pending)

    # ------------------------------------------------------------------ learning
    def _policy_update_device(self):
        """policy_update with the device replay buffer: the mini-batch is one launch into device tensors (drawn on the device, keyed
        (seed, update counter)), the KL and the explained variances stay on the device -- one .item() per value the host decides on
        or prints (the KL of every epoch: the early stop)."""
        state_batch, mcts_probs_batch, winner_batch = self.data_buffer.sample(self.batch_size, step=self._updates)
        self._updates += 1
        net = self.alphazero_agent.policy_value_net

        def policy_value(states):   # (AlphaZeroAgent.policy_value without the host copy)
            log_probs, value = net(states)
            return torch.exp(log_probs.detach()), value.detach()
        old_probs, old_v = policy_value(state_batch)
        for _ in range(self.epochs):
            loss, entropy = self.alphazero_agent.learn(state_batch, mcts_probs_batch, winner_batch)
            new_probs, new_v = policy_value(state_batch)
            kl = torch.mean(torch.sum(old_probs * (torch.log(old_probs + 1e-10) - torch.log(new_probs + 1e-10)), dim=1)).item()
            if kl > self.kl_targ * 4:  # early stopping if D_KL diverges badly
                break
        if kl > self.kl_targ * 2 and self.lr_multiplier > 0.1:
            self.lr_multiplier /= 1.5
        elif kl < self.kl_targ / 2 and self.lr_multiplier < 10:
            self.lr_multiplier *= 1.5
        var_z = torch.var(winner_batch, unbiased=False)
        explained_var_old = (1 - torch.var(winner_batch - old_v.flatten(), unbiased=False) / var_z).item()
        explained_var_new = (1 - torch.var(winner_batch - new_v.flatten(), unbiased=False) / var_z).item()
        print(('kl:{:.5f},'
               'lr_multiplier:{:.3f},'
               'loss:{},'
               'entropy:{},'
               'explained_var_old:{:.3f},'
               'explained_var_new:{:.3f}').format(kl, self.lr_multiplier, loss, entropy, explained_var_old,
                                                  explained_var_new))
        return loss, entropy

    def reanalyse_round(self):
        """Before a round's updates (rank 0, ``reanalyse`` on): stored positions searched again with the network as it is now, their
        pi rows rewritten in the device replay buffer.  -> positions refreshed."""
        if self.reanalyse is None or len(self.data_buffer) == 0:
            return 0
        if self._reanalyser is None:
            from rlzero_amd.replay import ReplayReanalyser
            self._reanalyser = ReplayReanalyser(self.alphazero_agent.policy_value_net, self.data_buffer, self.n_in_row,
                                                self.reanalyse_playouts, slots=self.reanalyse_slots, c_puct=self.c_puct,
                                                seed=self.selfplay_seed, targets=self.reanalyse_targets)
        self._reanalyser.refresh_weights()
        done = self._reanalyser.reanalyse_all() if self.reanalyse == 'all' else self._reanalyser.reanalyse_sample(self.reanalyse)
        self._reanalyser.check()
        return done

    def policy_update(self):
        """update the policy-value net."""
        if self.device_replay:
            return self._policy_update_device()
        mini_batch = random.sample(self.data_buffer, self.batch_size)
        state_batch, mcts_probs_batch, winner_batch = (list(col) for col in zip(*mini_batch))
        old_probs, old_v = self.alphazero_agent.policy_value(state_batch)
        for _ in range(self.epochs):
            loss, entropy = self.alphazero_agent.learn(state_batch, mcts_probs_batch, winner_batch)
            new_probs, new_v = self.alphazero_agent.policy_value(state_batch)
            kl = np.mean(np.sum(old_probs * (np.log(old_probs + 1e-10) - np.log(new_probs + 1e-10)), axis=1))
            if kl > self.kl_targ * 4:  # early stopping if D_KL diverges badly
                break
        if kl > self.kl_targ * 2 and self.lr_multiplier > 0.1:
            self.lr_multiplier /= 1.5
        elif kl < self.kl_targ / 2 and self.lr_multiplier < 10:
            self.lr_multiplier *= 1.5
        z = np.array(winner_batch)
        explained_var_old = 1 - np.var(z - old_v.flatten()) / np.var(z)
        explained_var_new = 1 - np.var(z - new_v.flatten()) / np.var(z)
        print(('kl:{:.5f},'
               'lr_multiplier:{:.3f},'
               'loss:{},'
               'entropy:{},'
               'explained_var_old:{:.3f},'
               'explained_var_new:{:.3f}').format(kl, self.lr_multiplier, loss, entropy, explained_var_old,
                                                  explained_var_new))
        return loss, entropy

    def _evaluate_batched(self, n_games):
        """The ``n_games`` evaluation games in lock-step on this GPU (rlzero_amd.evaluate.BatchedEvaluation: per game what
        start_play does with the two players below) -> their winner ids."""
        from rlzero.algorithms import BatchedEvaluation
        key = (n_games, self.pure_mcts_playout_num)
        if self._duel is None or self._duel_key != key:
            if self._duel is not None:
                self._duel.close()
            self._duel = BatchedEvaluation.for_network(
                self.alphazero_agent.policy_value_net, self.board_size, self.n_in_row, n_games=n_games,
                n_playout=self.n_playout, rollout_playouts=self.pure_mcts_playout_num, c_puct=self.c_puct, rollout_c_puct=5,
                device=str(self.device), seed=self.selfplay_seed, **self._game_kw())
            self._duel_key = key
        self._duel.refresh_weights()
        self._duel.seed = (self.selfplay_seed + 0x9E37 * self._evaluations) & 0x7fffffff   # fresh draws every evaluation
        self._evaluations += 1
        return [r.winner for r in self._duel.run()]

    def policy_evaluate(self, n_games=10):
        """Play the current policy against the pure-MCTS opponent (monitoring only)."""
        if self.selfplay_games_in_flight > 0:
            win_cnt = defaultdict(int)
            for winner in self._evaluate_batched(n_games):
                win_cnt[winner] += 1
            win_ratio = 1.0 * (win_cnt[1] + 0.5 * win_cnt[-1]) / n_games
            print('num_playouts:{}, win: {}, lose: {}, tie:{}'.format(self.pure_mcts_playout_num, win_cnt[1],
                                                                      win_cnt[2], win_cnt[-1]))
            return win_ratio
        current_mcts_player = AlphaZeroPlayer(self.alphazero_agent.policy_value_fn, n_playout=self.n_playout,
                                              c_puct=self.c_puct)
        pure_mcts_player = RolloutPlayer(n_playout=self.pure_mcts_playout_num, c_puct=5)
        win_cnt = defaultdict(int)
        for i in range(n_games):
            winner = self.game.start_play(current_mcts_player, pure_mcts_player, start_player=i % 2, is_shown=0)
            win_cnt[winner] += 1
        win_ratio = 1.0 * (win_cnt[1] + 0.5 * win_cnt[-1]) / n_games
        print('num_playouts:{}, win: {}, lose: {}, tie:{}'.format(self.pure_mcts_playout_num, win_cnt[1],
                                                                  win_cnt[2], win_cnt[-1]))
        return win_ratio

    def gate_match(self, n_pairs=8, n_openings=4, opening_plies=2):
        """The current network (A) against the ``gate_against`` checkpoint (B): ``n_pairs`` pairs from ``n_openings`` fresh openings
        -> the score (rlzero_amd.match.score).  Monitoring only."""
        from rlzero_amd.match import BatchedMatch, load_checkpoint, paired_openings, score
        if self._gate is None:
            opponent = load_checkpoint(self.gate_against, self.board_size, str(self.device))
            self._gate = BatchedMatch.for_networks(self.alphazero_agent.policy_value_net, opponent, self.board_size, self.n_in_row,
                                                   n_games=2 * n_pairs, n_playout=self.n_playout, c_puct=self.c_puct,
                                                   device=str(self.device), seed=self.selfplay_seed)
        self._gate.refresh_weights()
        self._gate.seed = (self.selfplay_seed + 0x9E37 * self._gate_rounds) & 0x7fffffff   # fresh openings and draws every time
        self._gate_rounds += 1
        openings = paired_openings(self.board_size, self.n_in_row, n_openings, opening_plies, self._gate.seed)
        s = score(self._gate.run(n_pairs, openings))
        print('gate against {}: score: {:.3f}, win: {}, lose: {}, tie: {}, elo: {:+.0f}'.format(
            self.gate_against, s['a_score'], s['a_wins'], s['b_wins'], s['ties'], s['elo_diff']))
        return s

    def _sync_weights(self):
        """After rank 0's policy_update: its parameters on every rank (one broadcast; nothing to do in one process)."""
        if self.world > 1:
            from rlzero.algorithms import broadcast_weights
            broadcast_weights(self.alphazero_agent.policy_value_net, src=0)

    def run(self):
        """run the training pipeline."""
        lead = self.rank == 0   # rank 0 holds the buffer, learns, evaluates, saves and prints; the others play their share
        try:
            for i in range(self.game_batch_num):
                self._final_round = i + 1 == self.game_batch_num   # (continuous self-play: this round stops the stream)
                self.collect_selfplay_data(self.play_batch_size)
                if lead:
                    print('batch i:{}, episode_len:{}'.format(i + 1, self.episode_len))
                    if len(self.data_buffer) > self.batch_size:
                        self.reanalyse_round()
                        for _ in range(self.updates_per_round):
                            loss, entropy = self.policy_update()
                self._sync_weights()
                if lead and (i + 1) % self.check_freq == 0:
                    print('current self-play batch: {}'.format(i + 1))
                    win_ratio = self.policy_evaluate()
                    if self.gate_against is not None:
                        self.gate_match()
                    self.alphazero_agent.save_model('./current_policy.model')
                    if win_ratio > self.best_win_ratio:
                        print('New best policy!!!!!!!!')
                        self.best_win_ratio = win_ratio
                        self.alphazero_agent.save_model('./best_policy.model')
                        if self.best_win_ratio == 1.0 and self.pure_mcts_playout_num < 5000:
                            self.pure_mcts_playout_num += 1000
                            self.best_win_ratio = 0.0
        except KeyboardInterrupt:
            print('\n\rquit')


def launch_ranks(n):
    """`--gpus n` without a launcher: run this command line under torch.distributed.run as a CHILD process (this process
    never touches the GPU); returns its exit code."""
    import socket
    import subprocess
    with socket.socket() as s_:
        s_.bind(('127.0.0.1', 0))
        port = s_.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr',
           '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def check_puct_options(score_mode, resident_puct, forced_playouts, games_in_flight, playout_cap, reanalyse, continuous_selfplay):
    """ValueError for a combination of the self-play rule's options that no route serves (TrainPipeline, main)."""
    if score_mode not in ('uct_ref', 'puct'):
        raise ValueError('score_mode %r: uct_ref or puct' % (score_mode, ))
    if score_mode != 'puct':
        if resident_puct:
            raise ValueError('--resident-puct is a route of --score-mode puct')
        if forced_playouts is not None:
            raise ValueError('--forced-playouts is a rule of --score-mode puct')
        return
    if games_in_flight <= 0:
        raise ValueError('--score-mode puct is a batched self-play option: --games-in-flight must be > 0')
    if playout_cap is not None:
        raise ValueError('--score-mode puct with --playout-cap: the playout cap is served by the uct_ref search only')
    if reanalyse:
        raise ValueError('--score-mode puct with --reanalyse: Reanalyse searches by uct_ref only')
    if continuous_selfplay:
        raise ValueError('--score-mode puct with --continuous-selfplay: continuous self-play is served by the uct_ref search only')
    if forced_playouts is not None and not (np.isfinite(forced_playouts) and forced_playouts > 0.0):
        raise ValueError('--forced-playouts K: a finite K > 0, not %r' % (forced_playouts, ))


def playout_cap_arg(text):
    """--playout-cap N_FAST:P_FULL -> (n_fast, p_full)."""
    import argparse
    try:
        n_fast, p_full = text.split(':')
        n_fast, p_full = int(n_fast), float(p_full)
    except ValueError:
        raise argparse.ArgumentTypeError('N_FAST:P_FULL, e.g. 100:0.25, not %r' % text)
    if n_fast < 1 or not 0.0 < p_full <= 1.0:
        raise argparse.ArgumentTypeError('N_FAST >= 1 and P_FULL in (0, 1], not %r' % text)
    return n_fast, p_full


def temperature_schedule_arg(text):
    """--temperature-schedule step:T_EARLY:N:T_LATE | decay:T_START:T_END:HALFLIFE -> ('step', t_early, n, t_late) or ('decay', t_start,
    t_end, halflife)."""
    import argparse
    form = 'step:T_EARLY:N:T_LATE or decay:T_START:T_END:HALFLIFE'
    parts = text.split(':')
    try:
        if parts[0] == 'step' and len(parts) == 4:
            spec = ('step', float(parts[1]), int(parts[2]), float(parts[3]))
            ok = spec[2] >= 0 and all(np.isfinite(t) and t > 0.0 for t in (spec[1], spec[3]))
        elif parts[0] == 'decay' and len(parts) == 4:
            spec = ('decay', float(parts[1]), float(parts[2]), float(parts[3]))
            ok = all(np.isfinite(t) for t in spec[1:]) and spec[1] > 0.0 and spec[2] >= 0.0 and spec[3] > 0.0
        else:
            raise ValueError(text)
    except ValueError:
        raise argparse.ArgumentTypeError('%s, e.g. step:1.0:30:0.001, not %r' % (form, text))
    if not ok:
        raise argparse.ArgumentTypeError('%s with finite positive temperatures and half-life (T_END may be 0), N >= 0, not %r' % (form, text))
    return spec


def temperature_table(spec, n_cells):
    """The table of a parsed --temperature-schedule for a board of ``n_cells`` cells (a game has no more plies)."""
    from rlzero_amd.selfplay import decay_schedule, step_schedule
    if spec[0] == 'step':
        if spec[2] + 1 > n_cells:
            raise ValueError('temperature schedule: N = %d early plies, the board has %d cells' % (spec[2], n_cells))
        return step_schedule(spec[1], spec[2], spec[3])
    return decay_schedule(spec[1], spec[2], spec[3], n_cells)


def reanalyse_arg(text):
    """--reanalyse N | all -> N (0 = off) or 'all'."""
    import argparse
    if text == 'all':
        return 'all'
    try:
        value = int(text)
    except ValueError:
        value = -1
    if value < 0:
        raise argparse.ArgumentTypeError('a number of positions >= 0 or "all", not %r' % text)
    return value


def positive_float_arg(text):
    import argparse
    try:
        value = float(text)
    except ValueError:
        value = float('nan')
    if not (np.isfinite(value) and value > 0.0):
        raise argparse.ArgumentTypeError('a finite positive number, not %r' % text)
    return value


def value_mix_of(args):
    """--value-mix of parsed arguments (0.0 when it was not given)."""
    return float(getattr(args, 'value_mix', 0.0))


def reanalyse_targets_of(args):
    """--reanalyse-targets of parsed arguments ('pi' when it was not given)."""
    return getattr(args, 'reanalyse_targets', 'pi')


def puct_options_of(args):
    """-> (--score-mode, --resident-puct, --forced-playouts) of parsed arguments ('uct_ref', False, None where they were not given)."""
    return getattr(args, 'score_mode', 'uct_ref'), getattr(args, 'resident_puct', False), getattr(args, 'forced_playouts', None)


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='AlphaZero training for Gomoku (or, --game connect4, Connect4) on MI355X (no arguments: the reference script\'s run)')
    ap.add_argument('--gpus', type=int, default=1, help='processes (one per GPU); > 1 without a launcher starts them itself')
    ap.add_argument('--game', choices=('gomoku', 'connect4'), default='gomoku',
                    help='connect4: batched mode on one GPU only (needs --games-in-flight > 0; no --gate-against)')
    ap.add_argument('--board', type=int, default=6, help='rows of the board (Gomoku: rows and columns)')
    ap.add_argument('--board-width', type=int, default=None, metavar='W', help='connect4 only: columns of the board (default 7)')
    ap.add_argument('--n-in-row', type=int, default=4)
    ap.add_argument('--playouts', type=int, default=400)
    ap.add_argument('--batches', type=int, default=64, help='game_batch_num')
    ap.add_argument('--check-freq', type=int, default=50)
    ap.add_argument('--games-in-flight', type=int, default=0, help='per GPU; 0 = the reference flow, one game at a time')
    ap.add_argument('--seed', type=int, default=None)
    ap.add_argument('--resign-threshold', default='off',
                    help="self-play resignation (batched mode only): off, auto (calibrated every round) or a value threshold")
    ap.add_argument('--resign-disabled-frac', type=float, default=0.1, help='games played out to measure false positives')
    ap.add_argument('--resign-fp-target', type=float, default=0.05, help="'auto': false-positive rate the threshold allows")
    ap.add_argument('--playout-cap', type=playout_cap_arg, default=None, metavar='N_FAST:P_FULL',
                    help='playout cap randomization (batched mode only): a search has --playouts simulations with probability P_FULL, '
                         'else N_FAST; only the full ones become policy samples')
    ap.add_argument('--temperature-schedule', type=temperature_schedule_arg, default=None, metavar='step:T_EARLY:N:T_LATE | decay:T_START:T_END:HALFLIFE',
                    help='batched mode only: the move temperature by ply -- T_EARLY for the first N plies, then T_LATE; or T_END + '
                         '(T_START - T_END) * 0.5 ** (ply / HALFLIFE).  Default: one temperature, the reference\'s run')
    ap.add_argument('--pi-temperature', type=positive_float_arg, default=None, metavar='T',
                    help='batched mode only: the stored policy targets at this temperature (default: at the temperature of the move)')
    ap.add_argument('--gate-against', default=None, metavar='CKPT',
                    help='batched mode only: at every --check-freq also report the match score of the current network against this '
                         'checkpoint (paired openings; nothing is decided on it)')
    ap.add_argument('--batch-size', type=int, default=32, help='entries of a mini-batch')
    ap.add_argument('--updates-per-round', type=int, default=1, help='policy updates after every collection round')
    ap.add_argument('--device-replay', action='store_true',
                    help='batched mode on a GPU only: the replay buffer lives in device memory and a mini-batch is one kernel launch '
                         '(drawn on the device, with replacement)')
    ap.add_argument('--reanalyse', type=reanalyse_arg, default=0, metavar='N|all',
                    help='with --device-replay: before every round\'s updates search N drawn positions of the buffer (or all) again '
                         'with the current network and refresh their policy targets (visit distribution at T = 1; z is kept)')
    ap.add_argument('--reanalyse-slots', type=int, default=512, metavar='G', help='positions searched per batch of a refresh')
    ap.add_argument('--reanalyse-playouts', type=int, default=None, metavar='P', help='simulations of a refreshing search (default: --playouts)')
    # (the two options below stay out of the namespace unless given -- argparse.SUPPRESS: value_mix_of / reanalyse_targets_of read them)
    ap.add_argument('--value-mix', type=float, default=argparse.SUPPRESS, metavar='L',
                    help='batched mode on one GPU: the value target (1 - L) z + L q, q the root value of the search that played the ply '
                         '(kept by self-play); 0 = z alone, the default')
    ap.add_argument('--reanalyse-targets', choices=('pi', 'value', 'both'), default=argparse.SUPPRESS,
                    help='with --reanalyse: refresh the policy targets, the stored root values q (needs --value-mix > 0) or both')
    ap.add_argument('--continuous-selfplay', action='store_true', default=argparse.SUPPRESS,   # (absent without the flag, like --value-mix)
                    help='batched mode on one GPU (an opt-in extension, not the reference loop): self-play is one stream that the rounds do '
                         'not stop -- a round ends when --games-in-flight more games have finished, the others run on under the next weights')
    # (the three options below stay out of the namespace unless given, like --value-mix: puct_options_of reads them)
    ap.add_argument('--score-mode', choices=('uct_ref', 'puct'), default=argparse.SUPPRESS,
                    help="batched mode: the selection rule of SELF-PLAY (evaluation games and --gate-against keep theirs); 'puct' reads the "
                         'policy head (with --playout-cap, --reanalyse or --continuous-selfplay: an error); default uct_ref')
    ap.add_argument('--resident-puct', action='store_true', default=argparse.SUPPRESS, help='with --score-mode puct: the one-launch resident search (boards of up to 10 rows)')
    ap.add_argument('--forced-playouts', type=float, default=argparse.SUPPRESS, metavar='K',
                    help='with --score-mode puct: forced playouts at the root (KataGo: K = 2) and policy target pruning of the stored pis')
    args = ap.parse_args(argv)
    value_mix, targets = value_mix_of(args), reanalyse_targets_of(args)
    if not 0.0 <= value_mix <= 1.0:
        ap.error('--value-mix: L in [0, 1]')
    if value_mix > 0.0 and args.games_in_flight <= 0:
        ap.error('--value-mix needs --games-in-flight > 0 (batched self-play)')
    if targets != 'pi' and not args.reanalyse:
        ap.error('--reanalyse-targets needs --reanalyse')
    if targets != 'pi' and not value_mix > 0.0:
        ap.error('--reanalyse-targets %s refreshes the stored root values: it needs --value-mix > 0' % targets)
    if args.game == 'connect4':
        if args.board_width is None:
            args.board_width = 7
        if args.games_in_flight <= 0:
            ap.error('--game connect4 needs --games-in-flight > 0 (batched mode)')
        if args.gate_against is not None:
            ap.error('--gate-against is a Gomoku option: matches play no Connect4')
        if args.gpus > 1:
            ap.error('--game connect4 runs on one GPU')
    elif args.board_width is not None:
        ap.error('--board-width is a Connect4 option (--game connect4)')
    n_cells = args.board * (args.board_width if args.game == 'connect4' else args.board)
    if args.batch_size < 1 or args.updates_per_round < 1:
        ap.error('--batch-size and --updates-per-round must be >= 1')
    if args.reanalyse and not args.device_replay:
        ap.error('--reanalyse needs --device-replay')
    if args.reanalyse and args.games_in_flight <= 0:
        ap.error('--reanalyse needs --games-in-flight > 0 (batched mode)')
    if args.reanalyse and (args.reanalyse_slots < 1 or (args.reanalyse_playouts is not None and args.reanalyse_playouts < 1)):
        ap.error('--reanalyse-slots and --reanalyse-playouts must be >= 1')
    if args.device_replay and args.games_in_flight <= 0:
        ap.error('--device-replay needs --games-in-flight > 0 (batched mode)')
    if args.device_replay and not torch.cuda.is_available():
        ap.error('--device-replay needs a GPU')
    if args.gate_against is not None and args.games_in_flight <= 0:
        ap.error('--gate-against needs --games-in-flight > 0 (batched mode)')
    if args.playout_cap is not None and args.games_in_flight <= 0:
        ap.error('--playout-cap needs --games-in-flight > 0 (batched self-play)')
    if args.playout_cap is not None and args.playout_cap[0] > args.playouts:
        ap.error('--playout-cap: N_FAST %d exceeds --playouts %d' % (args.playout_cap[0], args.playouts))
    if args.temperature_schedule is not None and args.games_in_flight <= 0:
        ap.error('--temperature-schedule needs --games-in-flight > 0 (batched self-play)')
    if args.pi_temperature is not None and args.games_in_flight <= 0:
        ap.error('--pi-temperature needs --games-in-flight > 0 (batched self-play)')
    if args.temperature_schedule is not None and args.temperature_schedule[0] == 'step' and args.temperature_schedule[2] + 1 > n_cells:
        ap.error('--temperature-schedule: N = %d early plies, the board has %d cells' % (args.temperature_schedule[2], n_cells))
    if args.resign_threshold != 'off' and args.games_in_flight <= 0:
        ap.error('--resign-threshold needs --games-in-flight > 0 (batched self-play)')
    if args.resign_threshold not in ('off', 'auto'):
        try:
            float(args.resign_threshold)
        except ValueError:
            ap.error('--resign-threshold: off, auto or a number, not %r' % args.resign_threshold)
    return args


def main(argv=None):
    args = parse_args(argv)
    score_mode, resident_puct, forced_playouts = puct_options_of(args)
    check_puct_options(score_mode, resident_puct, forced_playouts, args.games_in_flight, args.playout_cap, args.reanalyse,
                       getattr(args, 'continuous_selfplay', False))
    if value_mix_of(args) > 0.0 and (args.gpus > 1 or int(os.environ.get('WORLD_SIZE', '1')) > 1):
        raise ValueError('--value-mix runs on one rank: the payload the ranks gather carries no root values (--gpus %d, WORLD_SIZE %s)'
                         % (args.gpus, os.environ.get('WORLD_SIZE', '1')))
    if getattr(args, 'continuous_selfplay', False):
        if args.gpus > 1 or int(os.environ.get('WORLD_SIZE', '1')) > 1:
            raise ValueError('--continuous-selfplay runs on one rank: a stream of games is not sharded (--gpus %d, WORLD_SIZE %s)'
                             % (args.gpus, os.environ.get('WORLD_SIZE', '1')))
        if args.games_in_flight <= 0:
            raise ValueError('--continuous-selfplay needs --games-in-flight > 0 (batched self-play)')
        if os.environ.get('RZ_TRAIN_HOST_MOVES') == '1':
            raise ValueError('--continuous-selfplay needs the move step on the device (RZ_TRAIN_HOST_MOVES=1 is the host-driven loop)')
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    if args.seed is not None:   # a reproducible run: initial weights, random.sample of the replay buffer, numpy draws
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    pipe = TrainPipeline(board_size=args.board, n_in_row=args.n_in_row, n_playout=args.playouts, game_batch_num=args.batches,
                         check_freq=args.check_freq, selfplay_games_in_flight=args.games_in_flight, seed=args.seed,
                         resign=args.resign_threshold, resign_disabled_frac=args.resign_disabled_frac,
                         resign_fp_target=args.resign_fp_target, playout_cap=args.playout_cap, gate_against=args.gate_against,
                         batch_size=args.batch_size, updates_per_round=args.updates_per_round, device_replay=args.device_replay,
                         temperature_schedule=args.temperature_schedule, pi_temperature=args.pi_temperature,
                         reanalyse=args.reanalyse or None, reanalyse_slots=args.reanalyse_slots, reanalyse_playouts=args.reanalyse_playouts,
                         game=args.game, board_width=args.board_width, value_mix=value_mix_of(args), reanalyse_targets=reanalyse_targets_of(args),
                         continuous_selfplay=getattr(args, 'continuous_selfplay', False), score_mode=score_mode,
                         resident_puct=resident_puct, forced_playouts=forced_playouts)
    pipe.run()
    if pipe.world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
