"""Many self-play games in lock-step on one GPU, sharded over GPUs by game id.

Batched counterpart of ``GameControl.start_self_play`` (rlzero/games/gomoku/game.py:96-134)
+ ``AlphaZeroPlayer.get_action`` (rlzero/mcts/alphazero_mcts.py:136-165): every game does
exactly what the reference does for one game -- n_playout simulations from the current
root, pi = softmax(log(N + 1e-10) / T) over the legal moves, a move drawn from pi, tree
reuse, z from the final winner -- but the searches of all games advance together so each
simulation step is ONE batch for the kernels and the network.

Randomness: the reference draws the move with ``numpy.random.choice(acts, p=probs)`` from
the global stream (alphazero_mcts.py:148), i.e. ``acts[searchsorted(cdf, u, 'right')]`` for
the next uniform ``u``.  Here ``u`` comes from a counter-based generator keyed by
(seed, game id, ply), so a game's trajectory does not depend on which GPU plays it or on
how many games share the batch.

Multi-GPU: game ``g`` belongs to rank ``g % world_size``; there is no collective inside
the search.  ``gather_trajectories`` is the single exchange: fixed-stride records to
rank 0 (RCCL when the process group backend is nccl, gloo in the CPU tests).
"""
import collections
import contextlib

import numpy as np

from . import playlog
from . import route as _route
from ._hip import PLAY_FULL, HipError
from ._rng import mix64_u64 as _splitmix64
from .playlog import SlotBook
from .route import fc_in_trunk_pays   # noqa: F401  (a board rule: route.py; importable from here as before)


def move_uniform(seed, game_id, ply):
    """Uniform in [0,1) for (seed, game, ply): 53 high bits of a splitmix64 chain."""
    with np.errstate(over='ignore'):
        x = _splitmix64(np.uint64(seed))
        x = _splitmix64(x ^ np.asarray(game_id, dtype=np.uint64))
        x = _splitmix64(x ^ np.asarray(ply, dtype=np.uint64))
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


_RESIGN_SALT = np.uint64(0x72657369676E0000)   # ("resign": keeps the calibration draw apart from the move and noise streams)


def resign_uniform(seed, game_id):
    """Uniform in [0,1) for (seed, game): a game whose value is below ``disabled_frac`` is a calibration game (resignation disabled;
    the device's resign_uniform, the same bits)."""
    with np.errstate(over='ignore'):
        x = _splitmix64(_splitmix64(np.uint64(seed) ^ _RESIGN_SALT) ^ np.asarray(game_id, dtype=np.uint64))
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


_CAP_SALT = np.uint64(0x706C61796F757400)   # ("playout": the budget draw's own stream)


def cap_uniform(seed, game_id, ply):
    """Uniform in [0,1) for (seed, game, ply) of playout cap randomization: the search before ply ``ply`` of the game has the full
    budget when it is below ``p_full`` (the device's cap_uniform, the same bits)."""
    with np.errstate(over='ignore'):
        x = _splitmix64(np.uint64(seed) ^ _CAP_SALT)
        x = _splitmix64(x ^ np.asarray(game_id, dtype=np.uint64))
        x = _splitmix64(x ^ np.asarray(ply, dtype=np.uint64))
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def fp_margin(resign_stats, winner):
    """The lowest resignation statistic a non-loser saw on their own plies (player 0 moves the even plies; on a tie both players
    count): a calibration game would have been resigned by a player who did not lose at every threshold above it.  NaN statistics
    never fire; NaN when there is no finite one."""
    st = np.asarray(resign_stats, dtype=np.float32)
    own = st if winner < 0 else st[int(winner)::2]
    own = own[~np.isnan(own)]
    return np.float32(own.min()) if own.size else np.float32(np.nan)


def calibrate_resign_threshold(trajectories, target=0.05):
    """AlphaGo Zero's calibration: the largest threshold ``t`` such that at most ``target`` of the calibration games (``no_resign``)
    have ``fp_margin < t`` -- i.e. would have been resigned by a player who did not lose.  -inf without calibration games."""
    margins = np.array([t.fp_margin for t in trajectories if getattr(t, 'no_resign', False)], dtype=np.float64)
    if margins.size == 0:
        return float('-inf')
    margins = np.sort(np.where(np.isnan(margins), np.inf, margins))   # (a game whose statistic was never finite never fires)
    k = int(np.floor(float(target) * margins.size + 1e-9))   # false positives allowed
    return float(margins[k]) if k < margins.size else float('inf')


def visits_to_pi(counts, temperature):
    """alphazero_mcts.py:10-14,91-92 on the visit counts of the legal moves."""
    x = 1.0 / temperature * np.log(np.asarray(counts) + 1e-10)
    probs = np.exp(x - np.max(x))
    probs /= np.sum(probs)
    return probs


def step_schedule(t_early, n_plies, t_late):
    """AlphaGo Zero's / AlphaZero's temperature schedule as a table for set_temperature_schedule: ``n_plies`` entries of ``t_early``
    (T before plies 0 .. n_plies - 1), then ``t_late`` -- the last entry holds for every later ply.  float64 [n_plies + 1]."""
    n_plies = int(n_plies)
    if n_plies < 0:
        raise ValueError('n_plies %d is negative' % n_plies)
    return np.array([float(t_early)] * n_plies + [float(t_late)], dtype=np.float64)


def decay_schedule(t_start, t_end, halflife, n):
    """KataGo's kind of schedule: T before ply p is t_end + (t_start - t_end) * 0.5 ** (p / halflife) for p < ``n``; the last entry
    holds for every later ply.  float64 [n]."""
    ply = np.arange(int(n), dtype=np.float64)
    return float(t_end) + (float(t_start) - float(t_end)) * 0.5 ** (ply / float(halflife))


def _check_temperatures(temps, n_cells):
    """-> the table as float64 [n]; ValueError for what rz_play_set_temperatures refuses."""
    tab = np.array(temps, dtype=np.float64).reshape(-1)
    if tab.size < 1:
        raise ValueError('an empty temperature schedule (None turns it off)')
    if not (np.isfinite(tab) & (tab > 0.0)).all():
        raise ValueError('temperature schedule: every entry must be finite and positive')
    if tab.size > n_cells:
        raise ValueError('temperature schedule: %d entries for a board of %d cells (a game has no more plies)' % (tab.size, n_cells))
    return tab


def draw_move(acts, probs, u):
    """numpy's legacy choice(acts, p=probs) for the uniform ``u``."""
    cdf = np.cumsum(probs)
    cdf /= cdf[-1]
    return int(acts[int(cdf.searchsorted(u, side='right'))])


def batch_pi_and_moves(visits, legal, temperature, uniforms):
    """visits_to_pi + draw_move for many games at once: visits int [R, A], legal bool [R, A], uniforms [R]
    -> (pi float64 [R, A] with zeros at illegal actions, chosen action int [R]).  ``temperature``: one T, or one per row [R] -- a
    row is then bit for bit the scalar call at its T (1 / T and the product with the logarithms are elementwise).

    Bit-identical to the per-game expressions above (which are the reference's, alphazero_mcts.py:10-14,
    91-92,148): log / exp / divide are elementwise; the maximum is exact; the normalising sum is taken over
    each game's COMPRESSED legal entries, grouped by their count, because numpy's pairwise summation depends on
    the array length; cumsum is sequential and adding the zeros of illegal actions changes nothing, so the
    first index with cdf > u on the full row is searchsorted(u, 'right') on the compressed one."""
    visits = np.asarray(visits)
    legal = np.asarray(legal, dtype=bool)
    R, A = visits.shape
    if np.ndim(temperature) == 0:
        x = 1.0 / temperature * np.log(visits + 1e-10)
    else:
        x = (1.0 / np.asarray(temperature, dtype=np.float64).reshape(R))[:, None] * np.log(visits + 1e-10)
    mx = np.where(legal, x, -np.inf).max(axis=1)
    e = np.exp(np.where(legal, x - mx[:, None], -np.inf))  # exp(-inf) = 0 at illegal actions
    k = legal.sum(axis=1)
    flat = e[legal]                      # every game's legal entries, ascending, one game after the other
    start = np.cumsum(k) - k
    sums = np.ones(R)
    for kk in np.unique(k):
        if kk > 0:
            rows = np.nonzero(k == kk)[0]
            sums[rows] = flat[start[rows][:, None] + np.arange(kk)].sum(axis=1)   # (a contiguous [rows, kk] array: numpy's pairwise sum of kk)
    pi = e / sums[:, None]
    cdf = np.cumsum(pi, axis=1)
    cdf /= cdf[:, -1:]
    moves = (cdf > np.asarray(uniforms, dtype=np.float64)[:, None]).argmax(axis=1)
    return pi, moves.astype(np.int64)


def shard_game_ids(n_games_total, rank, world_size):
    return list(range(rank, n_games_total, world_size))


class Trajectory(object):
    """One finished game: what start_self_play returns, in compact form."""

    def __init__(self, game_id, board_size, n_in_row, moves, pis, winner, game='gomoku', resigned=False, no_resign=False,
                 resign_stats=None, fp_margin=np.nan, full=None, root_values=None, epochs=None, raw_visits=None):
        """Resignation (BatchedSelfPlay.set_resign): ``resigned`` -- the game ended with the loser's resignation; ``moves`` / ``pis``
        are the plies actually played (the resigning search's pi is not recorded).  ``no_resign``: a calibration game (played
        out).  ``resign_stats``: float32 max(v_root, q_best) of every search of the game -- one more than the moves of a resigned
        game --, None with resignation off.  ``fp_margin``: a calibration game's selfplay.fp_margin, else NaN.
        Playout cap (BatchedSelfPlay.set_playout_cap): ``full`` -- a bool per search of the game, True where it had the full budget
        (one entry more than the moves of a resigned game, like ``resign_stats``); None with the cap off.
        Root values (BatchedSelfPlay.set_root_values): ``root_values`` -- float32 [plies], aligned with ``moves`` / ``pis``: -W / N of
        the root of the search that played the ply, the value the mover saw (MCTSEngine.root_values()[:, 0]); like ``pis`` the
        resigning search of a resigned game is not recorded.  None with the option off.
        Streams (BatchedSelfPlay.stream_collect): ``epochs`` -- int32 [plies], non-decreasing: the epoch of the search that played
        each ply (a stalled ply: of its searched record); None outside a stream.  Not part of the ranks' payload."""
        self.epochs = None if epochs is None else np.asarray(epochs, dtype=np.int32).reshape(-1)
        if self.epochs is not None and len(self.epochs) != len(moves):
            raise ValueError('game %d: %d epochs for %d plies' % (int(game_id), len(self.epochs), len(moves)))
        self.root_values = None if root_values is None else np.asarray(root_values, dtype=np.float32).reshape(-1)
        # forced playouts (BatchedSelfPlay.set_forced_playouts): int32 [plies, A], the RAW visit counts of every ply's search -- what
        # the move was drawn from; ``pis`` is then formed from the pruned counts.  None with the option off.
        self.raw_visits = None if raw_visits is None else np.asarray(raw_visits, dtype=np.int32).reshape(len(moves), -1)
        self.full = None if full is None else np.asarray(full, dtype=bool).reshape(-1)
        self.resigned, self.no_resign = bool(resigned), bool(no_resign)
        self.resign_stats = None if resign_stats is None else np.asarray(resign_stats, dtype=np.float32)
        self.fp_margin = np.float32(fp_margin)
        self.game_id = int(game_id)
        self.game = game
        self.board_size, self.n_in_row = board_size, int(n_in_row)
        self.moves = [int(m) for m in moves]
        pis = np.asarray(pis)
        if pis.dtype != np.float32:   # (float32 rows -- what came over the wire for the learner -- stay as they are: no 2x copy of a round's pi)
            pis = pis.astype(np.float64, copy=False)
        self.pis = pis.reshape(len(self.moves), -1) if len(self.moves) else pis.reshape(0, 0)
        self.winner = int(winner)
        if self.root_values is not None and len(self.root_values) != len(self.moves):
            raise ValueError('game %d: %d root values for %d plies' % (self.game_id, len(self.root_values), len(self.moves)))

    def _env(self):
        if self.game == 'connect4':
            from .games.connect4.connect4_env import Connect4Env
            return Connect4Env(self.board_size[0], self.board_size[1], self.n_in_row)
        from .games.gomoku.gomoku_env import GomokuEnv
        env = GomokuEnv(self.board_size, self.n_in_row)
        env.reset()
        return env

    def z(self):
        """+1 for the plies of the winner, -1 for the loser's, 0 on a tie (game.py:121-126); a resigned game's winner is the
        player who did not resign."""
        movers = np.arange(len(self.moves)) % 2  # player 0 moves first
        if self.winner == -1:
            return np.zeros(len(self.moves))
        return np.where(movers == self.winner, 1.0, -1.0)

    def states(self):
        """Observation planes before every move (GomokuEnv.current_state, gomoku_env.py:95-114): own stones, the opponent's, the
        last move, ones iff an even number of stones.  Gomoku: formed from the move list at once (ply q's stone is on the board of
        ply p > q, in plane 0 when q and p have the same parity -- two products of 0 / 1 matrices); Connect4 (stones drop: the cell
        depends on the column's height) replays the moves through the env."""
        if self.game == 'connect4':
            env = self._env()
            out = []
            for m in self.moves:
                out.append(env.current_state())
                env.step(m)
            return out
        P, B = len(self.moves), self.board_size
        if P == 0:
            return []
        moves = np.asarray(self.moves, dtype=np.int64)
        onehot = np.zeros((P, B * B))
        onehot[np.arange(P), moves] = 1.0
        before = np.tri(P, P, -1)                                    # [p, q] = 1 where ply q was played before ply p
        parity = np.arange(P) % 2
        same = (parity[:, None] == parity[None, :]).astype(np.float64)
        planes = np.zeros((P, 4, B * B))
        planes[:, 0] = (before * same) @ onehot
        planes[:, 1] = (before * (1.0 - same)) @ onehot
        planes[1:, 2] = onehot[:-1]
        planes[0::2, 3] = 1.0
        return list(planes.reshape(P, 4, B, B))

    def as_reference_tuple(self):
        """(winner, [(state, mcts_prob, z), ...]) -- start_self_play's return value."""
        return self.winner, list(zip(self.states(), list(self.pis), self.z()))

    def training_samples(self, value_mix=0.0):
        """[(state, mcts_prob, z), ...] of the plies a learner takes its policy target from: under a playout cap the plies whose
        search had the full budget (``full``), each with its own state and z; every ply without a cap.  ``value_mix`` = lam > 0 on a
        game with ``root_values``: the third element is replay.mixed_value_targets(z, root_values, lam) -- (1 - lam) z + lam q, float32,
        what the device buffer's kernels write (DeviceReplay.set_value_mix) -- instead of z; without root values, or at 0, z as it is."""
        value_mix = float(value_mix)
        if not 0.0 <= value_mix <= 1.0:
            raise ValueError('value_mix %r not in [0, 1]' % value_mix)
        targets = self.z()
        if value_mix > 0.0 and self.root_values is not None:
            from .replay import mixed_value_targets
            targets = mixed_value_targets(targets, self.root_values, value_mix)
        samples = list(zip(self.states(), list(self.pis), targets))
        if self.full is None:
            return samples
        return [sm for sm, f in zip(samples, self.full[:len(self.moves)]) if f]




def plan_lanes(n_games, n_cus=256, hw_queues=None, deferred=False, cells=None, in_flight=1, resident_per_cu=1):
    """-> (lanes, trunk_workgroups, heads_algo) for ``n_games`` leaves per simulation step on a GPU with ``n_cus`` CUs and
    ``hw_queues`` hardware queues for its streams (default: what rlzero_amd claimed on import, rlzero_amd.HW_QUEUES).

    ``deferred``: the batch runs the deferred-priors route (HipNetEvaluator.deferred_ok: UCT_REF, one simulation in flight, boards
    of 11 .. 16 rows).  A lane's step is then trunk -> tree step (23 + 10 us at 15x15) and the table was measured again
    (profiles/r04/lane_sweep.txt, M simulations / s): up to one round of boards the resident search, one workgroup per game and one
    launch per search, on one lane up to half a round and on two beyond (256 games: 9.2 against 7.8 on two lanes of the two-launch
    step, profiles/r04/ab_resident.txt); up to
    1.75 rounds THREE (320 / 384 games: 9.2 / 10.3 against 8.7 / 9.8 with
    two); 448 games TWO (10.3 against 10.1); 2 .. 2.75 rounds FOUR on 8 hardware queues (512 / 640 games: 10.6 / 10.6 against 10.5
    / 10.1 with two -- with fewer queues two lanes, a percent behind); beyond, TWO (768 .. 1536 games: 10.9 .. 11.0).

    ``resident_per_cu`` = 2 (with ``deferred``: the receptive-field trunk, HipNetEvaluator.resident_delta_ok -- boards of 11 .. 16 rows
    and columns): the resident search holds TWO games per CU (k_delta_res: 82 KB of LDS), so up to 2 x CUs games -- the 512 per GPU of
    BASELINE.json configs[3] -- are ONE launch per search on ONE lane: one game's serial tree walk runs under the other game's matrix
    work on the same CU, and no hardware-queue layout is involved (round 6, same box: 512 games 18.95 M on one lane, 17.0 M on two,
    13.7 M on the four lanes of the two-launch step; profiles/r06/NOTES.md).  From 3 x CUs games on the same single lane again, the
    grid running in rounds of 2 x CUs workgroups (1024 .. 4096 games: 18.4 .. 18.8 M; profiles/r06/ab_rounds.txt).

    ``cells``: positions of the board, when known.  Boards of at most 42 cells on the split-f16 trunk (Connect4, 6x6: the
    two-launch step with a 12-us trunk and a 10-us tree step) run TWO lanes above one round of boards (Connect4, M simulations / s on
    2 / 3 / 4 lanes: 384 games 14.2 / 13.8 / 13.1, 512 games 17.7 / 15.7 / 16.7, 768 games 20.2 / 20.4 / 20.0, 1024 games
    22.9 / 21.9 / 21.1 -- profiles/r04/small_boards_lanes.txt; 9x9 keeps the table below: 512 games 14.8 / 14.5 / 15.4).

    ``in_flight`` = K > 1 (the opt-in virtual-loss mode; ``n_games`` = games x K leaves) on a board of at most 100 cells: the
    three-launch step of short kernels wants MORE lanes than the 15x15 table below gives it (9x9, K = 16, M simulations / s on
    1 / 2 / 3 / 4 lanes: 32 games 4.5 / 4.7 / 5.1 / 4.3, 64 games 6.8 / 7.4 / 7.9 / 8.1, 128 games 8.6 / 10.0 / 10.7 / 11.2; K = 8,
    64 games 6.0 / 6.5 / 6.9 / 7.0): three lanes from two rounds of leaves, four from four rounds.

    The three-launch step (every other batch), measured on
    MI355X at 15x15 (profiles/r03/lane_sweeps.txt; a trunk workgroup takes a board in ~23 us, three in ~65 us):

    * up to one round of boards (n_games <= CUs): ONE lane -- the step is a chain of three latency-bound launches, and splitting it
      shortens none of them (128 / 192 / 256 games: 3.4 / 4.9 / 6.3 M with one lane, 3-8 % less with two to four);
    * more: lanes with UN-capped trunks and the LDS-free 'parts' FC GEMM, whose single-wave workgroups -- like the tree step's -- fit
      on a CU beside a resident trunk workgroup (the trunk holds 151 of 160 KB LDS and at most 400 of 512 registers): the small kernels
      of a lane run UNDER the other lanes' trunks on the same CUs.  With TWO lanes a lane's tree step + FC GEMM (15 us + two kernel
      boundaries) must end before the other lane's trunk does (23 us at one board per workgroup), or the CUs wait: on most boxes they
      do (512 games: 8.0-8.9 M, on the best box 10.3 M).  FOUR lanes of a quarter of the games keep two lanes' trunk workgroups queued
      on the CUs at all times and the chip never waits for a lane's chain: 9.8-10.3 M on every box -- from ~1.75 to ~2.75 rounds of
      boards (448 .. 704 games), and only with 8 hardware queues (with HIP's default of 4 the fourth lane shares a queue and the lanes
      serialise: 6.1 M; five lanes and more collapse the same way even with 16);
    * THREE lanes between one and 1.75 rounds (320 / 384 games: +4 % / +1 % over two) and wherever four would need more queues;
    * beyond ~2.75 rounds TWO lanes: a trunk launch then runs two or three boards per workgroup (44 / 65 us) and hides a lane's chain
      by itself (768 / 1024 / 1536 games: 10.1 / 11.3 / 11.4 M with two lanes, 9.5 / 9.1 / 10.2 with four).
    ``trunk_workgroups`` is 0 = one per CU (capped trunks, 4 CUs per XCD left to the small kernels, lost 15-19 % against un-capped
    ones once the 'parts' GEMM existed)."""
    if hw_queues is None:
        from . import HW_QUEUES as hw_queues
    if cells is not None and cells <= 49 and n_cus < n_games <= 2 * n_cus and in_flight <= 1 and resident_per_cu >= 2:
        # boards of the compact LDS grid (up to 7 columns; HipNet.compact_resident): the resident search holds two games per CU --
        # one launch per search on one lane up to 2 x CUs games (profiles/r06/ab_compact_resident.txt, M simulations / s against
        # the two lanes below: Connect4 384 games 19.8 / 17.1, 512 games 24.8 / 21.3; 6x6 512 games 26.5 / 22.5).  Beyond, a
        # partial second round costs more than the lanes' overlap (768 games 21.2 / 24.7; 1024 25.7 / 25.0; 2048 26.5 / 27.6)
        return 1, 0, 'auto'
    if cells is not None and cells <= 42 and n_games > n_cus and in_flight <= 1:
        return 2, 0, 'parts'
    if cells is not None and cells <= 100 and in_flight > 1 and n_games >= 2 * n_cus:
        return (4 if (n_games >= 4 * n_cus and hw_queues >= 8) else 3), 0, 'parts'
    if deferred:
        if resident_per_cu >= 2 and (n_games <= 2 * n_cus or n_games >= 3 * n_cus):
            # two games per CU: the resident search with the receptive-field trunk, one lane -- and from 1.5 rounds of two per CU on
            # again: the launch's workgroups depend on nothing outside their game, so a bigger grid runs in ROUNDS, a CU's free half
            # going to the next game as a search ends (profiles/r06/ab_rounds.txt, M simulations / s, one resident lane against the
            # lanes below: 576 games 12.4 / 14.0, 640 13.6 / 14.5, 768 14.6 / 12.6, 1024 18.8 / 11.9, 1536 18.6 / 14.0, 2048 18.4 / 16.1,
            # 4096 18.4 / 16.9 -- between one and 1.5 rounds the second round is too empty and four lanes of the two-launch step win)
            return 1, 0, 'auto'
        if n_games <= n_cus:   # one game per CU at most: the resident search (one launch per search, a workgroup per game) --
            # on TWO lanes from half a round of boards on, so that a lane's host step runs under the other lane's search
            # (256 games: 9.17 against 8.57 M; 128 games 4.83 against 4.74; profiles/r04/ab_resident.txt)
            return (2 if 2 * n_games > n_cus else 1), 0, 'auto'
        if 4 * n_games < 7 * n_cus:
            return 3, 0, 'parts'
        if n_games < 2 * n_cus or 4 * n_games > 11 * n_cus:
            return 2, 0, 'parts'
        return (4 if hw_queues >= 8 else 2), 0, 'parts'
    if n_games <= n_cus:
        return 1, 0, 'auto'
    if 4 * n_games < 7 * n_cus:
        return 3, 0, 'parts'
    if 4 * n_games <= 11 * n_cus:
        if hw_queues < 8:
            import warnings
            from . import HW_QUEUES_TOO_LATE
            warnings.warn('plan_lanes: %d games want four lanes, but this process has %d hardware queues%s: three lanes (about 8 %% '
                          'slower at 512 games); see rlzero_amd.configure' % (
                              n_games, hw_queues, ' (rlzero_amd was imported after the HIP runtime had started)'
                              if HW_QUEUES_TOO_LATE else ''), RuntimeWarning, stacklevel=2)
            return 3, 0, 'parts'
        return 4, 0, 'parts'
    return 2, 0, 'parts'


# ------------------------------------------------------------------------- lanes by measurement
# plan_lanes() is a table measured on ONE chip (MI355X, 256 CUs, 8 hardware queues) for the reference's network: its thresholds are
# in units of that chip's CUs and its neighbouring choices differ by up to 15 %.  Anywhere else -- a partition of the GPU with
# fewer CUs, another chip -- the table's pick is only the starting point: the two or three neighbouring layouts are built, timed
# for two moves each and the fastest is kept, once per (device, CUs, board, batch, search) in this process.
TABLE_CUS = 256
_LANE_CACHE = {}


def lane_candidates(table_pick, hw_queues, n_games):
    """The layouts worth timing around the table's pick: one lane fewer, the pick, one more (four lanes need 8 hardware queues)."""
    most = min(4 if hw_queues >= 8 else 3, max(1, n_games))
    return sorted({min(most, max(1, table_pick - 1)), min(most, max(1, table_pick)), min(most, table_pick + 1)})


def time_moves(sp, moves=2):
    """Simulations / second of ``sp`` over ``moves`` moves of fresh games (one more move first, un-timed), the move step on the device."""
    import time
    t = sp.torch
    sp.device_attach(queue_capacity=4 * sp.n_slots)
    sp.device_queue(range(4 * sp.n_slots))
    sp.play_move_device()
    t.cuda.synchronize()
    sp.device_drain()
    s0, t0 = sp.sims_done, time.perf_counter()
    for _ in range(moves):
        sp.play_move_device()
    t.cuda.synchronize()
    sp.device_drain()
    return (sp.sims_done - s0) / (time.perf_counter() - t0)


def choose_lanes_by_measurement(key, table_pick, hw_queues, n_games, build, timer=time_moves, cache=None):
    """-> (lanes, {lanes: simulations / s}) for ``key``: every candidate layout is built by ``build(lanes)`` (-> a BatchedSelfPlay),
    timed by ``timer(sp)`` and closed; the fastest wins, ties go to fewer lanes.  Cached by ``key``."""
    cache = _LANE_CACHE if cache is None else cache
    if key in cache:
        return cache[key]
    rates = {}
    for lanes in lane_candidates(table_pick, hw_queues, n_games):
        sp = None
        try:   # (a candidate that cannot be built or timed -- e.g. a mode the timer's move step does not serve -- is no candidate)
            sp = build(lanes)
            rates[lanes] = float(timer(sp))
        except HipError:
            pass
        finally:
            for lane in getattr(sp, 'lanes', ()) if sp is not None else ():
                lane.eng.close()
    if not rates:   # nothing could be measured: the table's pick, not cached as a measurement
        return table_pick, None
    best = max(sorted(rates), key=lambda c: (rates[c], -c))
    cache[key] = (best, rates)
    return cache[key]


def plan_route(rows, cols, game, net_algo, score_mode, in_flight, deferred_priors=None, delta_trunk=None, resident_search=None,
               n_games=0, n_cus=0, resident_puct=False, lanes=None, host_evaluator=False):
    """What plan_lanes() is told of the route (its ``deferred`` / ``cells`` / ``in_flight`` / ``resident_per_cu``) for the evaluators
    for_network() will build from these arguments: route.decide() on numbers alone -- no net, no engine, no GPU.
    ``resident_puct`` (for_network's switch: the resident search under PUCT, one game per CU): asked for where it cannot be served it
    raises ValueError with the reason (route.resident_puct_refusal: the selection rule, sims_in_flight, the trunk, the board; a host
    evaluator; more games per lane than CUs, with ``lanes`` as given or as plan_lanes() splits the batch) -- never another route."""
    if resident_puct:
        why = 'a host evaluator has no resident search' if host_evaluator else _route.resident_puct_refusal(
            rows, cols, net_algo or 'split_f16', resident_search=resident_search is not False, score_mode=score_mode, in_flight=in_flight)
        if why is None:
            n_lanes = lanes if isinstance(lanes, int) else plan_lanes(n_games, n_cus or TABLE_CUS, in_flight=in_flight)[0]
            per_lane = -(-n_games // max(1, min(int(n_lanes), max(1, n_games))))
            if n_cus and per_lane > n_cus:
                why = '%d games per lane on %d CUs: the resident PUCT search holds one game per CU' % (per_lane, n_cus)
        if why is not None:
            raise ValueError('resident_puct=True cannot be served: ' + why)
    r = _route.decide(rows, cols, net_algo or 'split_f16', deferred_priors=deferred_priors is not False, delta_trunk=delta_trunk is not False,
                      resident_search=resident_search is not False, score_mode=score_mode, in_flight=in_flight, n_games=n_games, n_cus=n_cus,
                      resident_puct=bool(resident_puct))
    algo_of_small_boards = (net_algo or 'split_f16') in _route.EVERY_BOARD_SPLIT_TRUNKS
    return dict(deferred=r.deferred and game == 'gomoku' and _route.rows_kernel_board(rows, cols),   # (the table's deferred rows: 15x15 Gomoku and its kin)
                cells=rows * cols if ((r.deferred and algo_of_small_boards) or in_flight > 1) else None, in_flight=in_flight,
                resident_per_cu=r.resident_per_cu if r.resident else 1)


def stream_lookahead(copy_every, depth):
    """Moves of a lane enqueued and unread whenever a stream's calls return (BatchedSelfPlay.stream_start / stream_collect): a constant
    of the stream, ``depth`` read-backs of ``copy_every`` rows."""
    return int(copy_every) * int(depth)


def stream_topup(n_slots, copy_every, depth):
    """Ids a stream keeps pushed beyond the host's count of started games -- and the smallest ring its queue needs.  The count lags:
    when a push is enqueued, stream_lookahead rows are unread, ``copy_every`` more moves run before the next push, a slot claims at
    most one id per move step, and a claim shows one row later (the game's first record) -- with one more per slot for a claim before
    the rows read whose record waits (a stall at ply 0): no slot idles for want of an id."""
    return int(n_slots) * ((int(depth) + 1) * int(copy_every) + 1)


# what a log row is verified under: the settings in force when its move was enqueued (a stream's epochs; SelfPlayReader.read_rows)
Epoch = collections.namedtuple('Epoch', 'first_row temperature_schedule pi_temperature playout_cap resign_threshold resign_disabled_frac')


class SelfPlayReader(object):
    """What turns the device move step's log into Trajectories (include/rlzero_hip.h: rz_play_*): the settings a game depends on, the
    counters, and the book of the slots (playlog.SlotBook).  numpy only -- BatchedSelfPlay adds the engines; a test builds one alone.
    ``resolve(slot, move)`` hands a stalled slot's move back to the device."""

    forced_k, forced_prune = 0.0, True   # set_forced_playouts (off: what every object starts with)

    def __init__(self, n_slots, n_actions, max_plies, n_playout, geometry, resolve, temperature=1.0, seed=0):
        self.n_slots, self.n_playout, self.geometry = n_slots, n_playout, geometry   # geometry: (board_size, n_in_row, game)
        self.temperature = float(temperature)
        self.seed = int(seed)
        self.book = SlotBook(n_slots, max_plies, resolve, dict(
            pi=(np.float64, (n_actions, ), 'move'),
            stat=(np.float32, (), 'search'),    # resignation statistic of every search (set_resign)
            full=(bool, (), 'search'),          # full budget of every search (set_playout_cap)
            q=(np.float32, (), 'search'),       # root value of every search (set_root_values; NaN with it off)
            ep=(np.int32, (), 'search')))       # epoch of every search (a stream; 0 outside one)
        self.epochs = None   # a stream's epochs, oldest first: [Epoch] (BatchedSelfPlay.stream_start); None outside a stream
        self.root_values_on = False   # set_root_values: the side ring of the log is read and Trajectory.root_values formed
        self.forced_k, self.forced_prune = 0.0, True   # set_forced_playouts: k (0: off), and whether pis come from the pruned counts
        self.slot_game, self.slot_ply = self.book.slot_game, self.book.slot_ply
        # the plies of a slot's game (of its last one until it starts another), read-only: moves (a list), pis, root values
        self.slot_moves, self.slot_pis, self.slot_values = (
            playlog.Plies(self.book, None, as_list=True), playlog.Plies(self.book, 'pi'), playlog.Plies(self.book, 'q'))
        self.sims_done = 0
        self.resign_threshold, self.resign_disabled_frac = float('nan'), 0.0
        self.resign_would = 0   # plies of calibration games where the rule fired (RZ_PLAY_WOULD_RESIGN on the device)
        self.playout_cap = None   # set_playout_cap: (n_fast, p_full)
        self.full_plies = 0   # searches with the full budget so far (with the cap off: every search)
        self.temperature_schedule = None   # set_temperature_schedule: T before ply p, float64 [n <= cells]
        self.pi_temperature = None         # set_temperature_schedule: the T of the stored pis (None: the ply's)

    moves_done, stalls_resolved, _started = playlog.counter('moves_done'), playlog.counter('stalls_resolved'), playlog.counter('started')

    def _temps(self, plies):
        """-> T per row: the schedule's entry of the row's ply (the last one beyond it), or the one temperature."""
        tab = self.temperature_schedule
        if tab is None:
            return self.temperature
        return tab[np.minimum(np.asarray(plies, dtype=np.int64), tab.size - 1)]

    def _pis_moves(self, visits, legal, plies, uniforms):
        """batch_pi_and_moves at the rows' temperatures; the stored pi at pi_temperature where one is set."""
        pis, chosen = batch_pi_and_moves(visits, legal, self._temps(plies), uniforms)
        if self.pi_temperature is not None:
            pis = batch_pi_and_moves(visits, legal, self.pi_temperature, uniforms)[0]
        return pis, chosen

    def _full(self, game_ids, plies):
        """-> bool per (game, ply): the search has the full budget under the current cap."""
        return cap_uniform(self.seed, game_ids, plies) < self.playout_cap[1]

    @property
    def resign_on(self):
        return not np.isnan(self.resign_threshold)

    def _calibration(self, game_ids):
        """-> bool per game: resignation disabled (a calibration game) under the current rule."""
        return resign_uniform(self.seed, game_ids) < self.resign_disabled_frac

    def _resign_record(self, stats, winner, no_resign, resigned):
        """Trajectory keywords of a finished game under the rule (none without it)."""
        if not self.resign_on:
            return {}
        stats = np.asarray(stats, dtype=np.float32)
        return dict(resigned=resigned, no_resign=no_resign, resign_stats=stats,
                    fp_margin=fp_margin(stats, winner) if no_resign else np.nan)

    def settings(self, first_row=0):
        """-> Epoch: the settings a row is verified under, as they are now."""
        tab = self.temperature_schedule
        return Epoch(int(first_row), None if tab is None else tab.copy(), self.pi_temperature, self.playout_cap,
                     self.resign_threshold, self.resign_disabled_frac)

    @contextlib.contextmanager
    def _under(self, epoch):
        """The reader's settings as they were in ``epoch`` (an Epoch; None: as they are) for the block's length."""
        if epoch is None:
            yield
            return
        now = self.settings()
        try:
            (_, self.temperature_schedule, self.pi_temperature, self.playout_cap, self.resign_threshold, self.resign_disabled_frac) = epoch
            yield
        finally:
            (_, self.temperature_schedule, self.pi_temperature, self.playout_cap, self.resign_threshold, self.resign_disabled_frac) = now

    def read_rows(self, rows, lo=0, values=None, row_epochs=None, no_idle=False, pruned=None):
        """Log rows int32 [R, G, words] of the slots ``lo`` .. ``lo + G - 1``, oldest first -> (the trajectories of the games that
        ended in them, the RUNNING records of the last row).  pi is formed here, from the logged visit counts with the reference's
        expression, and every move and flag of the device is verified against this side's draw on the same key.  ``values``: the
        same rows of the side ring of root values, float32 [R, G] (set_root_values; required while it is on).
        ``row_epochs`` (a stream): int [R], the index into ``self.epochs`` of each row -- its moves, budgets and resignation flags are
        verified, and its pis formed, under THAT epoch's settings, not the current ones; the trajectories carry ``epochs``, and a
        game is a calibration game only if it was one in every epoch it spans.  ``no_idle``: HipError for a record without a game
        (a stream's slots never wait for an id).  ``pruned``: the same rows of the side ring of pruned counts, int32 [R, G, A]
        (set_forced_playouts with pruning; required while it is on): the moves are still verified from the log's raw counts, the pis
        are the same expression on the pruned ones, and the trajectories carry ``raw_visits``."""
        forced, pruning = self.forced_k > 0.0, self.forced_k > 0.0 and self.forced_prune
        if pruning and pruned is None:
            raise ValueError('policy target pruning is on (set_forced_playouts): read_rows needs the rows of the pruned counts\' ring')
        if forced and row_epochs is not None:
            raise ValueError('forced playouts are on (set_forced_playouts): a stream does not serve them')
        if self.root_values_on and values is None:
            raise ValueError('root values are on (set_root_values): read_rows needs the side ring\'s rows')
        if no_idle and ((rows[..., 4] & playlog.PLAY_RUNNING) == 0).any():
            r, g = [int(x[0]) for x in np.nonzero((rows[..., 4] & playlog.PLAY_RUNNING) == 0)]
            raise HipError('slot %d holds no game in row %d of this read: a slot of a stream waited for a game id' % (lo + g, r))
        g_i, d, last_running = playlog.running(rows)
        if g_i.size == 0:
            return [], last_running
        if row_epochs is None:
            rec_ep, groups = np.zeros(g_i.shape, dtype=np.int32), [(None, slice(None))]
        else:
            rec_ep = np.asarray(row_epochs, dtype=np.int32)[np.nonzero((rows[..., 4] & playlog.PLAY_RUNNING) != 0)[0]]
            groups = [(self.epochs[e], rec_ep == e) for e in np.unique(rec_ep)]
        pis = np.zeros(d.counts.shape, dtype=np.float64)
        chosen = np.zeros(g_i.shape, dtype=np.int64)
        fulls = np.zeros(g_i.shape, dtype=bool)
        for epoch, sel in groups:
            part = d if epoch is None else playlog.Records(*[f[sel] for f in d])
            with self._under(epoch):
                # the reference's expression on the logged counts; the draw with the game's uniform (numpy's inverse-CDF rule): the arbiter
                pis[sel], chosen[sel] = self._pis_moves(part.counts, part.legal, part.ply, move_uniform(self.seed, part.game, part.ply))
                cap = self.playout_cap
                sims, full = playlog.check_budgets(part, self.n_playout, cap, None if cap is None else cap_uniform(self.seed, part.game, part.ply))
                self.sims_done += sims
                self.full_plies += full
                fulls[sel] = ((part.flags & PLAY_FULL) != 0) | (cap is None and row_epochs is not None)   # (a stream: without a cap every search is full)
                if self.resign_on:
                    self.resign_would += playlog.check_resignation(part, self.resign_threshold, self._calibration(part.game))
        playlog.check_moves(d, chosen)
        q = playlog.running_values(rows, values) if self.root_values_on else np.full(g_i.shape, np.nan, dtype=np.float32)
        columns = dict(pi=pis, stat=d.stat, full=fulls, q=q, ep=rec_ep)
        if pruning:   # the host stays the arbiter: the same numpy expression, on the ring's pruned rows
            pruned = np.asarray(pruned)
            if pruned.shape != rows.shape[:2] + (d.counts.shape[-1], ):
                raise ValueError('the pruned counts\' rows %r do not match the log\'s %r' % (pruned.shape, rows.shape[:2]))
            pr = pruned[np.nonzero((rows[..., 4] & playlog.PLAY_RUNNING) != 0)]
            if ((pr >= 0) != d.legal).any() or (pr > d.visits).any() or (np.where(d.legal, pr, 0).sum(axis=-1) <= 0)[d.counts.sum(axis=-1) > 0].any():
                raise HipError('the ring of pruned counts disagrees with the log: another legal set, a count above the raw one or an empty row')
            columns['pi'] = self._pis_moves(np.where(d.legal, pr, 0), d.legal, d.ply, move_uniform(self.seed, d.game, d.ply))[0]
        if forced:
            columns['raw'] = d.counts.astype(np.int32)
        done = []
        for f in self.book.feed(lo + g_i, d, chosen, columns):
            eps = f.columns['ep']
            done.append(self.trajectory(f, [None] if row_epochs is None else self.epochs[int(eps[0]):int(eps[-1]) + 1]))
        return done, last_running

    def trajectory(self, f, span=(None, )):
        """A game the book has closed (playlog.Finished) -> its Trajectory.  ``span``: the epochs of its searches, oldest first (a
        stream); (None, ) outside one: the settings as they are."""
        calib = not f.resigned
        for epoch in span:   # (a calibration game: one in every epoch it spans)
            with self._under(epoch):
                calib = calib and self.resign_on and bool(self._calibration(f.game))
        with self._under(span[-1]):
            extra = self._resign_record(f.columns['stat'], f.winner, calib, f.resigned)
        caps = [self.playout_cap if epoch is None else epoch.playout_cap for epoch in span]
        if any(c is not None for c in caps):
            extra['full'] = f.columns['full']
        if self.root_values_on:   # (a resigned game has one search more than moves: the resigning one is not recorded)
            extra['root_values'] = f.columns['q'][:len(f.moves)]
        if span[0] is not None:
            extra['epochs'] = f.columns['ep'][:len(f.moves)]
        if self.forced_k > 0.0:
            extra['raw_visits'] = f.columns['raw']
        return Trajectory(f.game, self.geometry[0], self.geometry[1], f.moves.tolist(), f.columns['pi'], f.winner,
                          game=self.geometry[2], **extra)

    def decide_and_record(self, slots, visits, legal, values=None, pruned=None):
        """The move step of the host-driven loop, for running ``slots`` (distinct) after their searches: ``visits`` int [n, A] the
        roots' counts, ``legal`` bool [n, A], ``values`` fp64 [n, 2] = (v_root, q_best) of MCTSEngine.root_values (required under
        resignation or root values), ``pruned`` int [n, A] the pruned counts (required under policy target pruning) -> (the move of
        every slot, -1 where its mover resigns; bool per slot: resigned).  The rules of k_play_draw on the same numbers; the book and
        the counters take the searches and the moves, the caller ends the games (``book.close`` -> ``trajectory``)."""
        slots = np.asarray(slots, dtype=np.int64)
        n = len(slots)
        if n == 0:   # (a lane whose slots are all idle: nothing was fetched for it, nothing is decided)
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
        if (self.resign_on or self.root_values_on) and values is None:
            raise ValueError('resignation or root values are on: decide_and_record needs the roots\' values')
        if self.forced_k > 0.0 and self.forced_prune and pruned is None:
            raise ValueError('policy target pruning is on (set_forced_playouts): decide_and_record needs the pruned counts')
        gids, plies = self.slot_game[slots], self.slot_ply[slots]
        full = np.ones(n, dtype=bool) if self.playout_cap is None else self._full(gids, plies)
        self.sims_done += self.n_playout * n if self.playout_cap is None else int(np.where(full, self.n_playout, self.playout_cap[0]).sum())
        self.full_plies += int(full.sum())
        stat, quit_ = np.float32(np.nan), np.zeros(n, dtype=bool)
        if self.resign_on:   # the mover resigns when v_root and q_best are both below the threshold, except in a calibration game
            stat = np.maximum(values[:, 0], values[:, 1]).astype(np.float32)   # (NaN when either is)
            fire = (values[:, 0] < self.resign_threshold) & (values[:, 1] < self.resign_threshold)
            calib = self._calibration(gids)
            self.resign_would += int((fire & calib).sum())
            quit_ = fire & ~calib
        q = values[:, 0].astype(np.float32) if self.root_values_on else np.float32(np.nan)   # (k_play_draw's float32 of the same fp64 value)
        self.book.put_search(slots, plies, dict(stat=stat, full=full, q=q, ep=0))
        moves = np.full(n, -1, dtype=np.int64)
        on = ~quit_
        if on.any():
            us = move_uniform(self.seed, gids[on], plies[on])
            pis, moves[on] = self._pis_moves(visits[on], legal[on], plies[on], us)
            cols = dict(pi=pis)
            if self.forced_k > 0.0:   # the move from the raw counts, as ever; the stored pi from the pruned ones
                cols['raw'] = visits[on].astype(np.int32)
                if self.forced_prune:
                    cols['pi'] = self._pis_moves(np.where(legal[on], pruned[on], 0), legal[on], plies[on], us)[0]
            self.book.put_moves(slots[on], plies[on], moves[on], cols)
        return moves, quit_


class _Lane(object):
    """One engine + its evaluator + the HIP stream its kernels are enqueued on."""

    def __init__(self, engine, evaluator, stream, offset):
        self.eng, self.evaluator, self.stream, self.offset = engine, evaluator, stream, offset
        self.slots = slice(offset, offset + engine.n_games)
        self.primed = False       # play_move_pipelined: the coming move's simulations are in flight
        self.move_graph = None    # device_attach: the whole-move hipGraph of a resident lane


class BatchedSelfPlay(SelfPlayReader):
    """Plays games on one GPU; slots are refilled as games end.

    ``engine`` / ``evaluator`` may be lists of equal length: each (engine, evaluator) pair is a
    *lane* with its own HIP stream, and the simulation steps of the lanes are enqueued
    alternately.  While the network kernel of one lane owns the CUs' LDS, the latency-bound tree
    kernels of the other lane run beside it (they use no LDS), so the halves ping-pong and the
    tree work is hidden under the dense contraction.  Results do not depend on the lane split:
    games are independent and their uniforms are keyed by game id."""

    _dev_on = False      # device_attach: the move step is on the device
    _streaming = False   # stream_start: a collection that does not stop the device is open
    _chunks_done = -1    # graph chunks of the host loop so far (eager_every)

    def __init__(self, engine, evaluator, temperature=1.0, seed=0, use_graph=False, sims_per_graph=8,
                 eager_every=0):
        engines = list(engine) if isinstance(engine, (list, tuple)) else [engine]
        evaluators = list(evaluator) if isinstance(evaluator, (list, tuple)) else [evaluator]
        assert len(engines) == len(evaluators) >= 1
        torch = engines[0].torch
        self.torch = torch
        self.lanes, offset = [], 0
        for i, (eng, ev) in enumerate(zip(engines, evaluators)):
            stream = torch.cuda.current_stream(eng.device) if len(engines) == 1 else \
                torch.cuda.Stream(device=eng.device)
            # the engine's buffers were initialised on the current stream: order the lane's stream behind it
            stream.wait_stream(torch.cuda.current_stream(eng.device))
            self.lanes.append(_Lane(eng, ev, stream, offset))
            offset += eng.n_games
        n_cus = torch.cuda.get_device_properties(engines[0].device).multi_processor_count

        # (resident workgroups a CU holds: two of the receptive-field kernel (k_delta_res) and of the compact grid's)
        asked = [eng._ask(ev) for eng, ev in zip(engines, evaluators)]
        if len(engines) > 1 and sum(e.n_games for e in engines) > n_cus * min(r.resident_per_cu for r, _, _ in asked):
            # lanes that share CUs: the resident search (a workgroup keeps its CU for a whole search) is for games that have a CU
            # each -- these lanes run the two-launch step, whose trunk workgroups make way for the other lanes every step
            # (asked for explicitly -- resident_puct -- it stays: such lanes' launches take turns on the CUs)
            for _, owner, _ in asked:
                if owner is not None and not getattr(owner, 'resident_puct', False):
                    owner.resident_search = False
        self.eng = engines[0]  # geometry (board size, n_playout) is common to all lanes
        self.evaluator = evaluators[0]
        SelfPlayReader.__init__(self, offset, self.eng.n_actions, self.eng.n_cells, self.eng.n_playout,
                                (self.eng.board_size, self.eng.n_in_row, self.eng.game), self._resolve, temperature=temperature, seed=seed)
        self.use_graph = use_graph
        self.sims_per_graph = sims_per_graph
        self.eager_every = int(eager_every)  # with graphs: every k-th chunk runs eagerly (timing samples)
        G = self.n_slots
        self.cell_taken = np.zeros((G, self.eng.n_cells), dtype=bool)  # host mirror of the root boards
        self.cap_longest_first = True   # workgroups of k_delta_res take the full-budget games first (both loops; read at device_attach)

    def set_forced_playouts(self, k=2.0, prune=True):
        """Forced playouts and policy target pruning (KataGo, Wu 2019, section 3.2; an opt-in extension of score_mode 'puct') for every
        lane and BOTH loops (run, run_device).  ``k`` > 0: in every search a root child the search has touched is selected whatever
        its score while n n < (k p) N (MCTSEngine.set_forced_playouts; rz_forced.h).  The move is still drawn, and verified, from the
        RAW counts; ``prune`` True: Trajectory.pis is the same numpy expression on the PRUNED counts (MCTSEngine.root_pruned_visits;
        in run_device a side ring of the log, rz_play_set_pruned_visits, written in front of the draw and part of the whole-move
        graph), False: on the raw counts.  Trajectory.raw_visits keeps the raw counts either way.  ``k`` 0 / None: off.  Between
        runs; an attached object attaches again, and the simulation graphs are captured again: k travels in the kernel arguments.
        ValueError, never a fallback: a lane that selects by 'uct_ref' or has sims_in_flight > 1, a playout cap, an evaluator that
        puts no priors into the tree (RolloutEvaluator), an open stream, a lane in match mode."""
        k = 0.0 if k is None else float(k)
        if not (np.isfinite(k) and k >= 0.0):
            raise ValueError('forced playouts: k = %r is not a finite number >= 0' % (k, ))
        self._no_stream('set_forced_playouts')   # (continuous self-play under PUCT is not served)
        if k > 0.0:
            from . import _hip
            from .engine import RolloutEvaluator
            if self.playout_cap is not None:
                raise ValueError('forced playouts: a playout cap is set (set_playout_cap): the cap is a rule of the uct_ref search')
            for lane in self.lanes:
                if lane.eng.score_mode != _hip.SCORE_PUCT:
                    raise ValueError("forced playouts are a rule of score_mode 'puct' (a lane's engine selects by 'uct_ref')")
                if lane.eng.sims_in_flight != 1:
                    raise ValueError('forced playouts need one simulation in flight per tree (sims_in_flight = %d)' % lane.eng.sims_in_flight)
                if isinstance(lane.evaluator, RolloutEvaluator):
                    raise ValueError('forced playouts read the priors in the tree: this evaluator hands over none (uniform priors)')
                if getattr(lane.eng, 'play_match_on', False):
                    raise ValueError('a lane\'s engine is in match mode (play_set_match): its games are not training data')
        if (k, bool(prune)) == (self.forced_k, self.forced_prune):
            return
        was_dev = self._dev_on
        if was_dev:
            self.device_stop()
        self.abandon_running()
        rewarm = any(lane.eng._graphs for lane in self.lanes)
        for lane in self.lanes:
            if lane.eng.forced_k != k:
                with self._on(lane):
                    if getattr(lane.eng, '_play_on', False):   # (the move step holds the old k: a fresh attach lets go of it)
                        lane.eng.play_attach(self.seed, self.temperature, self._queue_ids, self._queue_ctl, ring_steps=2)
                    lane.eng.set_forced_playouts(k)
                lane.move_graph = None
        self.forced_k, self.forced_prune = k, bool(prune)
        self.book.set_column('raw', (np.int32, (self.eng.n_actions, ), 'move') if k > 0.0 else None)
        if rewarm:
            self.warm_graphs()
        if was_dev:
            self.device_attach(queue_capacity=self._queue_ids.numel(), **self._attach_kw)

    def set_root_values(self, on=True):
        """Keep the root value of every search that plays a ply (an opt-in extension: the learner's value target can mix it with z,
        DeviceReplay.set_value_mix / Trajectory.training_samples(value_mix=)), for every lane and BOTH loops (run, run_device):
        Trajectory.root_values, float32 [plies] -- float32 of MCTSEngine.root_values()[:, 0], -W / N of the root, as the draw saw it.
        run reads it after its search; the device move step writes it into a side ring of its log (rz_play_set_root_values), which
        is an argument of the draw: an attached object attaches again (same settings) when the option changes.  Games, moves, pis
        and the log's records do not depend on it.  ValueError while a lane's engine is in match mode."""
        on = bool(on)
        if on and any(getattr(lane.eng, 'play_match_on', False) for lane in self.lanes):
            raise ValueError('a lane\'s engine is in match mode (play_set_match): a match logs no root values')
        if self._streaming and on != self.root_values_on:
            raise ValueError('a stream is open (stream_start): the root values are an argument of its move step -- set them before stream_start')
        changed, self.root_values_on = on != self.root_values_on, on
        if self._dev_on and changed:
            self.device_attach(queue_capacity=self._queue_ids.numel(), **self._attach_kw)

    def set_playout_cap(self, n_fast, p_full=None):
        """Playout cap randomization (KataGo, Wu 2019, section 3.1; an opt-in extension) for every lane and BOTH loops (run,
        run_device): the search before ply ``ply`` of game ``gid`` has n_playout simulations when cap_uniform(seed, gid, ply) <
        ``p_full`` and ``n_fast`` otherwise, so a game depends on (seed, game id, cap) only.  Trajectory.full tells which plies had
        the full budget; Trajectory.training_samples() keeps those.  ``n_fast`` None: off.  Between runs; like set_resign, the first
        cap on an attached object whose whole-move graphs were captured without one attaches again, later values reach the graphs
        as they are.  Dirichlet noise and temperature are untouched: KataGo also drops the noise on fast moves, which is
        deliberately out of scope here.  ValueError for values out of range and for lanes without a resident search (two-launch
        lanes, PUCT, sims_in_flight > 1, host evaluators)."""
        self._stream_guard('play_cap_on', n_fast is not None)
        if n_fast is None:
            self.playout_cap = None
            for lane in self.lanes:
                with self._on(lane):
                    lane.eng.set_playouts(None)
        else:
            n_fast, p_full = int(n_fast), float(p_full if p_full is not None else 'nan')
            if self.forced_k > 0.0:
                raise ValueError('forced playouts are on (set_forced_playouts): the playout cap is a rule of the uct_ref search')
            if not 1 <= n_fast <= self.eng.n_playout:
                raise ValueError('n_fast %d not in 1 .. n_playout = %d' % (n_fast, self.eng.n_playout))
            if not 0.0 < p_full <= 1.0:
                raise ValueError('p_full %r not in (0, 1]' % p_full)
            for lane in self.lanes:
                r_lane = lane.eng._ask(lane.evaluator)[0]
                if not (r_lane.resident and r_lane.deferred):   # (the resident search under PUCT has no per-game budgets)
                    raise ValueError('the playout cap needs the resident search on every lane (this route has none: two-launch lanes, '
                                     'PUCT, sims_in_flight > 1 and host evaluators search every game alike)')
            self.playout_cap = (n_fast, p_full)
        self._apply_option(self._cap_option())
        self._open_epoch()

    def set_temperature_schedule(self, temps, pi_temperature=None):
        """A per-ply move temperature (an opt-in extension: the reference's self-play has one T) for every lane and BOTH loops (run,
        run_device): ``temps[p]`` is T before ply p and the last entry holds for every later ply -- step_schedule (AlphaGo Zero /
        AlphaZero: T = 1 for the opening, then T -> 0) and decay_schedule (KataGo's half-life) build such tables.  None: off, every ply
        at ``temperature`` again.  A game still depends on (seed, game id, settings) only: T follows from the ply.  Between runs,
        before or after device_attach; like set_resign, the first schedule on an attached object whose whole-move graphs were
        captured without one attaches again, later tables reach the graphs as they are.  Dirichlet noise is untouched, and
        KataGo's "no temperature on fast moves" of a playout cap is deliberately out of scope.
        ``pi_temperature``: None keeps the reference's rule -- the stored pi is the move distribution at the ply's T
        (alphazero_mcts.py:88-92), one-hot where the schedule has cooled; a float forms Trajectory.pis with visits_to_pi at that T
        instead, the moves still drawn at the ply's T (host side only, the same in both loops).
        ValueError for entries that are not finite and positive, for more entries than the board has cells, and for a lane whose
        engine is in match mode (a match keeps its own T)."""
        if pi_temperature is not None:
            pi_temperature = float(pi_temperature)
            if not (np.isfinite(pi_temperature) and pi_temperature > 0.0):
                raise ValueError('pi_temperature %r is not finite and positive' % pi_temperature)
        tab = None if temps is None else _check_temperatures(temps, self.eng.n_cells)
        if tab is not None and any(getattr(lane.eng, 'play_match_on', False) for lane in self.lanes):
            raise ValueError('a lane\'s engine is in match mode (play_set_match): a match keeps its own temperature')
        self._stream_guard('play_temp_on', tab is not None)
        self.temperature_schedule, self.pi_temperature = tab, pi_temperature
        self._apply_option(self._temperature_option())
        self._open_epoch()

    def set_resign(self, threshold, disabled_frac=0.1):
        """AlphaGo Zero's resignation for every lane (an opt-in extension: the reference plays every game to its end): the player to
        move resigns when both v_root and q_best of its search (MCTSEngine.root_values) are below ``threshold``, except in the
        calibration games -- resign_uniform(seed, game id) < ``disabled_frac`` -- which are played out and measure the false
        positives (Trajectory.fp_margin, calibrate_resign_threshold).  ``threshold`` None / NaN: off.  Before or after
        device_attach, between runs; the first rule on an attached object whose whole-move graphs were captured without one
        attaches again (same settings) so that they are captured with it -- a later threshold reaches the graphs as it is."""
        threshold = float('nan') if threshold is None else float(threshold)
        disabled_frac = float(disabled_frac)
        if not 0.0 <= disabled_frac <= 1.0:
            raise ValueError('disabled_frac %r not in [0, 1]' % disabled_frac)
        self._stream_guard('play_resign_on', not np.isnan(threshold))
        self.resign_threshold, self.resign_disabled_frac = threshold, disabled_frac
        self._apply_option(self._resign_option())
        self._open_epoch()

    # An option of the device move step: (on here, the engine's attribute that says it is on there, how to hand it to an engine)
    def _resign_option(self):
        return self.resign_on, 'play_resign_on', lambda eng: eng.play_set_resign(self.resign_threshold, self.resign_disabled_frac)

    def _cap_option(self):
        return self.playout_cap is not None, 'play_cap_on', lambda eng: eng.play_set_cap(*(self.playout_cap or (1, float('nan'))))

    def _temperature_option(self):
        return self.temperature_schedule is not None, 'play_temp_on', lambda eng: eng.play_set_temperatures(self.temperature_schedule)

    def _apply_option(self, option, attaching=None):
        """Hand an option to the lanes' engines after its setter, or (``attaching``: a lane, inside device_attach's stream context)
        before that lane's whole-move graph is captured, so that the graph reads the option's buffer.  After a setter: nothing while
        the move step is not attached; an option turned on over a graph captured without it attaches again with the same settings;
        otherwise the lanes where it is on, or being turned on, take the new value as they are."""
        on, flag, apply = option
        if attaching is not None:
            if on:
                apply(attaching.eng)
        elif not self._dev_on:
            return
        elif on and any(lane.move_graph is not None and not getattr(lane.eng, flag) for lane in self.lanes):
            self.device_attach(queue_capacity=self._queue_ids.numel(), **self._attach_kw)
        else:
            for lane in self.lanes:
                if on or getattr(lane.eng, flag):
                    with self._on(lane):
                        apply(lane.eng)

    @classmethod
    def for_network(cls, net_module, board, n_in_row, n_games, n_playout, c_puct=5.0, device='cuda:0',
                    game='gomoku', net_shape=None, lanes=None, trunk_workgroups=None, temperature=1.0, seed=0,
                    use_graph=True, sims_per_graph=16, eager_every=0, add_noise=True, sims_in_flight=1, before_warm=None,
                    deferred_priors=None, resident_search=None, net_algo=None, delta_trunk=None, resign=None, playout_cap=None,
                    temperature_schedule=None, pi_temperature=None, root_values=False, resident_puct=False, forced_playouts=None,
                    **engine_kw):
        """Self-play of ``n_games`` games in flight with the hand-written evaluator of ``net_module`` (a
        PolicyValueNet): builds the lanes (engine + HipNetEvaluator each) as plan_lanes() recommends, unless
        ``lanes`` / ``trunk_workgroups`` are given (more than four lanes take turns on the GPU's four compute pipes, and four need
        GPU_MAX_HW_QUEUES >= 8: profiles/r03/lane_sweeps.txt).  ``add_noise``: Dirichlet noise on the priors of every expanded
        node, what ``AlphaZeroPlayer(is_selfplay=True)`` does (alphazero_mcts.py:124-129, node.py:63-69).
        ``lanes``: None = the table (plan_lanes) on the chip it was measured on, the measuring fallback elsewhere (another CU count:
        the table's pick and its neighbours are built and timed for two moves each, choose_lanes_by_measurement); 'measure' forces the
        measurement, 'table' the table; an int is taken as given.
        ``sims_in_flight`` = K > 1: the opt-in virtual-loss mode (MCTSEngine), for batches too small to fill the GPU
        with one leaf per game; the evaluator batch of a lane is then its games x K.  ``deferred_priors``: None = the deferred-priors
        route wherever it exists (HipNetEvaluator.deferred_ok), False = the three-launch step everywhere; ``resident_search`` likewise for
        the one-launch-per-search kernel of batches that give every game a CU (False = the two-launch step).  ``before_warm(sp)``: called
        before the hipGraphs are captured (rlzero_amd.trace attaches its buffer there).  ``net_algo``: HipNet.set_algo for every lane's
        evaluator -- None keeps the default ('split_f16', the f32-accurate trunk); 'split_f16_fp8' is the OPT-IN arithmetic narrower than
        the reference's f32 (boards of 11 .. 16 rows and columns).  ``delta_trunk``: False = the full-board trunk on every leaf (the
        checker of the receptive-field evaluation, HipNetEvaluator.delta_trunk; with it goes the resident search's second game per CU).
        ``resign``: None (off) or a threshold or (threshold, disabled_frac): set_resign.  ``playout_cap``: None (off) or (n_fast, p_full):
        set_playout_cap.  ``temperature_schedule``: None (off) or a table of per-ply temperatures, with ``pi_temperature``:
        set_temperature_schedule.  ``root_values``: set_root_values.
        ``resident_puct`` (opt-in, with ``score_mode='puct'``): every lane searches with the one-launch resident search under PUCT
        (HipNetEvaluator.resident_puct: boards of up to 10 rows and columns, one simulation in flight, at most one game per CU and
        lane) -- run, run_device and the whole-move hipGraphs then play the games of the three-launch step, bit for bit.  ValueError
        where it cannot be served (plan_route names the reason); nothing falls back to another route.
        ``forced_playouts``: None (off) or k, or (k, prune): set_forced_playouts."""
        import torch
        from .engine import HipNetEvaluator, MCTSEngine
        dev = torch.device(device)
        n_cus = torch.cuda.get_device_properties(dev).multi_processor_count
        K = max(1, int(sims_in_flight))
        shape0 = net_shape if net_shape is not None else board
        rows0, cols0 = (shape0[0], shape0[1]) if isinstance(shape0, (tuple, list)) else (shape0, shape0)
        planned = plan_route(rows0, cols0, game, net_algo, engine_kw.get('score_mode', 'uct_ref'), K, deferred_priors=deferred_priors,
                             delta_trunk=delta_trunk, resident_search=resident_search, n_games=n_games, n_cus=n_cus,
                             resident_puct=resident_puct, lanes=lanes if isinstance(lanes, int) else None)
        deferred = planned['deferred']
        auto_lanes, auto_wgs, heads_algo = plan_lanes(n_games * K, n_cus, **planned)
        measured = None
        if lanes == 'table':
            lanes = None
        elif K > 1:
            # K simulations in flight: the timer's move step (rz_play_attach) serves one simulation in flight per tree only -- the table
            lanes = None if lanes == 'measure' else lanes
        elif lanes == 'measure' or (lanes is None and n_cus != TABLE_CUS and n_games * K > n_cus):
            # off the table's chip (or asked for): the table's pick and its neighbours, timed for two moves each
            from . import HW_QUEUES
            key = (torch.cuda.get_device_name(dev), n_cus, rows0, cols0, game, n_games, n_playout, K, bool(deferred), str(net_algo))

            def build(n_lanes):
                return cls.for_network(net_module, board, n_in_row, n_games, n_playout, c_puct=c_puct, device=device, game=game,
                                       net_shape=net_shape, lanes=n_lanes, trunk_workgroups=trunk_workgroups, temperature=temperature,
                                       seed=seed, use_graph=use_graph, sims_per_graph=sims_per_graph, add_noise=add_noise,
                                       sims_in_flight=sims_in_flight, deferred_priors=deferred_priors, resident_search=resident_search,
                                       net_algo=net_algo, delta_trunk=delta_trunk, resident_puct=resident_puct, **engine_kw)
            lanes, measured = choose_lanes_by_measurement(key, auto_lanes, HW_QUEUES, n_games, build)
        if lanes is None:
            lanes, wgs = auto_lanes, auto_wgs
        else:
            wgs, heads_algo = (0, 'parts') if lanes > 1 else (0, 'auto')
        if trunk_workgroups is not None:
            wgs = trunk_workgroups
        acts = shape0[2] if isinstance(shape0, (tuple, list)) and len(shape0) > 2 else rows0 * cols0
        if heads_algo == 'parts' and int(wgs) == 0 and fc_in_trunk_pays(rows0, cols0, acts):
            heads_algo = 'in_trunk'   # small FC layers: no GEMM launch at all (each lane's chain loses a kernel and a boundary)
        lanes = max(1, min(int(lanes), n_games))
        per_lane = [n_games // lanes + (1 if i < n_games % lanes else 0) for i in range(lanes)]
        engines, evaluators = [], []
        for g_lane in per_lane:
            engines.append(MCTSEngine(board, n_in_row, n_games=g_lane, n_playout=n_playout, c_puct=c_puct,
                                      device=str(device), game=game, add_noise=add_noise, sims_in_flight=K,
                                      noise_seed=(int(seed) * 7919 + len(engines)) & 0x7fffffff, **engine_kw))
            ev = HipNetEvaluator(net_module, shape0, str(device), max_boards=g_lane * K)
            if net_algo is not None:
                ev.hip.set_algo(net_algo)
            ev.hip.set_max_workgroups(max(0, int(wgs)))
            ev.hip.set_heads_algo(heads_algo)
            if deferred_priors is not None:
                ev.deferred_priors = bool(deferred_priors)
            if resident_search is not None:
                ev.resident_search = bool(resident_search)
            if delta_trunk is not None:
                ev.delta_trunk = bool(delta_trunk)
            ev.resident_puct = bool(resident_puct)
            evaluators.append(ev)
        sp = cls(engines if lanes > 1 else engines[0], evaluators if lanes > 1 else evaluators[0],
                 temperature=temperature, seed=seed, use_graph=use_graph, sims_per_graph=sims_per_graph,
                 eager_every=eager_every)
        if resident_puct:
            for lane in sp.lanes:   # (what plan_route could not see: the net's weights, the lanes as built)
                if not lane.eng._ask(lane.evaluator)[0].resident:
                    for other in sp.lanes:
                        other.eng.close()
                    raise ValueError('resident_puct=True cannot be served: a lane of %d games does not take the resident route '
                                     '(weights without finite activation bounds, or more games than CUs)' % lane.eng.n_games)
        sp.trunk_workgroups = int(wgs)
        sp.lanes_measured = measured   # {lanes: simulations / s} when the layout was chosen by measurement, else None
        if resign is not None:
            sp.set_resign(*(resign if isinstance(resign, (tuple, list)) else (resign, )))
        if playout_cap is not None:
            sp.set_playout_cap(*playout_cap)
        if temperature_schedule is not None or pi_temperature is not None:
            sp.set_temperature_schedule(temperature_schedule, pi_temperature=pi_temperature)
        if root_values:
            sp.set_root_values(True)
        if forced_playouts is not None:
            try:
                sp.set_forced_playouts(*(forced_playouts if isinstance(forced_playouts, (tuple, list)) else (forced_playouts, )))
            except ValueError:
                for lane in sp.lanes:
                    lane.eng.close()
                raise
        if before_warm is not None:
            before_warm(sp)
        sp.warm_graphs()
        return sp

    def warm_graphs(self):
        """Capture the simulation-chunk hipGraph of every lane (before any game is started: the capture
        runs the chunk once).  Weight updates keep the graphs valid: rz_net_load reuses its device buffers.  Weights that change
        the evaluation route (HipNetEvaluator.refresh: no finite activation bound, or finite again) drop them, and the lane's next
        replay raises HipError instead of running the old route: call warm_graphs (or device_attach) again before the next run."""
        if not self.use_graph:
            return
        per = self.eng.graph_chunk(self.sims_per_graph)
        for lane in self.lanes:
            with self._on(lane):
                lane.eng.reset_games()
                lane.eng.warm_graph(lane.evaluator, per)
        self.torch.cuda.synchronize()

    def refresh_weights(self):
        """Re-upload the network weights of every lane if the torch module changed (after a learner step).  Captured graphs stay
        valid unless the new weights change the evaluation route (see warm_graphs): they are then dropped, not captured again."""
        for lane in self.lanes:
            refresh = getattr(lane.evaluator, 'refresh_if_changed', None)
            if refresh is not None:
                refresh(content=True)
        self._open_epoch()   # (a stream: the moves enqueued from here on search with these weights)

    def _on(self, lane):
        return self.torch.cuda.stream(lane.stream)

    # -- slot management -----------------------------------------------------------
    def _start(self, slots, game_ids):
        mask = np.zeros(self.n_slots, dtype=np.uint8)
        for s, g in zip(slots, game_ids):
            mask[s] = 1
            self.book.start(s, g)
            self.cell_taken[s] = False
        # a game's Dirichlet noise (read by the PUCT rule only), like its move draws, is keyed by (seed, game id): the trajectory
        # does not depend on the slot, lane or GPU the game is played on
        with np.errstate(over='ignore'):
            keys = _splitmix64(_splitmix64(np.uint64(self.seed) ^ np.uint64(0x6E6F697365000000)) ^ self.slot_game.astype(np.uint64))
        for lane in self.lanes:
            if mask[lane.slots].any():
                if lane.primed:
                    # a pipelined run that stopped early (max_moves) left the next move's simulations enqueued: they end
                    # on the old roots, and the trees reset here must not be taken for searched ones
                    lane.stream.synchronize()
                    lane.primed = False
                with self._on(lane):
                    lane.eng.reset_games(mask=mask[lane.slots])
                    lane.eng.set_noise_keys(keys[lane.slots], mask=mask[lane.slots])

    def _set_active(self):
        active = (self.slot_game >= 0).astype(np.uint8)
        for lane in self.lanes:
            with self._on(lane):
                lane.eng.set_active(active[lane.slots])

    def _simulate(self):
        if any(lane.primed for lane in self.lanes):
            # a lane primed by play_move_pipelined has the coming move's simulations in flight already: searching it again
            # would double its visits -- the lanes are taken one by one, the primed ones as they are
            for lane in self.lanes:
                if not lane.primed:
                    self._simulate_lane(lane)
                lane.primed = False
            return
        n = self.eng.n_playout
        if all(lane.eng._ask(lane.evaluator)[0].resident for lane in self.lanes):
            for lane in self.lanes:   # one launch per lane for the whole search: nothing to interleave, no graph
                self._simulate_lane(lane)
            return
        if self.use_graph:
            per = self.eng.graph_chunk(self.sims_per_graph)
            full, n = divmod(n, per)
            for _ in range(full):
                # timing samples: every k-th chunk of the run (counted across moves) is launched eagerly
                c = self._chunks_done = self._chunks_done + 1
                eager = self.eager_every > 0 and c % self.eager_every == 0
                for lane in self.lanes:
                    with self._on(lane):
                        if eager:
                            lane.eng.sim_chunk(lane.evaluator, per)
                        else:
                            lane.eng.simulate(lane.evaluator, per, use_graph=True, sims_per_graph=per)
        if n and len(self.lanes) == 1:
            lane = self.lanes[0]
            with self._on(lane):
                lane.eng.sim_chunk(lane.evaluator, n)
        elif n:
            # interleave the lanes in chunks so that their kernels alternate on the device
            chunk = self.eng.graph_chunk(8)
            for c0 in range(0, n, chunk):
                for lane in self.lanes:
                    with self._on(lane):
                        lane.eng.sim_chunk(lane.evaluator, min(chunk, n - c0))

    def _simulate_lane(self, lane, host_counts=True):
        """Enqueue the n_playout simulations of ONE lane on its stream (graph replays + the eager remainder).  ``host_counts``: under
        a playout cap the budgets come from here (the host-driven loop); False: from the device's move step."""
        n = self.eng.n_playout
        with self._on(lane):
            r = lane.eng._ask(lane.evaluator)[0]
            if host_counts and self.playout_cap is not None:
                gids, plies = self.slot_game[lane.slots], self.slot_ply[lane.slots]
                full = self._full(np.maximum(gids, 0), plies) | (gids < 0)   # (an idle slot is not searched)
                lane.eng.set_playouts(np.where(full, n, self.playout_cap[0]).astype(np.int32), longest_first=self.cap_longest_first)
            if r.resident:   # one launch for the whole search: no graph, no chunks
                lane.eng.sim_chunk(lane.evaluator, n, r)
                return
            if self.use_graph:
                per = self.eng.graph_chunk(self.sims_per_graph)
                full, n = divmod(n, per)
                for _ in range(full):
                    c = self._chunks_done = self._chunks_done + 1
                    if self.eager_every > 0 and c % self.eager_every == 0:
                        lane.eng.sim_chunk(lane.evaluator, per)
                    else:
                        lane.eng.simulate(lane.evaluator, per, use_graph=True, sims_per_graph=per)
            if n:
                lane.eng.sim_chunk(lane.evaluator, n)

    # -- one move for every running game ----------------------------------------------
    def _fetch_lane(self, lane, running):
        """What the lane's search left for its ``running`` slots, read on the lane's stream (synchronises that stream only) ->
        (visits, root values or None, pruned counts or None), a row per slot."""
        at = running - lane.slots.start
        vals = pruned = None
        with self._on(lane):
            visits = lane.eng.root_visits()
            # the split-f16 trunk reports an input outside its range: float planes only (positions are 0 / 1 planes by construction,
            # and the query waits for the device)
            if hasattr(getattr(lane.evaluator, 'hip', None), 'check_flags') and getattr(lane.evaluator, 'needs_obs', True):
                lane.evaluator.hip.check_flags()
            if (self.resign_on or self.root_values_on) and len(running):
                vals = lane.eng.root_values()[at]
            if self.forced_k > 0.0 and self.forced_prune and len(running):
                pruned = lane.eng.root_pruned_visits()[at]
        return visits[at], vals, pruned

    def _apply_lane(self, lane, running, chosen, quit_):
        """The moves of ``decide_and_record`` on the lane's boards and trees: the host's mirror, tree reuse and the game step, then
        the ended and the resigned games out of the book -> their trajectories."""
        eng, lo = lane.eng, lane.slots.start
        moves = np.full(eng.n_games, -2, dtype=np.int32)
        moves[running - lo] = chosen   # (-1 where the mover resigns: no move, the tree is dropped like reset_player at a game's end)
        played, cells = running[~quit_], chosen[~quit_]
        if eng.game == 'connect4':   # action = column: the stone drops
            heights = self.cell_taken[played].reshape(len(played), eng.rows, eng.cols).sum(axis=1)
            cells = heights[np.arange(len(played)), cells] * eng.cols + cells
        self.cell_taken[played, cells] = True
        with self._on(lane):
            winner, ended = eng.advance_and_step(moves, np.where(moves >= 0, moves, -1).astype(np.int32))  # tree reuse before the boards change
        done = []
        for s, gone in zip(running, quit_):
            if gone or ended[s - lo]:   # (player 0 moves the even plies: the mover who resigns loses)
                done.append(self.trajectory(self.book.close(s, 1 - int(self.slot_ply[s]) % 2 if gone else int(winner[s - lo]), bool(gone))))
        return done

    def _finish_lane(self, lane):
        """The move of one lane after its simulations: root visits -> pi -> move drawn (alphazero_mcts.py:88-92,148),
        tree reuse, game step.  Synchronises that lane's stream only.  Returns the trajectories that ended."""
        running = lane.slots.start + np.nonzero(self.slot_game[lane.slots] >= 0)[0]
        visits, vals, pruned = self._fetch_lane(lane, running)
        legal = ~self.cell_taken[running]
        if lane.eng.game == 'connect4':   # action = column, legal while its top cell is empty
            legal = legal[:, (lane.eng.rows - 1) * lane.eng.cols:]
        return self._apply_lane(lane, running, *self.decide_and_record(running, visits, legal, vals, pruned))

    def play_move(self):
        """n_playout simulations, then pick / apply one move per game.  Returns the list of
        trajectories of the games that ended with this move."""
        self._simulate()
        done = []
        for lane in self.lanes:
            done.extend(self._finish_lane(lane))
        return done

    def play_move_pipelined(self, refill=None):
        """play_move() with the host side of one lane's move hidden under the other lanes' simulations: per lane, wait
        for ITS simulations, draw and apply its moves, refill its finished slots (``refill(n) -> up to n new game
        ids``, optional) and enqueue its NEXT move's simulations at once -- while a lane is on the host the others keep
        the GPU busy.  Every call completes exactly one move of every running game, like play_move(); between calls
        the simulations of the coming move are already in flight.  Results are those of play_move(): games are
        independent and their uniforms are keyed by (game, ply)."""
        for lane in self.lanes:
            if not lane.primed and (self.slot_game[lane.slots] >= 0).any():
                self._simulate_lane(lane)
                lane.primed = True
        done_all = []
        for lane in self.lanes:
            if not lane.primed:
                continue
            done = self._finish_lane(lane)
            lane.primed = False
            if done:
                if refill is not None:
                    free = lane.slots.start + np.nonzero(self.slot_game[lane.slots] < 0)[0]
                    ids = list(refill(len(free)))[:len(free)]
                    if ids:
                        self._start(free[:len(ids)], ids)
                self._retire_lane(lane)
            if (self.slot_game[lane.slots] >= 0).any():
                self._simulate_lane(lane)
                lane.primed = True
            done_all.extend(done)
        return done_all

    def _retire_lane(self, lane):
        idle = np.full(lane.eng.n_games, -2, dtype=np.int32)
        idle[np.nonzero(self.slot_game[lane.slots] < 0)[0]] = -1
        with self._on(lane):
            lane.eng.advance(idle)
            lane.eng.set_active((self.slot_game[lane.slots] >= 0).astype(np.uint8))

    def retire_finished(self):
        """reset_player(): discard the trees of idle slots (game.py:128) and mask them out."""
        for lane in self.lanes:
            self._retire_lane(lane)

    def abandon_running(self):
        """Drop every game still in a slot (a run that stopped early -- max_moves -- leaves its games there, and a pipelined one
        leaves their NEXT search finished on the device as well): the slots become idle, their trees are reset, no lane stays
        primed.  run() starts with this: games of an earlier run are neither played on nor searched a second time on top of a
        finished search."""
        if not (self.slot_game >= 0).any() and not any(lane.primed for lane in self.lanes):
            return
        self.slot_game[:] = -1
        for lane in self.lanes:
            if lane.primed:
                lane.stream.synchronize()
                lane.primed = False
            self._retire_lane(lane)

    def check(self):
        return [lane.eng.check() for lane in self.lanes]

    def run(self, game_ids, max_moves=None, pipelined=False):
        """Play all ``game_ids`` to the end; returns trajectories sorted by game id.  ``pipelined``: the host side of a
        lane's move under the other lanes' simulations (play_move_pipelined); same trajectories."""
        self._no_stream('run')
        self.abandon_running()
        if pipelined:
            return self._run_pipelined(game_ids, max_moves)
        pending = list(game_ids)
        G = self.n_slots
        first = pending[:G]
        pending = pending[G:]
        self._start(range(len(first)), first)
        self._set_active()
        out = []
        n_moves = 0
        while (self.slot_game >= 0).any():
            done = self.play_move()
            out.extend(done)
            n_moves += 1
            free = np.nonzero(self.slot_game < 0)[0]
            if done and pending:
                take = pending[:len(free)]
                pending = pending[len(take):]
                self._start(free[:len(take)], take)
            if done:
                self.retire_finished()
            if max_moves is not None and n_moves >= max_moves:
                break
        self.check()
        return sorted(out, key=lambda t: t.game_id)


    def _run_pipelined(self, game_ids, max_moves=None):
        pending = list(game_ids)
        first, pending = pending[:self.n_slots], pending[self.n_slots:]
        self._start(range(len(first)), first)
        self._set_active()

        def refill(n):
            take = pending[:n]
            del pending[:n]
            return take

        out, n_moves = [], 0
        while (self.slot_game >= 0).any():
            out.extend(self.play_move_pipelined(refill))
            n_moves += 1
            if max_moves is not None and n_moves >= max_moves:
                break
        self.torch.cuda.synchronize()   # (lanes still primed hold a finished search: play_move() / play_move_pipelined() use it)
        self.check()
        return sorted(out, key=lambda t: t.game_id)


    # -- the move step on the device (include/rlzero_hip.h: rz_play_*) -----------------------------------------------
    # The host enqueues whole moves -- search, draw, priors, tree reuse, game step, end / refill of slots -- and never waits for
    # one: what happened comes back through each lane's log, read behind the GPU.  pi is formed HERE, from the logged visit
    # counts with the reference's numpy expression (alphazero_mcts.py:10-14,91-92), and every move the device drew is checked
    # against numpy's inverse-CDF draw on the same uniform (a mismatch raises; a draw too close to an interval edge was never
    # made by the device: the slot stalls until the move computed here is handed back).  Same trajectories as play_move().
    def device_attach(self, queue_capacity=1 << 16, ring_steps=64, depth=None, copy_every=None, stall_margin=0.0, move_graphs=True,
                      _ring=False):
        """Switch this object to device-driven moves.  ``copy_every``: moves of a lane per read-back of its log rows (None: 1, or
        8 when a move is a fraction of a millisecond -- boards of a few cells with few simulations); ``depth``: read-backs a lane
        may be ahead of the rows processed here (None: 1 when a move is long, else 2).  ``move_graphs``: a lane whose search is the
        one-launch resident kernel replays its WHOLE move -- selection, search, draw, priors, tree reuse, game step, refill -- from
        one hipGraph."""
        t = self.torch
        from ._hip import PLAY_RECORD_WORDS
        dev = self.eng.device
        if self._streaming and not _ring:
            raise ValueError('a stream is open (stream_start): stream_stop ends it before the move step is attached again')
        if self._dev_on:
            self.device_stop()
        self._attach_kw = dict(ring_steps=ring_steps, depth=depth, copy_every=copy_every, stall_margin=stall_margin, move_graphs=move_graphs)
        t.cuda.synchronize(dev)
        work = self.eng.n_playout * self.eng.n_cells   # ~ the length of a move
        self._copy_every = int(copy_every) if copy_every else (1 if work >= 4000 else 8)
        self._depth = int(depth) if depth else (1 if work >= 100000 else 2)
        ring_steps = max(int(ring_steps), self._copy_every * (self._depth + 2) + 2)
        if _ring:   # (a stream: the queue is a ring of at least what the top-up keeps pushed)
            least = stream_topup(self.n_slots, self._copy_every, self._depth)
            if queue_capacity is not None and int(queue_capacity) < least:
                raise ValueError('a ring of %d game ids: the top-up of %d slots, copy_every %d, depth %d needs %d (stream_topup)' % (
                    queue_capacity, self.n_slots, self._copy_every, self._depth, least))
            queue_capacity = least if queue_capacity is None else int(queue_capacity)
        self._queue_ids = t.zeros(int(queue_capacity), dtype=t.int64, device=dev)
        self._queue_ctl = t.zeros(2, dtype=t.int32, device=dev)
        self._queue_len, self._started = 0, 0
        words = PLAY_RECORD_WORDS + self.eng.n_actions
        for lane in self.lanes:
            with self._on(lane):
                lane.eng.play_attach(self.seed, self.temperature, self._queue_ids, self._queue_ctl, ring_steps=ring_steps,
                                     stall_margin=stall_margin)
                if _ring:   # (an argument of the move step: before it is enqueued or captured)
                    lane.eng.play_queue_ring(queue_capacity)
                self._apply_option(self._resign_option(), attaching=lane)
                lane.eng.set_playouts(None)   # (the device's budgets, not a host-driven run's last counts)
                lane.eng.play_set_cap_order(self.cap_longest_first)
                self._apply_option(self._cap_option(), attaching=lane)
                self._apply_option(self._temperature_option(), attaching=lane)
                if self.root_values_on:   # (an argument of the draw: before the first move step is enqueued or captured)
                    lane.eng.play_set_root_values(True)
                if self.forced_k > 0.0 and self.forced_prune:   # (a launch in front of the draw: likewise)
                    lane.eng.play_set_pruned_visits(True)
                lane.move_graph = lane.eng.warm_move_graph(lane.evaluator) if move_graphs else None
            # (the engine's log ring is pinned host memory that its kernels write directly: nothing to copy -- or, RZ_PLAY_DEVICE_LOG=1,
            # a device ring whose rows _read_back copies)
            lane.host_log = lane.eng.play_log if lane.eng.play_log_on_host else t.empty((int(ring_steps), lane.eng.n_games, words), dtype=t.int32, pin_memory=True)
            lane.host_np = lane.host_log.numpy()
            lane.values_np = None   # (set_root_values: the side ring's rows, where the log's are)
            if self.root_values_on:
                ring = lane.eng.play_values
                lane.host_values = ring if lane.eng.play_log_on_host else t.empty(tuple(ring.shape), dtype=t.float32, pin_memory=True)
                lane.values_np = lane.host_values.numpy()
            lane.pruned_np = None   # (set_forced_playouts: the rows of the pruned counts' ring, where the log's are)
            if self.forced_k > 0.0 and self.forced_prune:
                ring = lane.eng.play_pruned
                lane.host_pruned = ring if lane.eng.play_log_on_host else t.empty(tuple(ring.shape), dtype=t.int32, pin_memory=True)
                lane.pruned_np = lane.host_pruned.numpy()
            lane.uncopied = []          # rows written by enqueued moves, their read-back not enqueued yet
            lane.inflight = []          # [(rows, event)] read-backs enqueued, oldest first
            lane.last_running = -1      # RUNNING records in the last row read (-1: none read yet)
            lane.primed = False
        self.book.clear()
        self.stalls_resolved = 0
        self._dev_on = True
        t.cuda.synchronize(dev)

    def device_queue(self, game_ids):
        """Replace the queue of waiting game ids (synchronises: not for the middle of a run) and let idle slots take from it."""
        t = self.torch
        self._no_stream('device_queue')
        ids = np.ascontiguousarray(list(game_ids), dtype=np.int64)
        if ids.size > self._queue_ids.numel():
            raise ValueError('%d game ids for a queue of %d: device_attach(queue_capacity=...)' % (ids.size, self._queue_ids.numel()))
        t.cuda.synchronize(self.eng.device)
        self._queue_ids[:ids.size].copy_(t.from_numpy(ids))
        self._queue_ctl.copy_(t.tensor([0, ids.size], dtype=t.int32))
        t.cuda.synchronize(self.eng.device)
        self._queue_len, self._started = int(ids.size), 0
        for lane in self.lanes:
            with self._on(lane):
                lane.eng.play_refill()
            lane.last_running = -1

    def _lane_quiet(self, lane):
        """Nothing left to do on this lane, as far as the rows read so far can tell (the host's view lags the device by design)."""
        return not lane.inflight and not lane.uncopied and lane.last_running == 0 and self._started >= self._queue_len

    def _read_back(self, lane):
        """An event behind the lane's new log rows (they are in pinned memory when it has passed: written there by the kernels, or
        -- a device ring -- copied there, contiguous runs of the ring in one copy each)."""
        rows = lane.uncopied
        if not rows:
            return
        lane.uncopied = []
        with self._on(lane):
            at = 0
            while at < len(rows):
                end = at + 1
                while end < len(rows) and rows[end] == rows[end - 1] + 1:
                    end += 1
                if not lane.eng.play_log_on_host:
                    lane.host_log[rows[at]:rows[end - 1] + 1].copy_(lane.eng.play_log[rows[at]:rows[end - 1] + 1], non_blocking=True)
                    if lane.values_np is not None:
                        lane.host_values[rows[at]:rows[end - 1] + 1].copy_(lane.eng.play_values[rows[at]:rows[end - 1] + 1], non_blocking=True)
                    if lane.pruned_np is not None:
                        lane.host_pruned[rows[at]:rows[end - 1] + 1].copy_(lane.eng.play_pruned[rows[at]:rows[end - 1] + 1], non_blocking=True)
                at = end
            ev = self.torch.cuda.Event()
            ev.record(lane.stream)
        lane.inflight.append((rows, ev))

    def play_move_device(self):
        """Enqueue ONE more move of every lane that may still have games and process the log rows that have arrived
        -> the trajectories of the games found finished in them."""
        for lane in self.lanes:
            if self._lane_quiet(lane):
                continue
            if lane.move_graph is not None:
                with self._on(lane):
                    lane.uncopied.append(lane.eng.play_move_replay(lane.move_graph))
            else:
                self._simulate_lane(lane, host_counts=False)
                with self._on(lane):
                    lane.uncopied.append(lane.eng.play_move())
            if len(lane.uncopied) >= self._copy_every:
                self._read_back(lane)
        done = []
        for lane in self.lanes:
            done.extend(self._harvest(lane, keep=self._depth))
        return done

    def device_drain(self):
        """Wait for every enqueued move and process its row -> the finished trajectories found."""
        done = []
        for lane in self.lanes:
            self._read_back(lane)
        for lane in self.lanes:
            done.extend(self._harvest(lane, keep=0))
        return done

    def _harvest(self, lane, keep):
        """The lane's log rows whose read-back has passed (all but the ``keep`` newest, and those only if ready) -> the finished games."""
        rows = []
        while lane.inflight and (len(lane.inflight) > keep or lane.inflight[0][1].query()):
            batch, ev = lane.inflight.pop(0)
            ev.synchronize()
            rows.extend(batch)
        if not rows:
            return []
        # (host_np[rows] is a copy: the pinned rows may be overwritten from now on)
        done, lane.last_running = self.read_rows(lane.host_np[rows], lane.slots.start,
                                                 values=None if lane.values_np is None else lane.values_np[rows],
                                                 **({} if lane.pruned_np is None else dict(pruned=lane.pruned_np[rows])))
        return done

    def _resolve(self, slot, move):
        lane = next(lane for lane in self.lanes if lane.slots.start <= slot < lane.slots.stop)
        with self._on(lane):
            lane.eng.play_resolve(slot - lane.slots.start, move)

    def device_stop(self):
        """Drop every game and every row in flight: all slots idle (a run that stops early)."""
        for lane in self.lanes:
            lane.stream.synchronize()
            with self._on(lane):
                lane.eng.play_stop()
            lane.stream.synchronize()
            lane.inflight, lane.uncopied, lane.last_running, lane.primed = [], [], 0, False
        self.book.clear()
        self._queue_len = self._started = 0

    def run_device(self, game_ids, max_moves=None, on_finished=None):
        """run() with the move step on the device: same trajectories, sorted by game id.  ``on_finished(trajectories)``: called with the
        games found finished after every enqueued move, while the GPU searches on (a consumer's per-game work -- the trainer's
        observation planes and replay-buffer entries -- then costs the round nothing)."""
        self._no_stream('run_device')
        game_ids = list(game_ids)
        if not self._dev_on:
            self.device_attach(queue_capacity=max(len(game_ids), 1))
        elif len(game_ids) > self._queue_ids.numel():
            self.device_attach(queue_capacity=len(game_ids), **self._attach_kw)   # (a longer queue: attach again, same settings)
        else:
            self.device_stop()
        for lane in self.lanes:   # (a host-driven run's last counts: the device's budgets rule here)
            with self._on(lane):
                lane.eng.set_playouts(None)
        self.device_queue(game_ids)
        out, n_moves = [], 0
        while len(out) < len(game_ids):
            if all(self._lane_quiet(lane) for lane in self.lanes):
                raise RuntimeError('device-driven self-play went quiet with %d of %d games finished' % (len(out), len(game_ids)))
            done = self.play_move_device()
            out.extend(done)
            if on_finished is not None and done:
                on_finished(done)
            n_moves += 1
            if max_moves is not None and n_moves >= max_moves:
                break
        done = self.device_drain()
        out.extend(done)
        if on_finished is not None and done:
            on_finished(done)
        self.check()
        if len(out) < len(game_ids):
            self.device_stop()
        return sorted(out, key=lambda t: t.game_id)

    # -- a streaming collection: games keep running across the caller's rounds ---------------------------------------------------
    # run_device returns when the last of its games has ended, the slots of the finished ones idle under its stragglers.  A stream
    # never stops the device: slots refill from a RING of game ids that the host tops up (rz_play_queue_push), stream_collect(n)
    # returns once n more games have been read finished, and the others stay in flight for the next call -- on weights and settings
    # that may change under them (epochs).  What makes that reproducible: rows are read strictly in enqueue order behind
    # synchronize() -- never "when ready" --, so every host decision that reaches the device (a push, a stalled slot's move, a new
    # epoch) is enqueued at a position of the stream that depends on the log's CONTENT only; the moves enqueued and unread when a
    # call returns are a constant, stream_lookahead(copy_every, depth); and the move steps of several lanes, which share the queue,
    # are chained by events into one order (lane 0, 1, .., lane 0, ..), so which game a slot takes does not depend on timing.
    def _no_stream(self, what):
        if self._streaming:
            raise ValueError('%s: a stream is open (stream_start); stream_stop ends it' % what)

    def _stream_guard(self, flag, on):
        """A setter called while a stream is open: an option that is turned on over a whole-move graph captured without it would need
        a new attach, which would drop the games in flight."""
        if self._streaming and on and any(lane.move_graph is not None and not getattr(lane.eng, flag) for lane in self.lanes):
            raise ValueError('a stream is open (stream_start) and its whole-move graphs were captured without this option: '
                             'turn it on before stream_start (a stream takes new VALUES of an option as they are)')

    def _open_epoch(self):
        """Behind a change of weights or settings while a stream is open: the moves enqueued from here on are searched, drawn and
        verified under it -- the host notes the first log row of the epoch."""
        if self._streaming:
            self.epochs.append(self.settings(first_row=self._stream_rounds))

    @property
    def stream_epoch(self):
        """The epoch the next enqueued move belongs to (None outside a stream)."""
        return len(self.epochs) - 1 if self._streaming else None

    def _chain(self, lane):
        """Several lanes: order what this lane enqueues next behind the last link of the chain (another lane's move step or push)."""
        if len(self.lanes) > 1 and self._chain_ev is not None:
            lane.stream.wait_event(self._chain_ev)

    def _chain_link(self, lane):
        if len(self.lanes) > 1:
            self._chain_ev = self.torch.cuda.Event()
            self._chain_ev.record(lane.stream)

    def stream_start(self, first_game_id=0, queue_capacity=None, **attach_kw):
        """Open a stream: the device move step is attached as device_attach does -- ``attach_kw``: its arguments, by default those of
        the last attach; options, whole-move graphs and the root-value ring carry over --, with the queue of game ids as a ring of
        ``queue_capacity`` entries (None: the smallest the top-up allows, stream_topup).  Games get consecutive ids from
        ``first_game_id``.  Every slot starts a game and stream_lookahead moves are enqueued: from here on that many moves are
        enqueued and unread whenever a call returns.  While the stream is open refresh_weights, set_resign, set_playout_cap and
        set_temperature_schedule each open a new EPOCH: the change is enqueued in stream order behind the moves already enqueued,
        and every log row is verified under the settings of its own epoch (Trajectory.epochs).  run, run_device, device_queue and
        device_attach raise ValueError until stream_stop; so do a lane in match mode and a route without the device move step."""
        self._no_stream('stream_start')
        first_game_id = int(first_game_id)
        if first_game_id < 0:
            raise ValueError('first_game_id %d is negative' % first_game_id)
        if self.forced_k > 0.0:
            raise ValueError('forced playouts are on (set_forced_playouts): continuous self-play under PUCT is not served')
        for lane in self.lanes:
            if getattr(lane.eng, 'play_match_on', False):
                raise ValueError('a lane\'s engine is in match mode (play_set_match): a match is no stream of self-play games')
            if getattr(lane.eng, 'sims_in_flight', 1) != 1:
                raise ValueError('this route has no device move step (sims_in_flight %d: one simulation in flight per tree only)' % lane.eng.sims_in_flight)
        kw = dict(self._attach_kw) if self._dev_on else {}
        kw.update(attach_kw)
        self._stream_before = (self._queue_ids.numel(), dict(self._attach_kw)) if self._dev_on else None
        self.device_attach(queue_capacity=queue_capacity, _ring=True, **kw)
        self._streaming = True
        self._stream_first, self._stream_pushed = first_game_id, 0
        self._stream_low, self._stream_done_ids = first_game_id, set()   # every id below _stream_low has been returned, and these above it
        self._stream_rounds = self._stream_batches = self._stream_returned = 0
        self._stream_topup = stream_topup(self.n_slots, self._copy_every, self._depth)
        self._chain_ev = None
        self.epochs = [self.settings(first_row=0)]
        for lane in self.lanes:   # (a host-driven run's last counts: the device's budgets rule here)
            with self._on(lane):
                lane.eng.set_playouts(None)
        self._stream_push()
        for lane in self.lanes:
            with self._on(lane):
                self._chain(lane)
                lane.eng.play_refill()
                self._chain_link(lane)
            lane.last_running = -1
        for _ in range(stream_lookahead(self._copy_every, self._depth)):
            self._stream_round()

    def _stream_push(self):
        """Top the ring up to stream_topup ids beyond the host's (lagged) count of started games: one launch on lane 0's stream, a
        link of the lanes' chain."""
        n = self._started + self._stream_topup - self._stream_pushed
        if n <= 0:
            return
        lane = self.lanes[0]
        with self._on(lane):
            self._chain(lane)
            lane.eng.play_queue_push(self._stream_first + self._stream_pushed, n)
            self._chain_link(lane)
        self._stream_pushed += n

    def _stream_round(self):
        """One more move of every lane, in the lanes' order; every copy_every rounds the read-back of their rows."""
        for lane in self.lanes:
            if getattr(lane.eng, 'play_match_on', False):
                raise ValueError('a lane\'s engine went into match mode (play_set_match) while a stream is open')
            if lane.move_graph is not None:
                with self._on(lane):
                    self._chain(lane)
                    lane.uncopied.append(lane.eng.play_move_replay(lane.move_graph))
                    self._chain_link(lane)
            else:   # (the search runs beside the other lanes' moves; only the move step joins the chain)
                self._simulate_lane(lane, host_counts=False)
                with self._on(lane):
                    self._chain(lane)
                    lane.uncopied.append(lane.eng.play_move())
                    self._chain_link(lane)
        self._stream_rounds += 1
        if self._stream_rounds % self._copy_every == 0:
            for lane in self.lanes:
                self._read_back(lane)

    def _stream_read(self, no_idle=True):
        """The oldest read-back of every lane, waited for -> the games that ended in its rows, by row, then game id."""
        ce = self._copy_every
        rounds = np.arange(self._stream_batches * ce, (self._stream_batches + 1) * ce)
        row_ep = np.searchsorted([e.first_row for e in self.epochs], rounds, side='right') - 1
        self._stream_batches += 1
        batches = []
        for lane in self.lanes:
            rows, ev = lane.inflight.pop(0)
            ev.synchronize()
            batches.append(rows)
        done = []
        # (host_np[rows] is a copy: the pinned rows may be overwritten from now on.)  Row by row, the games of a row by game id:
        # WHICH slot of a move step takes which id is a race among the step's waves (k_play_apply's CAS loop) -- the ids a step
        # takes, and so every game's content, are not
        for i in range(ce):
            ended = []
            for lane, rows in zip(self.lanes, batches):
                got, lane.last_running = self.read_rows(lane.host_np[rows[i:i + 1]], lane.slots.start,
                                                        values=None if lane.values_np is None else lane.values_np[rows[i:i + 1]],
                                                        row_epochs=row_ep[i:i + 1], no_idle=no_idle)
                ended.extend(got)
            done.extend(sorted(ended, key=lambda t: t.game_id))
        self._stream_returned += len(done)
        self._stream_done_ids.update(t.game_id for t in done)
        while self._stream_low in self._stream_done_ids:
            self._stream_done_ids.remove(self._stream_low)
            self._stream_low += 1
        return done

    def stream_collect(self, n_games, on_finished=None):
        """Enqueue moves until at least ``n_games`` more games have been read finished -> their Trajectories in finishing order (log
        row, then game id -- the slot a game sits in is not reproducible, see _stream_read), ``epochs`` filled in.  The other games stay in flight and are continued by the next call.
        ``on_finished(trajectories)``: as in run_device."""
        if not self._streaming:
            raise ValueError('stream_collect: no stream is open (stream_start)')
        out = []
        while len(out) < int(n_games):
            for _ in range(self._copy_every):
                self._stream_round()
            done = self._stream_read()
            self._stream_push()
            out.extend(done)
            if on_finished is not None and done:
                on_finished(done)
        return out

    def stream_running_ids(self):
        """The ids of the games the device has started and this stream has not returned yet, ascending (synchronises; what
        stream_stop(finish=True) would play to the end, or stream_stop() drop)."""
        if not self._streaming:
            raise ValueError('stream_running_ids: no stream is open (stream_start)')
        self.torch.cuda.synchronize(self.eng.device)
        head = int(self._queue_ctl.cpu()[0])
        return [g for g in range(self._stream_low, self._stream_first + head) if g not in self._stream_done_ids]

    def stream_stop(self, finish=False):
        """End the stream.  ``finish``: start no further game, play the running ones to their end -> their Trajectories, in finishing
        order.  Otherwise drop the running games -> how many were dropped.  Afterwards run / run_device work as before (an object
        that was attached before stream_start is attached again as it was)."""
        if not self._streaming:
            raise ValueError('stream_stop: no stream is open (stream_start)')
        t, dev = self.torch, self.eng.device
        out, head = [], self._stream_returned
        try:
            t.cuda.synchronize(dev)
            head = int(self._queue_ctl.cpu()[0])
            if finish:
                # the ids no slot has claimed are taken back (the device is idle: a plain copy), then rounds as before until a
                # read-back shows every slot idle and nothing is enqueued behind it
                self._queue_ctl.copy_(t.tensor([head, head], dtype=t.int32))
                t.cuda.synchronize(dev)
                while True:
                    while any(lane.inflight for lane in self.lanes):
                        out.extend(self._stream_read(no_idle=False))
                    if all(lane.last_running == 0 for lane in self.lanes):
                        break
                    for _ in range(self._copy_every):
                        self._stream_round()
                self.check()
                if self._stream_returned != head:
                    raise HipError('the stream started %d games and returned %d' % (head, self._stream_returned))
            else:
                self.check()
        finally:
            dropped = 0 if finish else head - self._stream_returned
            self._streaming, self.epochs = False, None
            self.device_stop()
            before, self._stream_before, self._dev_on = self._stream_before, None, False
            if before is not None:
                self.device_attach(queue_capacity=before[0], **before[1])
        return out if finish else dropped


# ------------------------------------------------------------------------- multi-GPU gather
def _resign_word(t):
    """Header word 3: bit 32 resigned, bit 33 calibration game, low 32 bits the float bits of a calibration game's fp_margin; 0 for
    every game played without resignation (the format of a run without it is unchanged)."""
    no_resign = bool(getattr(t, 'no_resign', False))
    low = int(np.float32(t.fp_margin).view(np.uint32)) if no_resign else 0
    word = (int(bool(getattr(t, 'resigned', False))) << 32) | (int(no_resign) << 33) | low
    full = getattr(t, 'full', None)
    if full is not None:
        # the playout cap: bit 34 the game was played under one (its plies' budget flags travel as bit 32 of the move words: _move_words),
        # bit 35 the flag of a resigned game's last search, which has no move
        word |= 1 << 34
        if len(full) > len(t.moves) and full[len(t.moves)]:
            word |= 1 << 35
    return word


def _move_words(t):
    """A game's moves as int64 words; under a playout cap bit 32 of a word says that the ply's search had the full budget (without
    one the words are the moves: the format of a run without a cap is unchanged)."""
    moves = np.asarray(t.moves, dtype=np.int64).reshape(-1)
    full = getattr(t, 'full', None)
    if full is None:
        return moves
    return moves | (np.asarray(full[:len(moves)], dtype=np.int64) << 32)


def _resign_fields(word):
    word = int(word)
    no_resign = bool((word >> 33) & 1)
    margin = np.uint32(word & 0xFFFFFFFF).view(np.float32) if no_resign else np.float32(np.nan)
    return dict(resigned=bool((word >> 32) & 1), no_resign=no_resign, fp_margin=margin)


def _full_field(word, move_words):
    """-> (moves, Trajectory.full or None) from the header word and the move words of one game (_resign_word, _move_words)."""
    word, move_words = int(word), np.asarray(move_words, dtype=np.int64)
    if not (word >> 34) & 1:
        return move_words, None
    full = ((move_words >> 32) & 1).astype(bool)
    if (word >> 32) & 1:   # (a resigned game: the flag of the search that resigned)
        full = np.append(full, bool((word >> 35) & 1))
    return move_words & 0xFFFFFFFF, full


def pack_trajectories(trajs, n_cells):
    """-> (header int64 [n,4] = game id, plies, winner, resignation word (_resign_word) ; moves int64 [P] ; pis float64 [P,S])."""
    header = np.array([[t.game_id, len(t.moves), t.winner, _resign_word(t)] for t in trajs], dtype=np.int64).reshape(-1, 4)
    moves = np.concatenate([_move_words(t) for t in trajs]) if trajs else np.zeros(0, dtype=np.int64)
    pis = np.concatenate([t.pis for t in trajs], axis=0) if trajs else np.zeros((0, n_cells))
    return header, moves, pis.reshape(-1, n_cells)


def unpack_trajectories(header, moves, pis, board_size, n_in_row, game='gomoku'):
    out, at = [], 0
    for gid, plies, winner, word in header:
        plies = int(plies)
        mv, full = _full_field(word, moves[at:at + plies])
        out.append(Trajectory(gid, board_size, n_in_row, mv, pis[at:at + plies], winner,
                              game=game, full=full, **_resign_fields(word)))
        at += plies
    return out


COLLECTIVES_PER_EXCHANGE = 2   # gather_trajectories: one all_gather of a 3-word size row + ONE gather of the byte payload


def _payload_bytes(header, moves, pis, pi_dtype):
    """One contiguous record of a rank's finished games: header int64 [n, 4] | moves int64 [P] | pi [P, A] (float32 or
    float64) -- fixed strides, so (n, P) from the size row are all the receiver needs to cut it up again."""
    return np.concatenate([np.ascontiguousarray(header, dtype=np.int64).reshape(-1).view(np.uint8),
                           np.ascontiguousarray(moves, dtype=np.int64).view(np.uint8),
                           np.ascontiguousarray(pis, dtype=pi_dtype).reshape(-1).view(np.uint8)])


def payload_of(trajs, n_cells, pi_dtype):
    """_payload_bytes(*pack_trajectories(trajs), pi_dtype) in ONE pass: every game's pi is converted straight into its place in the
    buffer (a collection round's pi is 100+ MB per rank: packing it through three intermediate copies cost more than sending it).
    -> (bytes uint8, games, plies)."""
    n_games, n_plies = len(trajs), sum(len(t.moves) for t in trajs)
    item = np.dtype(pi_dtype).itemsize
    raw = np.empty(n_games * 32 + n_plies * (8 + n_cells * item), dtype=np.uint8)
    header = raw[:n_games * 32].view(np.int64).reshape(n_games, 4)
    moves = raw[n_games * 32:n_games * 32 + 8 * n_plies].view(np.int64)
    pis = raw[n_games * 32 + 8 * n_plies:].view(pi_dtype).reshape(n_plies, n_cells)
    at = 0
    for i, t in enumerate(trajs):
        k = len(t.moves)
        header[i] = (t.game_id, k, t.winner, _resign_word(t))
        moves[at:at + k] = _move_words(t)
        if k:
            pis[at:at + k] = t.pis   # (numpy converts while it copies)
        at += k
    return raw, n_games, n_plies


def _payload_split(raw, n_games, n_plies, n_cells, pi_dtype):
    """-> header, moves, pi as VIEWS of the received bytes (float32 pi stays float32: Trajectory keeps it)."""
    at = n_games * 32
    header = raw[:at].view(np.int64).reshape(n_games, 4)
    moves = raw[at:at + 8 * n_plies].view(np.int64)
    at += 8 * n_plies
    pis = raw[at:at + n_plies * n_cells * np.dtype(pi_dtype).itemsize].view(pi_dtype).reshape(n_plies, n_cells)
    return header, moves, pis


def gather_trajectories(trajs, board_size, n_in_row, dst=0, group=None, game='gomoku', pi_dtype=np.float64):
    """The one exchange of the path: every rank sends its finished trajectories to ``dst``.  Two collectives
    (COLLECTIVES_PER_EXCHANGE): an all_gather of one 3-word row per rank (games, plies, error bit) and ONE gather of a byte
    payload -- header, moves and pi of all the rank's games in one buffer, padded to the longest rank's.  Returns the merged,
    game-id-sorted list on ``dst`` and None elsewhere.  Without an initialised process group: identity.
    ``pi_dtype``: what pi travels as -- float64 (default: bit-identical to the single-process run) or float32 (what the
    learner consumes, alphazero_agent.py:59-61: half the bytes, the exchange SURVEY.md 8e sizes; the trainer's choice).

    What can fail locally -- packing, the device copy of the rank's own payload -- happens BEFORE the size row is exchanged
    and travels in it as the error bit: a rank that failed still takes part in that all_gather and then ALL ranks raise, so
    no peer is left blocked in the gather.  (Behind the size row only the padding of the send buffer and the receive buffers
    of ``dst`` are allocated; running out of memory there is an out-of-memory inside a collective, fatal to the job.)"""
    import torch
    import torch.distributed as dist
    n_cells = board_size[1] if game == 'connect4' else board_size * board_size  # width of a pi row
    if not (dist.is_available() and dist.is_initialized()):
        return sorted(trajs, key=lambda t: t.game_id)
    rank, world = dist.get_rank(group), dist.get_world_size(group)  # a group of one runs the same collectives
    on_gpu = dist.get_backend(group) == 'nccl'
    device = torch.device('cuda', torch.cuda.current_device()) if on_gpu else torch.device('cpu')
    pi_dtype = np.dtype(pi_dtype).type
    local_error, mine, n_games, n_plies = None, None, 0, 0
    try:
        payload, n_games, n_plies = payload_of(trajs, n_cells, pi_dtype)
        mine = torch.from_numpy(payload).to(device)
    except Exception as exc:  # noqa: BLE001
        local_error, mine, n_games, n_plies = exc, None, 0, 0
    sizes = torch.tensor([n_games, n_plies, 0 if local_error is None else 1], dtype=torch.int64, device=device)
    all_sizes = [torch.zeros_like(sizes) for _ in range(world)]
    dist.all_gather(all_sizes, sizes, group=group)                                   # collective 1 of 2
    all_sizes = torch.stack(all_sizes).cpu().numpy()
    if all_sizes[:, 2].any():
        raise RuntimeError('gather_trajectories: packing failed on rank(s) %s%s' % (
            np.nonzero(all_sizes[:, 2])[0].tolist(), '' if local_error is None else ' (here: %r)' % (local_error, )))
    row_bytes = 8 + n_cells * np.dtype(pi_dtype).itemsize
    n_bytes = all_sizes[:, 0] * 32 + all_sizes[:, 1] * row_bytes
    send = torch.empty(max(int(n_bytes.max()), 1), dtype=torch.uint8, device=device)   # (padded to the longest rank's; the padding is never read)
    send[:mine.numel()] = mine
    bucket = [torch.empty_like(send) for _ in range(world)] if rank == dst else None
    dist.gather(send, gather_list=bucket, dst=dst, group=group)                      # collective 2 of 2
    if rank != dst:
        return None
    merged = []
    for r in range(world):
        raw = bucket[r][:int(n_bytes[r])].cpu().numpy()
        merged.extend(unpack_trajectories(*_payload_split(raw, int(all_sizes[r, 0]), int(all_sizes[r, 1]), n_cells, pi_dtype),
                                          board_size, n_in_row, game=game))
    return sorted(merged, key=lambda t: t.game_id)


def broadcast_weights(module, src=0, group=None):
    """After ``policy_update`` on rank ``src``: one broadcast of the flattened parameters
    (1.3 MB at 15x15) so every rank's self-play uses the same network.  RCCL when the process
    group backend is nccl; identity without a process group."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return module
    params = list(module.parameters())
    with torch.no_grad():
        flat = torch.cat([p.detach().reshape(-1) for p in params])
        if dist.get_backend(group) == 'nccl' and not flat.is_cuda:
            flat = flat.cuda()
        dist.broadcast(flat, src=src, group=group)
        at = 0
        for p in params:
            n = p.numel()
            # copy_ on the Parameter ITSELF (not on p.data, which carries a version counter of its own): the in-place write bumps
            # p._version, which is what HipNetEvaluator.refresh_if_changed() looks at -- a rank that only receives weights must
            # re-upload them like the rank whose optimiser stepped
            p.copy_(flat[at:at + n].reshape(p.shape).to(p.device))
            at += n
    return module
