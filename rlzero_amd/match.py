"""Network against network: matches from paired openings, played on the device's move step.

Batched counterpart of ``GameControl.start_play(player1, player2)`` (rlzero/games/gomoku/game.py:61-94) with two
``AlphaZeroPlayer(is_selfplay=False)`` (rlzero/mcts/alphazero_mcts.py:136-165), each holding a network of its own: per move
n_playout simulations from a FRESH root without noise, pi = softmax(log(N + 1e-10) / T) with T = 1e-3, two draws from pi of
which the second is played (:148,157), root reset (:158) -- what ``evaluate.BatchedEvaluation`` gives its network player.

Three things make the score of a match mean something:

* paired openings: games 2k and 2k + 1 start from opening k % n_openings of a table of legal, non-terminal positions with player 0
  to move; network A is player 0 in the even game and player 1 in the odd one, so first-move advantage and opening luck -- both
  large on Gomoku -- cancel within a pair;
* common random numbers: the draw of ply ``ply`` (counted from the opening) of a game uses move_uniform(seed, game id >> 1,
  2 ply + 1), shared by the two games of a pair: a network against itself plays every pair as the same game twice and scores
  exactly one half;
* the score: wins + ties / 2 per network, by seat and overall, the outcomes of the pairs, and an Elo difference from the score.

One engine holds every game.  A move is enqueued on one stream without a host round trip (include/rlzero_hip.h: rz_play_set_match):
play_side(A), the resident search with A's evaluator, play_side(B), the search with B's, the draw, the flush of the pending priors,
the game step.  Each evaluator keeps its own receptive-field bases and its own store of pending leaves; the engine flushes one
evaluator's before the other searches.  The host reads the log behind the GPU as ``BatchedSelfPlay.run_device`` does: its numpy
expression on the logged visit counts is the arbiter, every move the device drew is verified against it, and a draw too close to an
interval edge stalls until the move decided here has been handed back (play_resolve).  A match's moves are not captured into a
whole-move hipGraph (two evaluators, two searches): they are enqueued eagerly.
"""
import math

import numpy as np

from . import playlog
from ._hip import HipError
from .selfplay import batch_pi_and_moves, move_uniform

NET_A, NET_B = 0, 1


# ------------------------------------------------------------------------- pair and seat arithmetic
def pair_of(game_id):
    return np.asarray(game_id, dtype=np.int64) >> 1


def opening_of(game_id, n_openings):
    """Index of the opening game ``game_id`` starts from: the pair's, k % n_openings."""
    return pair_of(game_id) % int(n_openings)


def seat_of(game_id, net):
    """The player id (0 moves first from the opening) network ``net`` (NET_A / NET_B) has in game ``game_id``."""
    return (np.asarray(game_id, dtype=np.int64) & 1) ^ int(net)


def net_to_move(game_id, to_move):
    """The network whose turn it is: A iff (player 0 to move) == (even game id) -- the device's rule (k_play_side)."""
    a = (np.asarray(to_move) == 0) == ((np.asarray(game_id, dtype=np.int64) & 1) == 0)
    return np.where(a, NET_A, NET_B)


def match_uniform(seed, game_id, ply):
    """The uniform of the draw that is played at ``ply`` plies after the opening: the pair's, and the second of get_action's two."""
    return move_uniform(seed, pair_of(game_id), 2 * np.asarray(ply, dtype=np.int64) + 1)


# ------------------------------------------------------------------------- openings
def _env(board, n_in_row, moves=()):
    from .games.gomoku.gomoku_env import GomokuEnv
    env = GomokuEnv(int(board), int(n_in_row))
    env.reset()
    for m in moves:
        env.step(int(m))
    return env


def paired_openings(board, n_in_row, n, plies, seed, game='gomoku'):
    """``n`` distinct legal, non-terminal positions after ``plies`` uniformly random moves from the empty board, as move lists
    (position = stones, side to move and last move: two orders of the same stones with the same last move are one opening).
    ``plies`` is even, so player 0 is to move in every one; reproducible from ``seed``."""
    if game != 'gomoku':
        raise ValueError('paired_openings: Gomoku boards only (game=%r)' % (game, ))
    if plies < 0 or plies % 2:
        raise ValueError('paired_openings: an even number of plies (player 0 to move), not %r' % (plies, ))
    rs = np.random.RandomState(int(seed) & 0x7FFFFFFF)
    out, seen, tries = [], set(), 0
    while len(out) < n:
        tries += 1
        if tries > 1000 * max(int(n), 1):
            raise ValueError('paired_openings: fewer than %d distinct non-terminal positions of %d plies on this board' % (n, plies))
        env, moves = _env(board, n_in_row), []
        for _ in range(plies):
            legal = env.leagel_actions()
            if env.game_end_winner()[0] or not legal:
                break
            moves.append(int(legal[rs.randint(len(legal))]))
            env.step(moves[-1])
        key = env.bitboards() + (env.last_move, )
        if len(moves) != plies or env.game_end_winner()[0] or key in seen:
            continue
        assert env.current_player() == 0
        seen.add(key)
        out.append(moves)
    return out


def opening_arrays(openings, board, n_in_row):
    """Move lists -> (stones uint64 [n, 2, WORDS], to_move int32 [n], last_move int32 [n]): what MCTSEngine.play_set_match and
    set_roots take.  Every opening must be legal, non-terminal and have player 0 to move."""
    from .engine import WORDS, int_to_bits
    n = len(openings)
    stones, to_move, last = np.zeros((n, 2, WORDS), np.uint64), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    for i, moves in enumerate(openings):
        env = _env(board, n_in_row, moves)   # (an illegal move fails the environment's assertion)
        if env.game_end_winner()[0] or env.current_player() != 0:
            raise ValueError('opening %d (%r) is terminal or has player 1 to move' % (i, list(moves)))
        b0, b1 = env.bitboards()
        stones[i, 0], stones[i, 1] = int_to_bits(b0), int_to_bits(b1)
        to_move[i], last[i] = env.current_player(), env.last_move
    return stones, to_move, last


def load_checkpoint(path, board, device='cuda:0'):
    """A PolicyValueNet of a ``board`` x ``board`` game from a checkpoint: the directory ``AlphaZeroAgent.save_model`` writes (its
    ``model.th``) or a file holding the state_dict."""
    import os

    import torch

    from .games.gomoku.policy_value_net import PolicyValueNet
    if os.path.isdir(path):
        path = os.path.join(path, 'model.th')
    net = PolicyValueNet(int(board))
    net.load_state_dict(torch.load(path, map_location='cpu'))
    return net.to(device)


# ------------------------------------------------------------------------- results and score
class MatchResult(object):
    """One finished game of a match: the opening (index and moves), the moves played after it, the winner's player id (0 moves first
    from the opening, -1 = tie), the seats, and per ply the visit counts the move was drawn from (int32 [A], -1 = illegal) and
    N(root) of the search behind them."""

    def __init__(self, game_id, opening, opening_moves, moves, winner, visits, root_n=None):
        self.root_n = [int(n) for n in root_n] if root_n is not None else None
        self.game_id, self.opening, self.opening_moves = int(game_id), int(opening), [int(m) for m in opening_moves]
        self.moves, self.winner, self.visits = [int(m) for m in moves], int(winner), list(visits)
        self.pair = self.game_id >> 1
        self.seat_a, self.seat_b = int(seat_of(game_id, NET_A)), int(seat_of(game_id, NET_B))

    @property
    def points_a(self):
        """Network A's points: 1 win, 0.5 tie, 0 loss."""
        return 0.5 if self.winner < 0 else (1.0 if self.winner == self.seat_a else 0.0)


def elo_from_score(score, n_games):
    """Elo difference (A - B) of the logistic model for a score fraction, the fraction clipped to [1 / 2n, 1 - 1 / 2n] -- half a
    point away from all losses / all wins -- so that a shut-out is a large finite number.  -> (elo, clipped)."""
    lo = 0.5 / max(int(n_games), 1)
    p = min(max(float(score), lo), 1.0 - lo)
    return -400.0 * math.log10(1.0 / p - 1.0), p != float(score)


def score(results):
    """Summary of a match from network A's side: games, wins / losses / ties, the score fraction overall and by seat, the outcomes of
    the complete pairs (A's points - B's points: '2-0', '1.5-0.5', '1-1' for a win and a loss, 'tie-tie', '0.5-1.5', '0-2') and the Elo
    estimate."""
    results = list(results)
    n = len(results)
    pts = np.array([r.points_a for r in results], dtype=np.float64)
    seat = np.array([r.seat_a for r in results], dtype=np.int64)
    out = {'games': n, 'a_wins': int((pts == 1.0).sum()), 'b_wins': int((pts == 0.0).sum()), 'ties': int((pts == 0.5).sum()),
           'a_points': float(pts.sum()), 'a_score': float(pts.mean()) if n else float('nan')}
    for s, name in ((0, 'a_score_moving_first'), (1, 'a_score_moving_second')):
        out[name] = float(pts[seat == s].mean()) if (seat == s).any() else float('nan')
    by_pair = {}
    for r in results:
        by_pair.setdefault(r.pair, {})[r.game_id & 1] = r.points_a
    pairs = {'2-0': 0, '1.5-0.5': 0, '1-1': 0, 'tie-tie': 0, '0.5-1.5': 0, '0-2': 0}
    for both in by_pair.values():
        if len(both) != 2:
            continue
        total = both[0] + both[1]
        key = {2.0: '2-0', 1.5: '1.5-0.5', 0.5: '0.5-1.5', 0.0: '0-2'}.get(total)
        if key is None:
            key = 'tie-tie' if both[0] == 0.5 else '1-1'
        pairs[key] += 1
    out['pairs'] = pairs
    out['elo_diff'], out['elo_clipped'] = elo_from_score(out['a_score'], n) if n else (float('nan'), False)
    return out


# ------------------------------------------------------------------------- the match
class MatchReader(object):
    """What turns the log of a match's move step into MatchResults: seed and temperature, the counters and the book of the slots
    (playlog.SlotBook).  numpy only -- BatchedMatch adds the engine; a test builds one alone.  ``resolve(slot, move)`` hands a stalled
    slot's move back to the device."""

    def __init__(self, n_slots, n_actions, max_plies, n_playout, resolve, seed=0, temperature=1e-3):
        self.seed, self.temperature, self.n_playout = int(seed), float(temperature), n_playout
        self._book_args = (n_slots, max_plies, resolve, dict(visits=(np.int32, (n_actions, ), 'move'),
                                                             root_n=(np.int32, (), 'move')))
        self.start_reading(())

    stalls_resolved, moves_done, _started = playlog.counter('stalls_resolved'), playlog.counter('moves_done'), playlog.counter('started')

    def start_reading(self, openings):
        """A new match from ``openings`` (move lists): every slot idle, every counter zero."""
        self.openings = [list(o) for o in openings]
        self.book = playlog.SlotBook(*self._book_args)
        self.sims_done, self._last_running = 0, -1

    def read_rows(self, rows):
        """Log rows int32 [R, G, words], oldest first -> (the games that ended in them, the RUNNING records of the last row)."""
        slots, d, last_running = playlog.running(rows)
        if slots.size == 0:
            return [], last_running
        # the reference's expression on the logged counts, the draw with the pair's uniform (numpy's inverse-CDF rule): the arbiter
        _, chosen = batch_pi_and_moves(d.counts, d.legal, self.temperature, match_uniform(self.seed, d.game, d.ply))
        playlog.check_moves(d, chosen)
        self.sims_done += self.n_playout * playlog.check_match_roots(d, self.n_playout)
        done = []
        for f in self.book.feed(slots, d, chosen, dict(visits=d.visits, root_n=d.root_n)):
            k = int(opening_of(f.game, len(self.openings)))
            done.append(MatchResult(f.game, k, self.openings[k], f.moves, f.winner, f.columns['visits'], f.columns['root_n']))
        return done, last_running


class BatchedMatch(MatchReader):
    """A match between ``evaluator_a`` and ``evaluator_b`` in the slots of ONE engine (one lane); see the module docstring."""

    def __init__(self, engine, evaluator_a, evaluator_b, seed=0, temperature=1e-3, stall_margin=0.0, ring_steps=64, depth=2):
        self.eng, self.evaluators = engine, (evaluator_a, evaluator_b)
        MatchReader.__init__(self, engine.n_games, engine.n_actions, engine.n_cells, engine.n_playout, self._resolve, seed, temperature)
        self.stall_margin, self.ring_steps, self.depth = float(stall_margin), max(int(ring_steps), int(depth) + 3), int(depth)
        if engine.game != 'gomoku':
            raise ValueError('matches are played on Gomoku boards')
        for ev in self.evaluators:
            if not engine._ask(ev)[0].resident:
                raise ValueError('a match needs the resident search: this evaluator\'s route for this engine has none')
        self.torch = engine.torch
        # one lane: the stream current at construction, as a one-lane BatchedSelfPlay does (no stream of its own: a process's lanes
        # elsewhere keep the hardware queues they would have had)
        self.stream = self.torch.cuda.current_stream(engine.device)

    @classmethod
    def for_networks(cls, net_a, net_b, board, n_in_row, n_games, n_playout, c_puct=5.0, device='cuda:0', seed=0, temperature=1e-3,
                     net_shape=None, stall_margin=0.0, **engine_kw):
        """One engine of ``n_games`` slots and the hand-written evaluators of two PolicyValueNets."""
        from .engine import HipNetEvaluator, MCTSEngine
        eng = MCTSEngine(board, n_in_row, n_games=n_games, n_playout=n_playout, c_puct=c_puct, device=str(device), add_noise=False,
                         **engine_kw)
        shape = net_shape if net_shape is not None else board
        evs = [HipNetEvaluator(net, shape, str(device), max_boards=n_games) for net in (net_a, net_b)]
        return cls(eng, evs[0], evs[1], seed=seed, temperature=temperature, stall_margin=stall_margin)

    def refresh_weights(self):
        for ev in self.evaluators:
            refresh = getattr(ev, 'refresh_if_changed', None)
            if refresh is not None:
                refresh(content=True)

    def close(self):
        self.eng.close()
        for ev in self.evaluators:
            hip = getattr(ev, 'hip', None)
            if hip is not None:
                hip.close()

    # -- one move ------------------------------------------------------------------------------------------------------
    def enqueue_move(self):
        """One move of every running game on the match's stream -> the log row it writes."""
        eng = self.eng
        with self.torch.cuda.stream(self.stream):
            for side in (NET_A, NET_B):
                eng.play_side(side)
                eng.simulate(self.evaluators[side], eng.n_playout)
            return eng.play_move()

    def begin(self, n_pairs, openings):
        """Attach the move step, turn match mode on and queue the games of pairs 0 .. n_pairs - 1: the slots take the first of them."""
        t, eng = self.torch, self.eng
        self.start_reading(openings)
        arrays = opening_arrays(self.openings, eng.board_size, eng.n_in_row)
        ids = np.arange(2 * int(n_pairs), dtype=np.int64)
        with t.cuda.stream(self.stream):
            self._queue = (t.from_numpy(ids).to(eng.device) if ids.size else t.zeros(1, dtype=t.int64, device=eng.device),
                           t.tensor([0, ids.size], dtype=t.int32, device=eng.device))
            self.log = eng.play_attach(self.seed, self.temperature, self._queue[0], self._queue[1], ring_steps=self.ring_steps,
                                       stall_margin=self.stall_margin)
            eng.set_playouts(None)
            eng.play_set_match(arrays)
            eng.play_refill()
        if not eng.play_log_on_host:
            raise HipError('a match reads its log in place: the engine\'s log ring must be host memory the device can address')
        self._log_np = self.log.numpy()
        self._inflight, self._n_games = [], int(ids.size)

    def step(self):
        """Enqueue one move and process the log rows that have arrived (all but the ``depth`` newest) -> the games found finished."""
        row = self.enqueue_move()
        ev = self.torch.cuda.Event()
        ev.record(self.stream)
        self._inflight.append((row, ev))
        return self._harvest(self.depth)

    def _harvest(self, keep):
        done = []
        while self._inflight and (len(self._inflight) > keep or self._inflight[0][1].query()):
            row, ev = self._inflight.pop(0)
            ev.synchronize()
            done.extend(self.read_row(row))
        return done

    def read_row(self, row):
        """Process log row ``row`` (its move has finished on the device) -> the games that ended in it."""
        done, self._last_running = self.read_rows(self._log_np[[row]])   # (a copy: the pinned row may be overwritten from now on)
        return done

    def _resolve(self, slot, move):
        with self.torch.cuda.stream(self.stream):
            self.eng.play_resolve(slot, move)

    def run(self, n_pairs, openings):
        """Play pairs 0 .. n_pairs - 1 (game ids 0 .. 2 n_pairs - 1) from ``openings`` (move lists: paired_openings) to the end
        -> [MatchResult] sorted by game id."""
        self.begin(n_pairs, openings)
        out, eng = [], self.eng
        # (a game has at most n_cells plies, a slot plays its share of the games one after the other; stalls wait `depth` moves)
        limit = (-(-self._n_games // eng.n_games) + 1) * (eng.n_cells + 2) * (self.depth + 2) + 16
        while len(out) < self._n_games:
            limit -= 1
            if limit < 0:
                raise RuntimeError('the match did not finish: %d of %d games after the moves they can take' % (len(out), self._n_games))
            if not self._inflight and self._last_running == 0 and self._started >= self._n_games:
                raise RuntimeError('the match went quiet with %d of %d games finished' % (len(out), self._n_games))
            out.extend(self.step())
        out.extend(self._harvest(0))
        with self.torch.cuda.stream(self.stream):
            self.eng.play_stop()
        self.stream.synchronize()
        self.eng.check()
        for ev in self.evaluators:
            if hasattr(getattr(ev, 'hip', None), 'check_flags'):
                ev.hip.check_flags()
        return sorted(out, key=lambda r: r.game_id)

    score = staticmethod(score)
