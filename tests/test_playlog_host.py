"""The host's reader of the device move step's log (rlzero_amd/playlog.py and its two owners, selfplay.SelfPlayReader and
match.MatchReader) without a GPU: a scripted writer models the device side as include/rlzero_hip.h describes it ("The log: ..."), and
what the readers return is held against the script and against the reference's expressions formed here -- never against the code
under test.  3 x 3 boards (A = 9), 2 slots, 5 queued games, so every slot refills; one case with Connect4's shape (A = 7, 42 plies)."""
import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
from oracle.mcts_ref import inverse_cdf_choice, softmax
from rlzero_amd import playlog
from rlzero_amd._hip import (PLAY_ENDED, PLAY_FULL, PLAY_NO_RESIGN, PLAY_RECORD_WORDS, PLAY_RESIGNED, PLAY_RESOLVED, PLAY_RUNNING,
                             PLAY_SEARCHED, PLAY_STALLED, PLAY_WOULD_RESIGN, HipError)
from rlzero_amd.match import MatchReader, match_uniform
from rlzero_amd.selfplay import SelfPlayReader, cap_uniform, move_uniform, resign_uniform

SEED, N_PLAYOUT, W0 = 11, 40, PLAY_RECORD_WORDS
THRESHOLD, FRAC = -0.8, 0.3
CALIB = [g for g in range(200) if resign_uniform(SEED, g) < FRAC]        # calibration games under (SEED, FRAC)
PLAYED = [g for g in range(200) if resign_uniform(SEED, g) >= FRAC]      # games that may resign


def _bits(x):
    return int(np.float32(x).view(np.int32))


class Cfg(object):
    """The settings of one log: what the device was told, and what the reader is told."""

    def __init__(self, A=9, room=9, temps=1.0, pi_T=None, resign=None, cap=None, match=False, geometry=(3, 3, 'gomoku')):
        self.A, self.room, self.temps, self.pi_T, self.resign, self.cap, self.match, self.geometry = A, room, temps, pi_T, resign, cap, match, geometry
        self.T0 = 1e-3 if match else 1.0

    def T(self, ply):
        return self.T0 if np.ndim(self.temps) == 0 else float(self.temps[min(ply, len(self.temps) - 1)])

    def u(self, gid, ply):
        return float((match_uniform if self.match else move_uniform)(SEED, gid, ply))

    def reader(self, resolve, n_slots=2):
        if self.match:
            r = MatchReader(n_slots, self.A, self.room, N_PLAYOUT, resolve, seed=SEED, temperature=self.T0)
            r.start_reading(OPENINGS)
            return r
        r = SelfPlayReader(n_slots, self.A, self.room, N_PLAYOUT, self.geometry, resolve, temperature=self.T0, seed=SEED)
        r.playout_cap = self.cap
        if self.resign is not None:
            r.resign_threshold, r.resign_disabled_frac = self.resign
        if np.ndim(self.temps):
            r.temperature_schedule = np.asarray(self.temps, dtype=np.float64)
        r.pi_temperature = self.pi_T
        return r


OPENINGS = [[0, 1], [4, 2], [8, 3]]


class Game(object):
    """One scripted game: per search the visit counts (-1: illegal), the statistic and the budget; per ply the expected move and pi."""

    def __init__(self, cfg, rng, gid, n_plies, winner, stalls=(), resign=False, would_at=None, peaked=False):
        self.gid, self.winner, self.stalls, self.resigned = gid, winner, set(stalls), resign
        self.calib = cfg.resign is not None and gid in CALIB
        assert not (resign and self.calib) and (would_at is None or self.calib)
        self.counts, self.moves, self.pis, self.stats, self.full, self.would = [], [], [], [], [], []
        taken = np.zeros(cfg.A, dtype=bool)
        for ply in range(n_plies + (1 if resign else 0)):
            legal = np.nonzero(~taken)[0]
            n = np.zeros(len(legal), dtype=np.int64)
            if peaked:   # (one visited child: the draw is that child whatever the uniform)
                n[rng.randint(len(legal))] = N_PLAYOUT - 1
            else:
                n[:] = rng.multinomial(N_PLAYOUT - 1, rng.dirichlet(np.ones(len(legal))))
            counts = np.full(cfg.A, -1, dtype=np.int32)
            counts[legal] = n
            self.counts.append(counts)
            resigning = resign and ply == n_plies
            self.would.append(ply == would_at)
            if cfg.resign is None:
                self.stats.append(np.float32(-5.0))          # (resignation off: word 7 is not read)
            else:
                self.stats.append(np.float32(-0.9 if resigning else -0.95 if ply == would_at else rng.uniform(-0.5, 0.5)))
            self.full.append(True if cfg.cap is None else bool(cap_uniform(SEED, gid, ply) < cfg.cap[1]))
            if resigning:
                self.winner = 1 - ply % 2
                break
            # the reference's expressions (alphazero_mcts.py:10-14,91-92,148) on the scripted counts
            x = np.log(n + 1e-10)
            probs = softmax(1.0 / cfg.T(ply) * x)
            self.moves.append(inverse_cdf_choice([cfg.u(gid, ply)])(legal, probs))
            pi = np.zeros(cfg.A)
            pi[legal] = probs if cfg.pi_T is None else softmax(1.0 / cfg.pi_T * x)
            self.pis.append(pi)
            if cfg.A == 9:   # (Connect4's shape: a column stays legal)
                taken[self.moves[-1]] = True
        self.sims = sum(N_PLAYOUT if f else cfg.cap[0] for f in self.full) if cfg.cap is not None else N_PLAYOUT * len(self.full)


class Writer(object):
    """The device side: ``G`` slots that take the queued games in turn and write one row [G, 8 + A] per move step.  A stalled slot
    repeats STALLED until the move handed to ``resolve`` has waited ``delay`` rows; the RESOLVED record then carries counts that
    mean nothing (the position after the move)."""

    def __init__(self, cfg, games, G, delay=1):
        self.cfg, self.queue, self.G, self.delay = cfg, list(games), G, delay
        self.slot = [None] * G            # [game, ply, stalled]
        self.mail = [None] * G            # [move, rows to wait]
        self.stale = np.zeros((G, W0 + cfg.A), dtype=np.int32)
        self.rows, self.calls = [], []
        self.junk = np.random.RandomState(99)

    def resolve(self, slot, move):
        assert self.slot[slot] is not None and self.slot[slot][2] and self.mail[slot] is None
        self.calls.append((slot, move))
        self.mail[slot] = [move, self.delay]

    def busy(self):
        return bool(self.queue) or any(s is not None for s in self.slot)

    def step(self):
        row = self.stale.copy()
        row[:, 4] = 0                     # (an idle slot: flags 0, the rest is its last game's)
        for s in range(self.G):
            if self.slot[s] is None and self.queue:
                self.slot[s] = [self.queue.pop(0), 0, False]
            if self.slot[s] is None:
                continue
            game, ply, stalled = self.slot[s]
            rec = row[s]
            rec[0:2], rec[2] = np.array([game.gid], dtype=np.int64).view(np.int32), ply
            rec[3], rec[6], rec[7] = -1, 0, 0
            rec[5] = N_PLAYOUT if self.cfg.match else int(np.maximum(game.counts[ply], 0).sum()) + 1
            rec[W0:] = game.counts[ply]
            flags, played = PLAY_RUNNING, None
            if not stalled:
                flags |= PLAY_SEARCHED
                rec[7] = _bits(game.stats[ply]) if not self.cfg.match else 0
                if self.cfg.resign is not None:
                    flags |= (PLAY_NO_RESIGN if game.calib else 0) | (PLAY_WOULD_RESIGN if game.would[ply] else 0)
                if self.cfg.cap is not None and game.full[ply]:
                    flags |= PLAY_FULL
                if game.resigned and ply == len(game.moves):
                    flags |= PLAY_RESIGNED | PLAY_ENDED
                    rec[4] = flags | ((game.winner + 1) << 16)
                    self.slot[s] = None
                    continue
                if ply in game.stalls:
                    flags |= PLAY_STALLED
                    self.slot[s][2] = True
                else:
                    played = game.moves[ply]
                    rec[6] = _bits(0.25)
            elif self.mail[s] is not None and self.mail[s][1] <= 0:
                flags |= PLAY_RESOLVED
                played, self.mail[s] = self.mail[s][0], None
                legal = game.counts[ply] >= 0
                rec[W0:] = np.where(legal, self.junk.randint(0, N_PLAYOUT, size=legal.size), -1)
            else:
                flags |= PLAY_STALLED
                if self.mail[s] is not None:
                    self.mail[s][1] -= 1
            if played is not None:
                rec[3] = played
                self.slot[s] = [game, ply + 1, False]
                if ply + 1 == len(game.moves) and not game.resigned:
                    flags |= PLAY_ENDED | ((game.winner + 1) << 16)
                    self.slot[s] = None
            rec[4] = flags
        self.stale = row
        self.rows.append(row)
        return row


def record(cfg, games, G=2, delay=1):
    """Write the log of ``games`` with a reader reading row by row (a stall needs its answer) -> (log [R, G, words], what the reader
    returned, the reader, the resolve calls)."""
    w = Writer(cfg, games, G, delay)
    reader = cfg.reader(w.resolve, G)
    out = []
    while w.busy():
        done, last = reader.read_rows(w.step()[None])
        out.extend(done)
    done, last = reader.read_rows(w.step()[None])   # (a row of idle slots)
    assert done == [] and last == 0
    return np.stack(w.rows), out, reader, w.calls


def replay(cfg, log, batches=None, G=2):
    """Read a recorded log again, ``batches`` rows per call (None: all at once) -> (games, reader, resolve calls)."""
    calls = []
    reader = cfg.reader(lambda s, m: calls.append((s, m)), G)
    sizes = list(batches) if batches is not None else [len(log)]
    out, at, k = [], 0, 0
    while at < len(log):
        n = sizes[k % len(sizes)]
        k += 1
        out.extend(reader.read_rows(log[at:at + n])[0])
        at += n
    return out, reader, calls


def counters(r):
    return dict((k, getattr(r, k)) for k in ('sims_done', 'moves_done', 'stalls_resolved', '_started') +
                (() if isinstance(r, MatchReader) else ('full_plies', 'resign_would')))


def want_counters(cfg, games):
    want = dict(sims_done=sum(g.sims for g in games), moves_done=sum(len(g.moves) for g in games),
                stalls_resolved=sum(len(g.stalls) for g in games), _started=len(games))
    if not cfg.match:
        want.update(full_plies=sum(sum(g.full) for g in games), resign_would=sum(sum(g.would) for g in games))
    return want


def check_trajectories(cfg, out, games):
    """Every field of every returned Trajectory against the script."""
    assert sorted(t.game_id for t in out) == sorted(g.gid for g in games)
    by_id = dict((g.gid, g) for g in games)
    for t in out:
        g = by_id[t.game_id]
        assert t.moves == g.moves and t.winner == g.winner, t.game_id
        if g.moves:
            assert t.pis.dtype == np.float64 and t.pis.shape == (len(g.moves), cfg.A) and np.array_equal(t.pis, np.array(g.pis)), t.game_id
        assert (t.board_size, t.n_in_row, t.game) == cfg.geometry
        if cfg.cap is None:
            assert t.full is None
        else:
            assert t.full.tolist() == g.full and len(t.full) == len(g.moves) + g.resigned
        if cfg.resign is None:
            assert t.resign_stats is None and not t.resigned and not t.no_resign and np.isnan(t.fp_margin)
            continue
        assert (t.resigned, t.no_resign) == (g.resigned, g.calib)
        assert t.resign_stats.dtype == np.float32 and t.resign_stats.tolist() == [float(s) for s in g.stats]
        assert len(t.resign_stats) == len(g.moves) + g.resigned
        if g.calib:   # the lowest statistic a player who did not lose saw on their own plies
            own = g.stats if g.winner < 0 else g.stats[g.winner::2]
            assert t.fp_margin == min(own)
        else:
            assert np.isnan(t.fp_margin)


# ----------------------------------------------------------------------------------------------- the logs
def plain_games(cfg, ids=range(5), seed=1):
    """Five games through two slots: slots 0 and 1 stall together at ply 1 of their first games, the third game stalls at ply 0, the
    fourth on its last move; a win for each side and a tie; the last game's counts are peaked (the error cases corrupt it)."""
    rng, ids = np.random.RandomState(seed), list(ids)
    return [Game(cfg, rng, ids[0], 4, 0, stalls=[1]), Game(cfg, rng, ids[1], 6, -1, stalls=[1, 3]), Game(cfg, rng, ids[2], 3, 1, stalls=[0]),
            Game(cfg, rng, ids[3], 3, 0, stalls=[2]), Game(cfg, rng, ids[4], 5, 1, peaked=True)]


def rules_games(cfg):
    """Resignation, a playout cap and a schedule at once: a resigning game (stalled once before), a calibration game that would have
    resigned at ply 2, a second calibration game, and two plain ones."""
    rng = np.random.RandomState(2)
    return [Game(cfg, rng, PLAYED[0], 3, None, stalls=[1], resign=True), Game(cfg, rng, CALIB[0], 5, 0, would_at=2),
            Game(cfg, rng, PLAYED[1], 4, 1, peaked=True), Game(cfg, rng, CALIB[1], 2, -1, stalls=[0]), Game(cfg, rng, PLAYED[2], 0, None, resign=True)]


PLAIN = Cfg()
RULES = Cfg(temps=[1.0, 1.0, 1e-3], resign=(THRESHOLD, FRAC), cap=(7, 0.5))
MATCH = Cfg(match=True)
_cache = {}


def logged(name):
    """-> (cfg, games, log, returned, reader, calls) of a named log, written once."""
    if name not in _cache:
        cfg = {'plain': PLAIN, 'rules': RULES, 'match': MATCH}[name]
        games = rules_games(cfg) if name == 'rules' else plain_games(cfg)
        _cache[name] = (cfg, games) + record(cfg, games, delay=2 if name == 'plain' else 0)
    return _cache[name]


# ----------------------------------------------------------------------------------------------- the decoder
def test_decoder_names_every_word():
    rec = np.zeros((2, 3, W0 + 4), dtype=np.int32)
    rec[1, 2] = [-2, 5, 17, 3, PLAY_RUNNING | PLAY_ENDED | (2 << 16), 41, _bits(0.125), _bits(-0.75), 30, -1, 0, 10]
    d = playlog.decode(rec)
    assert d.game.dtype == np.int64 and d.game[1, 2] == (5 << 32) | 0xFFFFFFFE and d.game.shape == (2, 3)
    assert (d.ply[1, 2], d.move[1, 2], d.flags[1, 2], d.winner[1, 2], d.root_n[1, 2]) == (17, 3, PLAY_RUNNING | PLAY_ENDED, 1, 41)
    assert d.edge.dtype == d.stat.dtype == np.float32 and (d.edge[1, 2], d.stat[1, 2]) == (0.125, -0.75)
    assert d.visits[1, 2].tolist() == [30, -1, 0, 10] and d.legal[1, 2].tolist() == [True, False, True, True]
    assert d.counts[1, 2].tolist() == [30, 0, 0, 10] and d.winner[0, 0] == -1
    slots, run, last = playlog.running(rec)
    assert slots.tolist() == [2] and run.ply.tolist() == [17] and last == 1


# ----------------------------------------------------------------------------------------------- self-play
def test_plain_games_stalls_and_refills():
    cfg, games, log, out, reader, calls = logged('plain')
    check_trajectories(cfg, out, games)
    assert [g.winner for g in games] == [0, -1, 1, 0, 1]
    assert counters(reader) == want_counters(cfg, games)          # (a stalled search counts once: sims_done is per SEARCHED record)
    assert (reader.slot_game == -1).all() and reader.book.stalls == {}
    # resolve exactly once per stall, with the script's move; slots 0 and 1 were stalled in the same rows
    stalled = sorted((g.gid, p) for g in games for p in g.stalls)
    assert len(calls) == len(stalled) == 5 and sorted(m for _, m in calls) == sorted(g.moves[p] for g in games for p in g.stalls)
    flags = log[:, :, 4]
    assert ((flags[:, 0] & PLAY_STALLED) != 0)[1] and ((flags[:, 1] & PLAY_STALLED) != 0)[1]
    assert (((flags & PLAY_STALLED) != 0) & ((flags & PLAY_SEARCHED) == 0)).sum() >= 5      # (STALLED was repeated while the move waited)
    assert ((flags & (PLAY_RESOLVED | PLAY_ENDED)) == (PLAY_RESOLVED | PLAY_ENDED)).sum() == 1   # a stall on a game's last move
    assert ((flags == 0).any(axis=1)).any()                        # rows with an idle slot


def test_a_slot_that_stays_idle():
    cfg = PLAIN
    games = [Game(cfg, np.random.RandomState(3), 7, 4, 1)]
    log, out, reader, _ = record(cfg, games)
    assert (log[:, 1, 4] == 0).all()
    check_trajectories(cfg, out, games)
    assert counters(reader) == want_counters(cfg, games)


def test_resignation_cap_and_schedule():
    cfg, games, log, out, reader, calls = logged('rules')
    check_trajectories(cfg, out, games)
    assert counters(reader) == want_counters(cfg, games)
    by_id = dict((t.game_id, t) for t in out)
    quit_ = by_id[PLAYED[0]]
    assert quit_.resigned and len(quit_.moves) == 3 and len(quit_.resign_stats) == 4 and quit_.winner == 0   # (player 1 resigns before ply 3)
    assert by_id[PLAYED[2]].resigned and by_id[PLAYED[2]].moves == [] and by_id[PLAYED[2]].winner == 1       # a game resigned at ply 0
    assert by_id[CALIB[0]].no_resign and not by_id[CALIB[0]].resigned and reader.resign_would == 1
    fulls = [f for g in games for f in g.full]
    assert 0 < sum(fulls) < len(fulls)                                   # both budgets occur
    assert reader.sims_done == 40 * sum(fulls) + 7 * (len(fulls) - sum(fulls)) and reader.full_plies == sum(fulls)
    # the schedule: plies 0 and 1 at T = 1, later plies all but greedy -- their pi is one-hot at the most visited child
    for g in games:
        for ply, pi in enumerate(g.pis):
            if ply >= 2:
                assert pi.max() > 1.0 - 1e-6 and int(pi.argmax()) == int(g.counts[ply].argmax())


def test_pi_temperature_keeps_the_moves():
    """With ``pi_temperature`` the stored pi is the counts' distribution at that T; the moves are those of the schedule."""
    base = Cfg(temps=[1.0, 1e-3])
    flat = Cfg(temps=[1.0, 1e-3], pi_T=1.0)
    games = [plain_games(c, seed=4) for c in (base, flat)]
    for cfg, gs in zip((base, flat), games):
        log, out, reader, _ = record(cfg, gs)
        check_trajectories(cfg, out, gs)
    assert [g.moves for g in games[0]] == [g.moves for g in games[1]]
    assert all(p.max() > 1.0 - 1e-6 for g in games[0] for p in g.pis[1:]) and any(p.max() < 0.9 for g in games[1] for p in g.pis[1:])


def test_connect4_shape():
    """A = 7 actions, 42 plies of room: the action count is not the ply capacity (games longer than 7 plies)."""
    cfg = Cfg(A=7, room=42, geometry=((6, 7), 4, 'connect4'))
    rng = np.random.RandomState(5)
    games = [Game(cfg, rng, 0, 12, 0, stalls=[8]), Game(cfg, rng, 1, 9, 1), Game(cfg, rng, 2, 11, -1, stalls=[0])]
    log, out, reader, _ = record(cfg, games)
    assert log.shape[2] == W0 + 7
    check_trajectories(cfg, out, games)
    assert counters(reader) == want_counters(cfg, games)


@pytest.mark.parametrize('name', ['plain', 'rules', 'match'])
def test_batching_invariance(name):
    """One row per call, all rows in one call, uneven batches: identical games (in order) and counters, one resolve per stall."""
    cfg, games, log, out, reader, calls = logged(name)
    for batches in ([1], None, [3, 1, 5, 2]):
        again, r2, calls2 = replay(cfg, log, batches)
        assert counters(r2) == counters(reader) and calls2 == calls
        assert [t.game_id for t in again] == [t.game_id for t in out]
        for a, b in zip(again, out):
            if cfg.match:
                assert (a.moves, a.winner, a.root_n, a.opening) == (b.moves, b.winner, b.root_n, b.opening)
                assert all(np.array_equal(x, y) for x, y in zip(a.visits, b.visits))
            else:
                assert (a.moves, a.winner, a.resigned, a.no_resign) == (b.moves, b.winner, b.resigned, b.no_resign)
                assert np.array_equal(a.pis, b.pis) and np.array_equal(a.fp_margin, b.fp_margin, equal_nan=True)
                assert (a.full is None and b.full is None) or np.array_equal(a.full, b.full)
                assert (a.resign_stats is None and b.resign_stats is None) or np.array_equal(a.resign_stats, b.resign_stats)


def test_two_lanes_one_book():
    """Two engines' logs (slot offsets 0 and 2) read into one book; a stall is answered to the lane it came from."""
    cfg = PLAIN
    games = [plain_games(cfg, ids=range(0, 5), seed=6), plain_games(cfg, ids=range(10, 15), seed=7)]
    writers = [Writer(cfg, gs, 2, delay=k) for k, gs in enumerate(games)]
    reader = cfg.reader(lambda s, m: writers[s // 2].resolve(s % 2, m), n_slots=4)
    out = []
    while any(w.busy() for w in writers):
        for k, w in enumerate(writers):
            if w.busy():
                out.extend(reader.read_rows(w.step()[None], lo=2 * k)[0])
    check_trajectories(cfg, out, games[0] + games[1])
    assert counters(reader) == want_counters(cfg, games[0] + games[1])
    assert all(len(w.calls) == 5 for w in writers)


# ----------------------------------------------------------------------------------------------- matches
def test_match_reader():
    cfg, games, log, out, reader, calls = logged('match')
    assert counters(reader) == want_counters(cfg, games) and len(calls) == 5
    assert sorted(r.game_id for r in out) == [0, 1, 2, 3, 4]
    for r in out:
        g = games[r.game_id]
        assert r.moves == g.moves and r.winner == g.winner and r.root_n == [N_PLAYOUT] * len(g.moves)
        assert r.opening == (r.game_id >> 1) % 3 and r.opening_moves == OPENINGS[r.opening]
        # the visits the move was drawn from: a resolved ply's are the STALLED record's, not the RESOLVED record's
        assert len(r.visits) == len(g.moves) and all(np.array_equal(v, c) for v, c in zip(r.visits, g.counts))
    # the pair's uniform: games 2k and 2k + 1 draw ply p with the same u, the second of get_action's two
    assert match_uniform(SEED, 2, 3) == match_uniform(SEED, 3, 3) == move_uniform(SEED, 1, 7)


# ----------------------------------------------------------------------------------------------- errors
def _find(log, want, avoid=0, ply=None, gid=None, nth=0):
    """(row, slot) of the nth record whose flags hold ``want`` and none of ``avoid``."""
    d = playlog.decode(log)
    ok = ((d.flags & want) == want) & ((d.flags & avoid) == 0)
    if ply is not None:
        ok &= ply(d.ply) if callable(ply) else d.ply == ply
    if gid is not None:
        ok &= d.game == gid
    r, s = np.argwhere(ok)[nth]
    return int(r), int(s)


def _raises(name, where, word, value, match):
    """One word of a valid log corrupted: reading raises ``match``; the rows before it are read in a call of their own, so the
    failing call has returned nothing and the games found before it are what a good log gives up to there."""
    cfg, games, log, out, _, _ = logged(name)
    r, s = where(log)
    bad = log.copy()
    bad[r, s, word] = value(bad[r, s, word]) if callable(value) else value
    assert not np.array_equal(bad, log)
    reader = cfg.reader(lambda slot, move: None)
    got = list(reader.read_rows(bad[:r])[0]) if r else []
    good = [t.game_id for t in replay(cfg, log[:r])[0]] if r else []
    with pytest.raises(HipError, match=match):
        got.extend(reader.read_rows(bad[r:])[0])
    assert [t.game_id for t in got] == good


MID = PLAY_STALLED | PLAY_RESOLVED | PLAY_RESIGNED | PLAY_ENDED
PEAKED_PLAIN, PEAKED_RULES = 4, PLAYED[1]     # the games whose draws do not depend on the uniform


def test_wrong_move():
    def other(m):
        return (m + 1) % 9
    _raises('plain', lambda log: _find(log, PLAY_SEARCHED, MID, ply=lambda p: p > 0), 3, other, r"the move drawn on the device \(\d+\) is not numpy's")


def test_slot_mismatch_in_the_vectorised_path():
    _raises('plain', lambda log: _find(log, PLAY_SEARCHED, MID, ply=2, gid=PEAKED_PLAIN), 2, 3,
            r'slot \d: the log says game 4 ply 3, the host expected game 4 ply 2')


def test_slot_mismatch_in_the_per_record_path():
    _raises('plain', lambda log: _find(log, PLAY_ENDED, gid=PEAKED_PLAIN), 2, 3, r'slot \d: the log says game 4 ply 3, the host expected game 4 ply 4')


def test_resolved_without_a_stall():
    _raises('plain', lambda log: _find(log, PLAY_SEARCHED, MID, ply=2, gid=PEAKED_PLAIN), 4, PLAY_RUNNING | PLAY_RESOLVED,
            r'the device resolved game 4 ply 2 with move \d, the host had decided None')


def test_resolved_with_another_move():
    _raises('plain', lambda log: _find(log, PLAY_RESOLVED), 3, lambda m: (m + 1) % 9, r'the device resolved game \d ply \d with move \d, the host had decided \(')


def test_budget_flag_flipped():
    _raises('rules', lambda log: _find(log, PLAY_SEARCHED, MID, ply=lambda p: p > 0), 4, lambda f: f ^ PLAY_FULL,
            r"the device's budget flag 0x[0-9a-f]+ of game \d+ ply \d disagrees with cap_uniform")


def test_no_resign_flipped():
    _raises('rules', lambda log: _find(log, PLAY_SEARCHED, MID, ply=lambda p: p > 0), 4, lambda f: f ^ PLAY_NO_RESIGN,
            r"the device's resignation flags 0x[0-9a-f]+ of game \d+ ply \d disagree with s = ")


def test_fired_above_the_threshold():
    _raises('rules', lambda log: _find(log, PLAY_RESIGNED), 7, _bits(-0.5), r"resignation flags 0x[0-9a-f]+ of game \d+ ply \d disagree with s = -0.5, threshold -0.8, calibration False")


def test_not_fired_below_the_threshold():
    _raises('rules', lambda log: _find(log, PLAY_SEARCHED, MID | PLAY_WOULD_RESIGN, gid=PEAKED_RULES, ply=1), 7, _bits(-0.9),
            r"resignation flags 0x[0-9a-f]+ of game \d+ ply 1 disagree with s = -0.8999\d+, threshold -0.8, calibration False")


def test_resigned_in_a_calibration_game():
    _raises('rules', lambda log: _find(log, PLAY_WOULD_RESIGN), 4, lambda f: f | PLAY_RESIGNED,
            r"resignation flags 0x[0-9a-f]+ of game \d+ ply 2 disagree with s = -0.9\d+, threshold -0.8, calibration True")


def test_match_root_of_the_wrong_size():
    _raises('match', lambda log: _find(log, PLAY_SEARCHED, MID, ply=lambda p: p > 0), 5, N_PLAYOUT - 1,
            r'game \d ply \d was drawn from a root of 39 visits, not n_playout = 40')
