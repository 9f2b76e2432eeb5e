"""The host-driven loop's bookkeeping without a GPU: SelfPlayReader.decide_and_record / SlotBook.close / SelfPlayReader.trajectory are
driven move by move with the scripted games of tests/test_playlog_host.py -- the counts, values and pruned rows an engine would hand
over -- and what they return is held against the script (the reference's expressions, formed there and here from oracle.mcts_ref) and
against what read_rows returns for the scripted device log of the same games.  Then the book's direct writer against feed, and the
three views other code reads (slot_moves, slot_pis, slot_values).  3 x 3 boards, 2 slots, 5 games; one case of Connect4's shape."""
import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import forced_twin as ft
from oracle.mcts_ref import softmax
from rlzero_amd import playlog
from rlzero_amd._hip import PLAY_RUNNING, HipError
from test_playlog_host import (CALIB, FRAC, PLAIN, PLAYED, RULES, THRESHOLD, Cfg, Game, Writer, check_trajectories, counters, plain_games,
                               rules_games, want_counters)

C_PUCT = 5.0


class Case(object):
    """A configuration and its five games; per game and search what an engine adds to the counts: (v_root, q_best) in fp64 -- the
    script's statistic is their maximum, and on odd plies it is q_best that stays above a threshold v_root is below -- and the pruned
    counts (forced_twin.pruned_counts on scripted value sums and priors).  The expected pis are then the pruned counts'."""

    def __init__(self, cfg, games, values=False, forced=None, seed=8):
        self.cfg, self.games, self.values_on, self.forced = cfg, games, values, forced
        rng = np.random.RandomState(seed)
        self.vals, self.pruned, self.lowered = {}, {}, 0
        for g in games:
            main = np.array(g.stats, dtype=np.float64) if cfg.resign is not None else rng.uniform(-1.0, 1.0, len(g.counts))
            self.vals[g.gid] = np.stack([main, main - 0.25], axis=1)
            swap = [i for i in range(1, len(main), 2) if main[i] > THRESHOLD]
            self.vals[g.gid][swap] = np.stack([np.full(len(swap), -0.99), main[swap]], axis=1)
            self.pruned[g.gid] = [self.prune(rng, c) for c in g.counts]
            if forced is not None and forced[1]:
                g.pis = [self.pi_of(self.pruned[g.gid][ply], ply) for ply in range(len(g.moves))]

    def prune(self, rng, counts):
        legal = np.nonzero(counts >= 0)[0]
        n = counts[legal].tolist()
        w = [float(rng.uniform(-1.0, 1.0) * x) for x in n]
        p = [np.float32(x) for x in rng.dirichlet(np.full(len(legal), 0.5))]
        out = np.full(len(counts), -1, dtype=np.int32)
        out[legal] = ft.pruned_counts(n, w, p, sum(n) + 1, ft.K, C_PUCT)
        self.lowered += int((out[legal] < counts[legal]).sum())
        return out

    def pi_of(self, counts, ply):
        legal = np.nonzero(counts >= 0)[0]
        pi = np.zeros(self.cfg.A)
        pi[legal] = softmax(1.0 / (self.cfg.pi_T or self.cfg.T(ply)) * np.log(counts[legal] + 1e-10))
        return pi

    def reader(self, resolve=lambda slot, move: None):
        r = self.cfg.reader(resolve, 2)
        r.root_values_on = self.values_on
        if self.forced is not None:
            r.forced_k, r.forced_prune = ft.K, self.forced[1]
            r.book.set_column('raw', (np.int32, (self.cfg.A, ), 'move'))
        return r

    def engine_rows(self, gids, plies):
        """-> (visits, legal, values, pruned) of the searches before ``plies`` of ``gids``, as the host loop fetches them."""
        by_id = dict((g.gid, g) for g in self.games)
        counts = np.stack([by_id[g].counts[p] for g, p in zip(gids, plies)])
        values = np.stack([self.vals[g][p] for g, p in zip(gids, plies)]) if self.values_on or self.cfg.resign is not None else None
        pruned = np.stack([self.pruned[g][p] for g, p in zip(gids, plies)]) if self.forced is not None and self.forced[1] else None
        return np.where(counts >= 0, counts, 0), counts >= 0, values, pruned


def host_loop(case):
    """The host-driven loop on the script: slots refill after the move that ended their game -> (trajectories, the reader)."""
    reader, queue, slot, out = case.reader(), list(case.games), [None, None], []
    while queue or any(g is not None for g in slot):
        for s in range(2):
            if slot[s] is None and queue:
                slot[s] = queue.pop(0)
                reader.book.start(s, slot[s].gid)
        running = np.array([s for s in range(2) if slot[s] is not None])
        plies = reader.slot_ply[running].copy()
        moves, quit_ = reader.decide_and_record(running, *case.engine_rows([slot[s].gid for s in running], plies))
        for s, ply, move, gone in zip(running, plies, moves, quit_):
            g = slot[s]
            assert gone == (g.resigned and ply == len(g.moves)) and move == (-1 if gone else g.moves[ply]), (g.gid, ply)
            if gone or ply + 1 == len(g.moves) and not g.resigned:
                out.append(reader.trajectory(reader.book.close(s, 1 - ply % 2 if gone else g.winner, bool(gone))))
                slot[s] = None
    return out, reader


def device_log(case):
    """The scripted device's log of the same games through read_rows, with the side rings the options ask for."""
    w = Writer(case.cfg, case.games, 2, delay=0)
    reader, out, busy = case.reader(w.resolve), [], True
    while busy:
        busy = w.busy()
        row = w.step()[None]
        d = playlog.decode(row[0])
        on = np.nonzero((d.flags & PLAY_RUNNING) != 0)[0]
        values, pruned = np.zeros((1, 2), dtype=np.float32), np.zeros((1, 2, case.cfg.A), dtype=np.int32)
        for s in on:
            values[0, s] = case.vals[int(d.game[s])][d.ply[s], 0]
            pruned[0, s] = case.pruned[int(d.game[s])][d.ply[s]]
        kw = dict(values=values) if case.values_on else {}
        if case.forced is not None and case.forced[1]:
            kw['pruned'] = pruned
        out.extend(reader.read_rows(row, **kw)[0])
    return out, reader


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def smooth_games(cfg, seed=9):
    """Five games without stalls (a stall's RESOLVED record carries counts that mean nothing -- no pruned row fits them)."""
    rng = np.random.RandomState(seed)
    return [Game(cfg, rng, gid, n, w) for gid, n, w in ((0, 4, 0), (1, 6, -1), (2, 3, 1), (3, 9, 0), (4, 5, 1))]


def resign_games(cfg):
    """One resigning game, one calibration game where the rule fires (ply 2), one that plays on; a game resigned at ply 0, a tie."""
    rng = np.random.RandomState(10)
    return [Game(cfg, rng, PLAYED[0], 3, None, resign=True), Game(cfg, rng, CALIB[0], 5, 0, would_at=2), Game(cfg, rng, PLAYED[1], 4, 1),
            Game(cfg, rng, PLAYED[2], 0, None, resign=True), Game(cfg, rng, CALIB[1], 6, -1)]


RESIGN = Cfg(resign=(THRESHOLD, FRAC))
CAP = Cfg(cap=(7, 0.5))
SCHEDULE = Cfg(temps=[1.0, 1.0, 1e-3], pi_T=0.5)
CONNECT4 = Cfg(A=7, room=42, geometry=((6, 7), 4, 'connect4'))
CASES = {
    'plain': lambda: Case(PLAIN, plain_games(PLAIN)),
    'resign': lambda: Case(RESIGN, resign_games(RESIGN)),
    'cap': lambda: Case(CAP, plain_games(CAP)),
    'schedule': lambda: Case(SCHEDULE, plain_games(SCHEDULE)),
    'values': lambda: Case(PLAIN, plain_games(PLAIN), values=True),
    'values_resign': lambda: Case(RESIGN, resign_games(RESIGN), values=True),
    'rules': lambda: Case(RULES, rules_games(RULES), values=True),
    'forced_pruned': lambda: Case(PLAIN, smooth_games(PLAIN), forced=(ft.K, True)),
    'forced_raw': lambda: Case(PLAIN, smooth_games(PLAIN), forced=(ft.K, False)),
    'connect4': lambda: Case(CONNECT4, [Game(CONNECT4, np.random.RandomState(5), gid, n, w) for gid, n, w in
                                        ((0, 12, 0), (1, 9, 1), (2, 11, -1), (3, 8, 1), (4, 15, 0))]),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_loop_against_script_and_log(name):
    case = CASES[name]()
    cfg, games = case.cfg, case.games
    out, reader = host_loop(case)
    check_trajectories(cfg, out, games)
    by_id = dict((g.gid, g) for g in games)
    for t in out:
        g = by_id[t.game_id]
        assert t.epochs is None
        if case.values_on:   # one entry per move: the resigning search is not recorded
            assert same(t.root_values, np.array([case.vals[g.gid][p, 0] for p in range(len(g.moves))], dtype=np.float32).reshape(-1))
        else:
            assert t.root_values is None
        if case.forced is not None:   # the raw counts the move was drawn from, whatever the pis are formed from
            assert same(t.raw_visits, np.maximum(np.array(g.counts[:len(g.moves)], dtype=np.int32), 0).reshape(len(g.moves), -1))
        else:
            assert t.raw_visits is None
    want = want_counters(cfg, games)
    assert counters(reader) == dict(want, stalls_resolved=0, _started=0)   # (no device queue, no stall: those two are feed's)
    assert (reader.slot_game == -1).all()
    if case.forced is not None:
        assert case.lowered > 10                                   # the pruning rule was at work ...
        raw_pis = [Case.pi_of(case, g.counts[p], p) for g in games for p in range(len(g.moves))]
        differs = any(not np.array_equal(a, b) for a, b in zip(raw_pis, [pi for g in games for pi in g.pis]))
        assert differs == case.forced[1]                           # ... and the stored pis are the pruned counts' only when asked
    if name in ('resign', 'values_resign', 'rules'):
        assert reader.resign_would == 1 and sum(t.resigned for t in out) == 2 and sum(t.no_resign for t in out) == 2
        # searches with v_root below the threshold and q_best above it: host_loop saw nobody resign there
        assert sum(int((v[:, 0] < THRESHOLD).sum() - (v.max(axis=1) < THRESHOLD).sum()) for v in case.vals.values()) >= 5
    if name in ('cap', 'rules'):
        assert 0 < reader.full_plies < sum(len(g.full) for g in games)
    # ... and what read_rows makes of the device's log of the same games
    dev, dev_reader = device_log(case)
    assert sorted(t.game_id for t in dev) == sorted(t.game_id for t in out)
    dev = dict((t.game_id, t) for t in dev)
    for t in out:
        u = dev[t.game_id]
        assert (t.moves, t.winner, t.resigned, t.no_resign, t.board_size, t.n_in_row, t.game) == \
            (u.moves, u.winner, u.resigned, u.no_resign, u.board_size, u.n_in_row, u.game)
        for field in ('pis', 'resign_stats', 'fp_margin', 'full', 'root_values', 'raw_visits', 'epochs'):
            assert same(getattr(t, field), getattr(u, field)), (t.game_id, field)
    for k in ('moves_done', 'sims_done', 'full_plies', 'resign_would'):
        assert getattr(reader, k) == getattr(dev_reader, k) == want[k], k


@pytest.mark.parametrize('name', ['plain', 'resign', 'values', 'rules', 'forced_pruned'])
def test_a_lane_without_a_running_slot(name):
    """play_move finishes every lane, one whose slots are all idle too: nothing was fetched for it (no values, no pruned rows),
    nothing is decided, no counter and no slot moves -- with a game running in another lane's slot, and before any game."""
    case = CASES[name]()
    reader = case.reader()
    for started in (False, True):
        if started:
            _play(reader, case, 1, case.games[1], 2)
        before = (counters(reader), reader.slot_game.tolist(), reader.slot_ply.tolist(), reader.slot_moves[1])
        moves, quit_ = reader.decide_and_record(np.zeros(0, dtype=np.int64), np.zeros((0, 9), dtype=np.int32), np.zeros((0, 9), dtype=bool), None, None)
        assert moves.shape == quit_.shape == (0, ) and moves.dtype == np.int64 and quit_.dtype == bool
        assert (counters(reader), reader.slot_game.tolist(), reader.slot_ply.tolist(), reader.slot_moves[1]) == before
    # ... while a running slot without what its options need is still refused
    if name != 'plain':
        with pytest.raises(ValueError, match='needs'):
            reader.decide_and_record(np.array([1]), *case.engine_rows([case.games[1].gid], [2])[:2])


# ----------------------------------------------------------------------------------------------- the book's writer alone
COLUMNS = {'n': (np.int32, (), 'move'), 'stat': (np.float32, (), 'search')}


@pytest.mark.parametrize('resign', [False, True])
def test_direct_writer_equals_feed(resign):
    cfg = RESIGN if resign else PLAIN
    game = Game(cfg, np.random.RandomState(12), PLAYED[0], 4, None if resign else 1, resign=resign)
    w = Writer(cfg, [game], 1)
    fed, direct = [playlog.SlotBook(1, 9, None, COLUMNS) for _ in range(2)]
    from_feed, root_n = [], []
    while w.busy():
        at, d, _ = playlog.running(w.step()[None])
        root_n.append(int(d.root_n[0]))
        from_feed.extend(fed.feed(at, d, d.move, {'n': d.root_n, 'stat': d.stat}))
    direct.start(0, game.gid)
    for ply in range(len(game.counts)):
        direct.put_search(np.array([0]), np.array([ply]), {'stat': np.array([game.stats[ply]])})
        if ply < len(game.moves):
            direct.put_moves(np.array([0]), np.array([ply]), np.array([game.moves[ply]]), {'n': np.array([root_n[ply]])})
    f, g = from_feed[0], direct.close(0, game.winner, resign)
    assert len(from_feed) == 1 and (f.slot, f.game, f.searched, f.winner, f.resigned) == (g.slot, g.game, g.searched, g.winner, g.resigned)
    assert g.searched == len(game.moves) + resign and same(f.moves, g.moves) and sorted(f.columns) == sorted(g.columns) == ['n', 'stat']
    assert all(same(f.columns[k], g.columns[k]) for k in f.columns)
    assert (fed.moves_done, direct.moves_done) == (len(game.moves), len(game.moves)) and (fed.started, direct.started) == (1, 0)
    assert direct.slot_game[0] == -1


def test_direct_writer_refusals():
    book = playlog.SlotBook(2, 9, None, COLUMNS)
    with pytest.raises(HipError, match='slot 1 holds no game'):
        book.close(1, 0, False)
    with pytest.raises(HipError, match=r'slot 1: a write at ply 0, the book has game -1'):
        book.put_search(np.array([1]), np.array([0]), {'stat': np.zeros(1)})
    book.start(1, 7)
    book.put_moves(np.array([1]), np.array([0]), np.array([4]), {'n': np.array([3])})
    with pytest.raises(HipError, match=r'slot 1: a write at ply 0, the book has game 7 at ply 1'):
        book.put_moves(np.array([1]), np.array([0]), np.array([5]), {'n': np.array([3])})
    with pytest.raises(HipError, match=r'slot 1: a write at ply 2, the book has game 7 at ply 1'):
        book.put_search(np.array([1]), np.array([2]), {'stat': np.zeros(1)})
    with pytest.raises(HipError, match=r'slot 0: a write at ply 0, the book has game -1'):
        book.put_moves(np.array([1, 0]), np.array([1, 0]), np.array([5, 5]), {'n': np.array([3, 3])})
    assert book.moves_done == 1 and book.slot_ply.tolist() == [0, 1]   # (a refused write changes nothing)
    assert book.close(1, 1, False).moves.tolist() == [4]
    with pytest.raises(HipError, match='slot 1 holds no game'):
        book.close(1, 1, False)


# ----------------------------------------------------------------------------------------------- the views
def _play(reader, case, slot, game, n_moves):
    reader.book.start(slot, game.gid)
    for ply in range(n_moves):
        reader.decide_and_record(np.array([slot]), *case.engine_rows([game.gid], [ply]))


def test_views_of_the_book():
    case = CASES['values']()
    a, b = case.games[0], case.games[1]
    reader, other = case.reader(), case.reader()
    assert isinstance(reader.slot_moves[0], list) and not reader.slot_moves[0] and len(reader.slot_pis[0]) == 0
    assert reader.slot_moves == other.slot_moves
    _play(reader, case, 0, a, 3)
    _play(reader, case, 1, b, 2)
    assert isinstance(reader.slot_moves[0], list) and reader.slot_moves[0] == a.moves[:3] and reader.slot_moves[1] == b.moves[:2]
    assert reader.slot_moves[0][-1] == a.moves[2] and np.array_equal(reader.slot_pis[0][-1], a.pis[2])
    assert reader.slot_pis[0].dtype == np.float64 and reader.slot_pis[0].shape == (3, 9)
    assert same(reader.slot_values[0], case.vals[a.gid][:3, 0].astype(np.float32))
    assert reader.slot_moves != other.slot_moves
    _play(other, case, 0, a, 3)
    assert reader.slot_moves != other.slot_moves            # slot 1 still differs
    _play(other, case, 1, b, 2)
    assert reader.slot_moves == other.slot_moves and not reader.slot_moves != other.slot_moves
    # a closed slot keeps its last game's plies until it starts another
    reader.book.close(1, 0, False)
    assert reader.slot_game[1] == -1 and reader.slot_moves[1] == b.moves[:2] and reader.slot_moves == other.slot_moves
    reader.book.start(1, case.games[2].gid)
    assert reader.slot_moves[1] == [] and not reader.slot_moves[1] and reader.slot_moves != other.slot_moves
