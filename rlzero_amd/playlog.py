"""The host's reader of the device move step's log (include/rlzero_hip.h, "The log: ..."): the one decoder of its records, and the
book both consumers -- self-play (selfplay.SelfPlayReader) and matches (match.MatchReader) -- keep of what each slot is playing.
numpy only: no torch, no engine; the owner hands in the rows, the arbiter's moves and a ``resolve`` callable."""
import collections

import numpy as np

from ._hip import (PLAY_ENDED, PLAY_FULL, PLAY_NO_RESIGN, PLAY_RECORD_WORDS, PLAY_RESIGNED, PLAY_RESOLVED, PLAY_RUNNING, PLAY_SEARCHED,
                   PLAY_STALLED, PLAY_WOULD_RESIGN, HipError)

Records = collections.namedtuple('Records', 'game ply move flags winner root_n edge stat visits legal counts')
Finished = collections.namedtuple('Finished', 'slot game moves searched winner resigned columns')


def decode(rec):
    """Records int32 [..., PLAY_RECORD_WORDS + A] -> their fields as arrays [...]: game id (int64), ply before the move, the move or
    -1, the PLAY_* flags, the winner (-1: none / a tie), N(root), the draw's distance to the nearer interval edge and the resignation
    statistic (float32), and per action [..., A] the visit counts as logged (-1: illegal), ``legal``, and ``counts`` with 0 there."""
    rec = np.asarray(rec)
    visits = rec[..., PLAY_RECORD_WORDS:]
    legal = visits >= 0
    return Records(game=rec[..., 0].astype(np.uint32).astype(np.int64) | (rec[..., 1].astype(np.int64) << 32), ply=rec[..., 2].astype(np.int64),
                   move=rec[..., 3], flags=rec[..., 4] & 0xFFFF, winner=((rec[..., 4] >> 16) & 3) - 1, root_n=rec[..., 5],
                   edge=np.ascontiguousarray(rec[..., 6]).view(np.float32), stat=np.ascontiguousarray(rec[..., 7]).view(np.float32),
                   visits=visits, legal=legal, counts=np.where(legal, visits, 0))


def running(rows):
    """Log rows int32 [R, G, words] -> (slot of every RUNNING record, row-major: a slot's records in move order; those records
    decoded; the number of them in the last row)."""
    on = (rows[..., 4] & PLAY_RUNNING) != 0
    row_i, g_i = np.nonzero(on)
    return g_i, decode(rows[row_i, g_i]), int(on[-1].sum())


def running_values(rows, side):
    """The optional column of the log: the side ring of root values (rz_play_set_root_values), float32 [R, G] -- the same rows as
    ``rows`` -> its entries of the RUNNING records, in running()'s order (a stalled slot's rows repeat its searched record's value)."""
    side = np.asarray(side, dtype=np.float32)
    if side.shape != rows.shape[:2]:
        raise ValueError('the side ring\'s rows %r do not match the log\'s %r' % (side.shape, rows.shape[:2]))
    row_i, g_i = np.nonzero((rows[..., 4] & PLAY_RUNNING) != 0)
    return side[row_i, g_i]


def check_moves(d, chosen):
    """Every move the device drew is the arbiter's (a stalled, resolved or resigning record holds no draw)."""
    wrong = ((d.flags & (PLAY_STALLED | PLAY_RESOLVED | PLAY_RESIGNED)) == 0) & (chosen != d.move)
    if wrong.any():
        i = np.nonzero(wrong)[0][0]
        raise HipError('the move drawn on the device (%d) is not numpy\'s (%d): game %d, ply %d' % (d.move[i], chosen[i], d.game[i], d.ply[i]))


def check_budgets(d, n_playout, cap=None, cap_u=None):
    """-> (simulations, searches with the full budget) of the searched records.  Under a playout cap ``cap`` = (n_fast, p_full) the
    device's budget flag is held against this side's draw on the same key, ``cap_u`` (selfplay.cap_uniform of the records)."""
    searched = (d.flags & PLAY_SEARCHED) != 0
    if cap is None:
        return n_playout * int(searched.sum()), int(searched.sum())
    fulls = (d.flags & PLAY_FULL) != 0
    bad = searched & (fulls != (cap_u < cap[1]))
    if bad.any():
        i = np.nonzero(bad)[0][0]
        raise HipError('the device\'s budget flag 0x%x of game %d ply %d disagrees with cap_uniform = %r, p_full %r' % (
            d.flags[i], d.game[i], d.ply[i], float(cap_u[i]), cap[1]))
    return int(np.where(fulls, n_playout, cap[0])[searched].sum()), int((fulls & searched).sum())


def check_resignation(d, threshold, calib):
    """The device's decision against its logged statistic s (float32 of the fp64 s it compared): resigned / would resign =>
    s <= threshold, played on => s >= threshold or NaN; the calibration flag against this side's draw ``calib`` (bool per record).
    -> the records of calibration games where the rule fired."""
    t32, flags = np.float32(threshold), d.flags
    searched = (flags & PLAY_SEARCHED) != 0
    fired = (flags & (PLAY_RESIGNED | PLAY_WOULD_RESIGN)) != 0
    with np.errstate(invalid='ignore'):
        bad = searched & (((flags & PLAY_NO_RESIGN) != 0) != calib)
        bad |= searched & fired & ~(d.stat <= t32)
        bad |= searched & ~fired & (d.stat < t32)
        bad |= ((flags & PLAY_RESIGNED) != 0) & calib
    if bad.any():
        i = np.nonzero(bad)[0][0]
        raise HipError('the device\'s resignation flags 0x%x of game %d ply %d disagree with s = %r, threshold %r, calibration %s' % (
            flags[i], d.game[i], d.ply[i], float(d.stat[i]), threshold, bool(calib[i])))
    return int(((flags & PLAY_WOULD_RESIGN) != 0).sum())


def check_match_roots(d, n_playout):
    """A match draws every move from a fresh root and ONE search of n_playout simulations -> the searched records."""
    bad = ((d.flags & PLAY_SEARCHED) != 0) & (d.root_n != n_playout)
    if bad.any():
        i = np.nonzero(bad)[0][0]
        raise HipError('game %d ply %d was drawn from a root of %d visits, not n_playout = %d' % (d.game[i], d.ply[i], d.root_n[i], n_playout))
    return int(((d.flags & PLAY_SEARCHED) != 0).sum())


def counter(name):
    """A counter of an owner's ``book`` as an attribute of the owner."""
    return property(lambda self: getattr(self.book, name), lambda self, value: setattr(self.book, name, value))


class Plies(object):
    """A read-only view ``v`` of a book's column (None: the moves): ``v[slot]`` is the entries of the plies of the slot's game -- of its
    last one until the slot starts another --, a list (``as_list``) or an array, sliced when asked for; two views are equal when
    every slot's entries are -- exactly: meant for the moves -- and, mutable, a view has no hash."""

    def __init__(self, book, column, as_list=False):
        self.book, self.column, self.as_list = book, column, as_list

    def __len__(self):
        return len(self.book.slot_ply)

    def __getitem__(self, slot):
        rows = (self.book.moves if self.column is None else self.book.buf[self.column])[slot, :self.book.slot_ply[slot]]
        return rows.tolist() if self.as_list else rows

    def __eq__(self, other):
        if not hasattr(other, '__len__'):
            return NotImplemented
        return len(self) == len(other) and all(np.array_equal(self[s], other[s]) for s in range(len(self)))


class SlotBook(object):
    """Which game and ply every slot is at, what its plies logged, and the stalls the host has decided.

    ``columns``: {name: (dtype, shape of one entry, 'move' | 'search')} -- what to keep per ply beside the move: a 'move' column of every
    move played, a 'search' column of every SEARCHED record (the stalled one and the resigning one included: a resigned game has ``ply``
    moves and ``ply + 1`` searches).  ``resolve(slot, move)`` hands a stalled slot's move back to the device.
    Two ways in: ``feed`` for the records of a log, ``start`` / ``put_search`` / ``put_moves`` / ``close`` for an owner that has the moves."""

    def __init__(self, n_slots, max_plies, resolve, columns):
        self.resolve = resolve
        self.slot_game = np.full(n_slots, -1, dtype=np.int64)
        self.slot_ply = np.zeros(n_slots, dtype=np.int64)
        self.move_cols = [name for name, (_, _, per) in columns.items() if per == 'move']
        self.search_cols = [name for name, (_, _, per) in columns.items() if per == 'search']
        self.moves = np.zeros((n_slots, max_plies), dtype=np.int32)
        self.buf = dict((name, np.zeros((n_slots, max_plies) + tuple(shape), dtype=dtype))   # (pages are touched as games grow)
                        for name, (dtype, shape, _) in columns.items())
        self.stalls = {}    # slot -> (game id, ply, move, the 'move' columns of its record): decided here, waiting for the device to take it
        self.started = self.stalls_resolved = self.moves_done = 0

    def set_column(self, name, spec=None):
        """Add a column ((dtype, shape of one entry, 'move' | 'search')) or, ``spec`` None, drop it -- between runs, with every slot
        idle: an optional column costs its pages only while its option is on."""
        if (self.slot_game >= 0).any() or self.stalls:
            raise HipError('the columns of a book change only while every slot is idle')
        for cols in (self.move_cols, self.search_cols):
            if name in cols:
                cols.remove(name)
        self.buf.pop(name, None)
        if spec is not None:
            dtype, shape, per = spec
            (self.move_cols if per == 'move' else self.search_cols).append(name)
            self.buf[name] = np.zeros(self.moves.shape + tuple(shape), dtype=dtype)

    def clear(self):
        """Every slot idle, no stall waiting."""
        self.slot_game[:] = -1
        self.stalls = {}

    def _expect(self, slot, game, ply):
        if self.slot_game[slot] != game or self.slot_ply[slot] != ply:
            raise HipError('slot %d: the log says game %d ply %d, the host expected game %d ply %d' % (
                slot, game, ply, self.slot_game[slot], self.slot_ply[slot]))

    # The direct writer.  ``slots`` / ``plies``: one slot or an array of distinct ones, and the ply the CALLER counts each to be at: a
    # caller out of step with the book -- an idle slot, a ply written twice, a count kept elsewhere -- is refused before anything is
    # written (SelfPlayReader reads its plies from the book: there the idle half is the one at work).
    def _here(self, slots, plies):
        bad = np.atleast_1d((self.slot_game[slots] < 0) | (self.slot_ply[slots] != plies))
        if bad.any():
            i = np.nonzero(bad)[0][0]
            s, p = int(np.atleast_1d(slots)[i]), int(np.atleast_1d(plies)[i])
            raise HipError('slot %d: a write at ply %d, the book has game %d at ply %d' % (s, p, self.slot_game[s], self.slot_ply[s]))

    def start(self, slot, game):
        """``slot`` begins ``game`` at ply 0 (``started`` counts the ids taken from the device's queue: feed's alone)."""
        self.slot_game[slot], self.slot_ply[slot] = game, 0

    def put_search(self, slots, plies, values, check=True):
        """The 'search' columns ({name: one entry per slot, or one for all}) of the searches before the slots' plies (``check``
        False: feed's records, held against the log by feed itself)."""
        if check:
            self._here(slots, plies)
        for name in self.search_cols:
            self.buf[name][slots, plies] = values[name]

    def put_moves(self, slots, plies, moves, values, check=True):
        """One move per slot with its 'move' columns ({name: one entry per slot}); the slots are a ply further."""
        if check:
            self._here(slots, plies)
        self.moves[slots, plies] = moves
        for name in self.move_cols:
            self.buf[name][slots, plies] = values[name]
        self.slot_ply[slots] += 1
        self.moves_done += int(np.size(slots))

    def close(self, slot, winner, resigned):
        """The slot's game has ended, ``resigned``: by the resignation of the player to move, after one search more than moves ->
        Finished, each column copied up to its own length; the slot is idle."""
        game, plies = int(self.slot_game[slot]), int(self.slot_ply[slot])
        if game < 0:
            raise HipError('slot %d holds no game to close' % slot)
        searched = plies + (1 if resigned else 0)
        self.slot_game[slot] = -1
        cols = dict((name, self.buf[name][slot, :plies].copy()) for name in self.move_cols)
        cols.update((name, self.buf[name][slot, :searched].copy()) for name in self.search_cols)
        return Finished(slot, game, self.moves[slot, :plies].copy(), searched, winner, resigned, cols)

    def feed(self, slots, d, chosen, values):
        """The RUNNING records of one or more log rows, row-major (a new row begins where the slot number does not rise): ``slots``
        their global slot numbers, ``d`` their fields (decode), ``chosen`` the arbiter's move and ``values`` {column: array} per
        record -> [Finished] of the games that ended in them, each column copied up to its own length."""
        flags, gids, plies = d.flags, d.game, d.ply
        special = ((flags & (PLAY_STALLED | PLAY_RESOLVED | PLAY_RESIGNED | PLAY_ENDED)) != 0) | (plies == 0)
        done = []

        def pick(cols, at):
            return dict((name, values[name][at]) for name in cols)
        first = [0] + (np.nonzero(slots[1:] <= slots[:-1])[0] + 1).tolist() + [len(slots)]
        for a, b in zip(first[:-1], first[1:]):
            easy = np.nonzero(~special[a:b])[0] + a
            if easy.size:   # moves in the middle of a game: the whole row at once
                s, p = slots[easy], plies[easy]
                bad = (self.slot_game[s] != gids[easy]) | (self.slot_ply[s] != p)
                if bad.any():
                    i = easy[np.nonzero(bad)[0][0]]
                    self._expect(slots[i], gids[i], plies[i])
                self.put_search(s, p, pick(self.search_cols, easy), check=False)
                self.put_moves(s, p, d.move[easy], pick(self.move_cols, easy), check=False)
            for i in np.nonzero(special[a:b])[0] + a:
                s, f, gid, ply, mv = int(slots[i]), int(flags[i]), int(gids[i]), int(plies[i]), int(d.move[i])
                if f & PLAY_SEARCHED:   # (a stall's searched record comes before the resolved one of its ply)
                    self.put_search(s, ply, pick(self.search_cols, i), check=False)
                if f & PLAY_STALLED:
                    known = self.stalls.get(s)
                    if known is None or known[:2] != (gid, ply):   # first sight of this stall: decide, hand the move back
                        self.stalls[s] = (gid, ply, int(chosen[i]), dict((name, np.array(values[name][i])) for name in self.move_cols))
                        self.resolve(s, int(chosen[i]))
                    continue
                played = None
                if f & PLAY_RESOLVED:   # the move decided here: what its ply logged is in the stalled record
                    known = self.stalls.pop(s, None)
                    if known is None or known[:3] != (gid, ply, mv):
                        raise HipError('slot %d: the device resolved game %d ply %d with move %d, the host had decided %r' % (
                            s, gid, ply, mv, known and known[:3]))
                    played = known[3]
                    self.stalls_resolved += 1
                if ply == 0:   # the slot has started this game
                    self.start(s, gid)
                    self.started += 1
                self._expect(s, gid, ply)
                if f & PLAY_RESIGNED:   # the game ends without a move: the plies before it
                    done.append(self.close(s, int(d.winner[i]), True))
                    continue
                self.put_moves(s, ply, mv, pick(self.move_cols, i) if played is None else played, check=False)
                if f & PLAY_ENDED:
                    done.append(self.close(s, int(d.winner[i]), False))
        return done
