"""Continuous self-play without a GPU: the ring's index and room rules (rlzero_amd/csrc/rz_play.h: queue_slot, queue_room) through a
stand-alone driver, plain and under the address and undefined-behaviour sanitizers; the reader on scripted log rows whose settings
change mid-game (rows verified under their own epoch, Trajectory.epochs, the calibration rule across epochs); the collect loop
driven by a stub lane (what is enqueued, read and pushed depends on the log's content only, the unread look-ahead is constant at
return, no slot waits for an id); the trainer's refusals; and the ranks' payload, which does not know of epochs."""
import contextlib
import importlib.util
import os
import types

import numpy as np
import pytest

from conftest import REPO
import host_driver
from oracle.mcts_ref import inverse_cdf_choice, softmax
from rlzero_amd import playlog
from rlzero_amd._hip import PLAY_ENDED, PLAY_NO_RESIGN, PLAY_RECORD_WORDS, PLAY_RUNNING, PLAY_SEARCHED, HipError
from rlzero_amd.selfplay import (BatchedSelfPlay, Epoch, SelfPlayReader, Trajectory, cap_uniform, move_uniform, pack_trajectories, payload_of,
                                 resign_uniform, stream_lookahead, stream_topup)
from test_playlog_host import CALIB, FRAC, N_PLAYOUT, PLAIN, PLAYED, SEED, Cfg, Game, Writer, _bits

W0 = PLAY_RECORD_WORDS
INT32_MAX = 2 ** 31 - 1

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rz_play.h"

namespace ry = rzplay;

template <typename T>
static std::vector<T> load(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (bytes && fread(v.data(), 1, (size_t)bytes, f) != (size_t)bytes) exit(2);
    fclose(f);
    return v;
}
template <typename T>
static void store(const char *path, const std::vector<T> &v) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror(path); exit(2); }
    fclose(f);
}

// rules in.i32 [N][3] (head, valid, capacity) -> out.i32 [N][3]: queue_slot(head), queue_slot(valid), queue_room
static int rules(char **a) {
    const std::vector<int32_t> in = load<int32_t>(a[0]);
    std::vector<int32_t> out(in.size());
    for (size_t i = 0; i + 2 < in.size(); i += 3) {
        out[i] = ry::queue_slot(in[i], in[i + 2]);
        out[i + 1] = ry::queue_slot(in[i + 1], in[i + 2]);
        out[i + 2] = ry::queue_room(in[i], in[i + 1], in[i + 2]);
    }
    store(a[1], out);
    return 0;
}

// ring capacity start ops.i32 [N][2] (0 = push n ids, 1 = claim up to n) -> out.i64: per push 1 / 0 (taken / refused), per claim the
// ids claimed.  The ring as k_play_push and k_play_apply keep it: a heap array of exactly `capacity` entries, head = valid = start.
static int ring(char **a) {
    const int cap = atoi(a[0]);
    int head = atoi(a[1]), valid = head;
    const std::vector<int32_t> ops = load<int32_t>(a[2]);
    std::vector<int64_t> ids((size_t)cap, -1), out;
    int64_t next = 1000;
    for (size_t i = 0; i + 1 < ops.size(); i += 2) {
        const int n = ops[i + 1];
        if (ops[i] == 0) {
            const bool ok = n <= ry::queue_room(head, valid, cap);
            for (int k = 0; ok && k < n; ++k) ids[(size_t)ry::queue_slot(valid + k, cap)] = next + k;
            if (ok) valid += n, next += n;
            out.push_back(ok ? 1 : 0);
        } else {
            for (int k = 0; k < n && head < valid; ++k, ++head) out.push_back(ids[(size_t)ry::queue_slot(head, cap)]);
        }
    }
    out.push_back(head);
    out.push_back(valid);
    store(a[3], out);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 3;
    const std::string what = argv[1];
    if (what == "rules" && argc == 4) return rules(argv + 2);
    if (what == "ring" && argc == 6) return ring(argv + 2);
    return 3;
}
'''


drv = host_driver.fixture('queue', '#include <string>\n' + DRIVER)


def room(head, valid, cap):
    """queue_room restated: free entries of the ring, and never past the int32 range of the counts."""
    if cap <= 0 or head < 0 or valid < head:
        return 0
    return max(0, min(cap - (valid - head), INT32_MAX - valid))


def test_queue_rules(drv):
    """Wrap, a full ring, the linear queue and counts at the int32 limit: no overflow (the sanitized build would stop), the restated
    values."""
    rows = [(0, 0, 0), (5, 9, 0), (0, 0, 7), (6, 7, 7), (7, 7, 7), (7, 14, 7), (8, 14, 7), (13, 20, 7), (0, 18, 18), (17, 18, 18),
            (3, 2, 7), (-1, 4, 7), (0, 4, -3), (INT32_MAX, INT32_MAX, 7), (INT32_MAX - 3, INT32_MAX - 1, 7), (INT32_MAX - 9, INT32_MAX - 8, 5),
            (0, INT32_MAX, INT32_MAX), (INT32_MAX - 1, INT32_MAX, 1), (INT32_MAX - 4, INT32_MAX - 4, INT32_MAX)]
    rng = np.random.RandomState(0)
    for _ in range(300):
        cap = int(rng.randint(1, 40))
        head = int(rng.randint(0, INT32_MAX - 50))
        rows.append((head, head + int(rng.randint(0, cap + 1)), cap))
    got = drv.run('rules', [], [np.array(rows, dtype=np.int32)], [np.int32])[0].reshape(-1, 3)
    for (head, valid, cap), (s_head, s_valid, r) in zip(rows, got.tolist()):
        if head >= 0:   # (a negative count is no queue's: only queue_room answers for it)
            assert s_head == (head % cap if cap > 0 else head) and s_valid == (valid % cap if cap > 0 else valid), (head, valid, cap)
        assert r == room(head, valid, cap), (head, valid, cap)
    by = dict((row, g[2]) for row, g in zip(rows, got.tolist()))
    assert by[7, 14, 7] == 0 and by[8, 14, 7] == 1 and by[0, 0, 7] == 7            # a full ring, one claim later, an empty one
    assert by[INT32_MAX, INT32_MAX, 7] == 0 and by[INT32_MAX - 3, INT32_MAX - 1, 7] == 1   # the counts' last values


@pytest.mark.parametrize('cap,start', [(1, 0), (5, 0), (18, 3), (7, INT32_MAX - 40)])
def test_a_ring_played_through(drv, cap, start):
    """Pushes and claims in a random order through a ring of exactly ``cap`` entries: ids come out in the order they went in, a push
    beyond the room is refused whole, and at the int32 limit the ring refuses instead of wrapping its counts."""
    rng = np.random.RandomState(cap)
    ops = np.stack([rng.randint(0, 2, size=400), rng.randint(0, cap + 2, size=400)], axis=1).astype(np.int32)
    got = drv.run('ring', [cap, start], [ops], [np.int64])[0].tolist()
    head = valid = start
    queue, nxt, want = [], 1000, []
    for op, n in ops.tolist():
        if op == 0:
            ok = n <= room(head, valid, cap)
            if ok:
                queue.extend(range(nxt, nxt + n))
                valid, nxt = valid + n, nxt + n
            want.append(1 if ok else 0)
        else:
            for _ in range(min(n, len(queue))):
                want.append(queue.pop(0))
                head += 1
    assert got == want + [head, valid]
    assert valid == INT32_MAX if start > INT32_MAX // 2 else valid > 10 * cap   # (the last case runs into the limit and stays there)


# ----------------------------------------------------------------------------------------------- the reader across epochs
def setting(temps, cap, threshold, frac=FRAC, pi_T=None, first_row=0):
    return Epoch(first_row, np.asarray(temps, dtype=np.float64), pi_T, cap, threshold, frac)


EPOCHS = [setting([1.0, 1.0, 1e-3], (7, 0.5), -0.8), setting([1e-3, 1.0], (5, 0.9), -0.2, first_row=3),
          setting([0.5], (9, 0.2), -0.6, first_row=7)]
SCRIPT = [(PLAYED[0], 3, None, [1], True), (CALIB[0], 5, 0, [], False), (PLAYED[1], 4, 1, [0], False), (CALIB[1], 2, -1, [], False),
          (PLAYED[2], 6, 0, [2], False), (PLAYED[3], 0, None, [], True)]   # game id, plies, winner, stalled plies, resigns
BASE = Cfg(temps=[1.0], resign=(-0.8, FRAC), cap=(7, 0.5))   # (what the scripted device writes flags for: a rule and a cap, in every epoch)


def scripted(epoch_of, A=9):
    """The games of SCRIPT, every search under the settings of the epoch that ``epoch_of(game id, ply)`` names: counts, the
    reference's move and pi at that epoch's T, the budget flag under its cap, a statistic that its threshold -- and not every
    other -- explains."""
    rng, games = np.random.RandomState(5), []
    for gid, n_plies, winner, stalls, resign in SCRIPT:
        g = types.SimpleNamespace(gid=gid, winner=winner, stalls=set(stalls), resigned=resign, calib=gid in CALIB, counts=[], moves=[], pis=[],
                                  stats=[], full=[], would=[], epochs=[])
        taken = np.zeros(A, dtype=bool)
        for ply in range(n_plies + (1 if resign else 0)):
            e = epoch_of(gid, ply)
            S = EPOCHS[e]
            legal = np.nonzero(~taken)[0]
            n = rng.multinomial(N_PLAYOUT - 1, rng.dirichlet(np.ones(len(legal))))
            counts = np.full(A, -1, dtype=np.int32)
            counts[legal] = n
            g.counts.append(counts)
            resigning = resign and ply == n_plies
            g.would.append(False)
            g.stats.append(np.float32(S.resign_threshold + (-0.05 if resigning else 0.05)))
            g.full.append(bool(cap_uniform(SEED, gid, ply) < S.playout_cap[1]))
            g.epochs.append(e)
            if resigning:
                g.winner = 1 - ply % 2
                break
            T = float(S.temperature_schedule[min(ply, len(S.temperature_schedule) - 1)])
            probs = softmax(1.0 / T * np.log(n + 1e-10))
            g.moves.append(inverse_cdf_choice([float(move_uniform(SEED, gid, ply))])(legal, probs))
            pi = np.zeros(A)
            pi[legal] = probs
            g.pis.append(pi)
            taken[g.moves[-1]] = True
        games.append(g)
    return games


def reader_for(resolve, epochs=EPOCHS):
    r = SelfPlayReader(2, 9, 9, N_PLAYOUT, (3, 3, 'gomoku'), resolve, temperature=1.0, seed=SEED)
    r.epochs = list(epochs)
    (_, r.temperature_schedule, r.pi_temperature, r.playout_cap, r.resign_threshold, r.resign_disabled_frac) = epochs[-1]   # (what is current)
    return r


def row_epoch(row):
    return int(np.searchsorted([e.first_row for e in EPOCHS], row, side='right') - 1)


def record_epochs(games):
    w = Writer(BASE, games, 2, delay=0)
    reader = reader_for(w.resolve)
    out = []
    while w.busy():
        out.extend(reader.read_rows(w.step()[None], row_epochs=[row_epoch(len(w.rows) - 1)])[0])
    return np.stack(w.rows), out, reader


@pytest.fixture(scope='module')
def epoch_log():
    """The layout first -- which row searches which (game, ply) depends on the script's lengths and stalls only --, then the games
    under the epochs of their rows, written and read row by row."""
    layout, _, _ = record_epochs(scripted(lambda gid, ply: 0)) if False else (None, None, None)
    w = Writer(BASE, scripted(lambda gid, ply: 0), 2, delay=0)
    plain = SelfPlayReader(2, 9, 9, N_PLAYOUT, (3, 3, 'gomoku'), w.resolve, temperature=1.0, seed=SEED)
    plain.playout_cap, plain.resign_threshold, plain.resign_disabled_frac = EPOCHS[0].playout_cap, EPOCHS[0].resign_threshold, FRAC
    plain.temperature_schedule = EPOCHS[0].temperature_schedule
    while w.busy():
        plain.read_rows(w.step()[None])
    rows = np.stack(w.rows)
    searched = {}
    for r, s in zip(*np.nonzero((rows[..., 4] & PLAY_SEARCHED) != 0)):
        d = playlog.decode(rows[r, s])
        searched[int(d.game), int(d.ply)] = int(r)
    games = scripted(lambda gid, ply: row_epoch(searched[gid, ply]))
    log, out, reader = record_epochs(games)
    assert log.shape == rows.shape
    return games, log, out, reader


def check_games(out, games):
    by_id = dict((g.gid, g) for g in games)
    assert sorted(t.game_id for t in out) == sorted(by_id)
    for t in out:
        g = by_id[t.game_id]
        assert t.moves == g.moves and t.winner == g.winner, t.game_id
        if g.moves:
            assert np.array_equal(t.pis, np.array(g.pis)), t.game_id
        assert t.full.tolist() == g.full and t.resign_stats.tolist() == [float(s) for s in g.stats]
        assert t.epochs.dtype == np.int32 and t.epochs.tolist() == g.epochs[:len(g.moves)] and (np.diff(t.epochs) >= 0).all()
        assert (t.resigned, t.no_resign) == (g.resigned, g.calib)


def test_rows_are_verified_under_their_own_epoch(epoch_log):
    """A threshold, a cap and a schedule that change mid-game: every game comes back as scripted, each ply with the epoch of its
    search -- a stalled ply with that of its searched record, though its move arrives rows later --, and games span epochs."""
    games, log, out, reader = epoch_log
    check_games(out, games)
    assert sum(len(set(g.epochs)) > 1 for g in games) >= 3 and set(e for g in games for e in g.epochs) == {0, 1, 2}
    stalled = [g for g in games if g.stalls]
    assert stalled and reader.stalls_resolved == sum(len(g.stalls) for g in games)
    assert reader.sims_done == sum(N_PLAYOUT if f else EPOCHS[e].playout_cap[0] for g in games for f, e in zip(g.full, g.epochs))


def test_the_batching_does_not_matter(epoch_log):
    games, log, _, _ = epoch_log
    calls = []
    reader = reader_for(lambda s, m: calls.append((s, m)))
    eps = [row_epoch(r) for r in range(len(log))]
    out = []
    for at in range(0, len(log), 4):
        out.extend(reader.read_rows(log[at:at + 4], row_epochs=eps[at:at + 4])[0])
    check_games(out, games)


@pytest.mark.parametrize('wrong', [0, 1, 2])
def test_the_current_settings_alone_do_not_explain_the_log(epoch_log, wrong):
    """Read under ONE epoch's settings -- what the reader did before it knew of epochs -- the log is refused."""
    _, log, _, _ = epoch_log
    reader = reader_for(lambda s, m: None)
    with pytest.raises(HipError):
        reader.read_rows(log, row_epochs=[wrong] * len(log))


def hand_row(gid, ply, move, flags, stat, winner=-1, A=9):
    """One slot's record with a single visited child (the draw is that child whatever the uniform)."""
    rec = np.zeros((1, 1, W0 + A), dtype=np.int32)
    rec[0, 0, 0:2] = np.array([gid], dtype=np.int64).view(np.int32)
    rec[0, 0, 2], rec[0, 0, 3], rec[0, 0, 5], rec[0, 0, 7] = ply, move, N_PLAYOUT, _bits(stat)
    rec[0, 0, 4] = flags | ((winner + 1) << 16 if flags & PLAY_ENDED else 0)
    rec[0, 0, W0:] = 0
    rec[0, 0, W0 + move] = N_PLAYOUT - 1
    return rec


@pytest.mark.parametrize('fracs,calibration', [((1.0, 1.0), True), ((1.0, 0.0), False), ((0.0, 1.0), False)])
def test_a_calibration_game_is_one_in_every_epoch_it_spans(fracs, calibration):
    """Two plies, two epochs that differ in the share of calibration games: no_resign and fp_margin only if both made it one."""
    epochs = [setting([1.0], None, -0.5, frac=fracs[0]), setting([1.0], None, -0.5, frac=fracs[1], first_row=1)]
    reader = SelfPlayReader(1, 9, 9, N_PLAYOUT, (3, 3, 'gomoku'), lambda s, m: None, temperature=1.0, seed=SEED)
    reader.epochs = epochs
    reader.resign_threshold, reader.resign_disabled_frac = -0.5, fracs[1]
    gid = 4
    assert 0.0 < resign_uniform(SEED, gid) < 1.0
    base = PLAY_RUNNING | PLAY_SEARCHED
    rows = np.concatenate([hand_row(gid, 0, 3, base | (PLAY_NO_RESIGN if fracs[0] else 0), 0.25),
                           hand_row(gid, 1, 5, base | PLAY_ENDED | (PLAY_NO_RESIGN if fracs[1] else 0), -0.125, winner=0)])
    done, _ = reader.read_rows(rows, row_epochs=[0, 1])
    (t, ) = done
    assert t.moves == [3, 5] and t.epochs.tolist() == [0, 1] and t.no_resign == calibration and not t.resigned
    assert t.fp_margin == np.float32(0.25) if calibration else np.isnan(t.fp_margin)   # (the winner, player 0, moved ply 0)
    assert t.resign_stats.tolist() == [0.25, -0.125]


def test_the_payload_does_not_know_of_epochs():
    """pack_trajectories / payload_of: the same bytes with and without ``epochs``."""
    rng = np.random.RandomState(3)
    kw = dict(resigned=False, no_resign=True, resign_stats=np.float32([0.1, -0.2, 0.3]), fp_margin=-0.2, full=[True, False, True],
              root_values=np.float32([0.0, 0.5, -0.5]))
    pis = rng.dirichlet(np.ones(9), size=3)
    plain = [Trajectory(7, 3, 3, [4, 0, 8], pis, 1, **kw), Trajectory(9, 3, 3, [1], pis[:1], -1)]
    streamed = [Trajectory(7, 3, 3, [4, 0, 8], pis, 1, epochs=[0, 0, 2], **kw), Trajectory(9, 3, 3, [1], pis[:1], -1, epochs=[2])]
    assert plain[0].epochs is None and streamed[0].epochs.dtype == np.int32 and streamed[0].epochs.tolist() == [0, 0, 2]
    for a, b in zip(pack_trajectories(plain, 9), pack_trajectories(streamed, 9)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for dt in (np.float32, np.float64):
        assert payload_of(plain, 9, dt)[0].tobytes() == payload_of(streamed, 9, dt)[0].tobytes()
    with pytest.raises(ValueError, match='epochs'):
        Trajectory(7, 3, 3, [4, 0, 8], pis, 1, epochs=[0, 0])


# ----------------------------------------------------------------------------------------------- the collect loop on a stub lane
class StubEvent(object):
    def __init__(self, trace, rows):
        self.trace, self.rows = trace, rows

    def synchronize(self):
        self.trace.append(('wait', tuple(self.rows)))

    def query(self):   # (a stream never asks whether rows happen to be ready)
        raise AssertionError('a stream reads behind synchronize only')


class StubEngine(object):
    """The device of one lane: test_playlog_host's Writer behind the engine's calls, a ring of log rows, a queue that holds the
    pushed ids only.  Every call is noted in ``trace``."""

    def __init__(self, games, G, ring, trace):
        self.pending, self.trace, self.play_match_on = list(games), trace, False
        self.writer = Writer(PLAIN, [], G, delay=0)
        self.log = np.zeros((ring, G, W0 + PLAIN.A), dtype=np.int32)
        self.steps = 0

    def play_queue_push(self, first, count):
        self.trace.append(('push', int(first), int(count)))
        for _ in range(count):
            assert self.pending[0].gid == first
            self.writer.queue.append(self.pending.pop(0))
            first += 1

    def play_move_replay(self, graph):
        row = self.steps % len(self.log)
        self.log[row] = self.writer.step()
        self.steps += 1
        self.trace.append(('move', row))
        return row

    def play_resolve(self, slot, move):
        self.trace.append(('resolve', slot, move))
        self.writer.resolve(slot, move)


class StubPlay(BatchedSelfPlay):
    """BatchedSelfPlay's stream methods over a StubEngine: the state stream_start leaves, without a device."""

    def __init__(self, games, G=2, copy_every=2, depth=2):
        self.trace = []
        SelfPlayReader.__init__(self, G, PLAIN.A, PLAIN.room, N_PLAYOUT, PLAIN.geometry, self._resolve, temperature=1.0, seed=SEED)
        eng = StubEngine(games, G, copy_every * (depth + 2) + 2, self.trace)
        lane = types.SimpleNamespace(eng=eng, slots=slice(0, G), move_graph=object(), uncopied=[], inflight=[], last_running=-1,
                                     host_np=eng.log, values_np=None)
        self.lanes, self._copy_every, self._depth = [lane], copy_every, depth
        self._streaming, self._stream_first, self._stream_pushed = True, games[0].gid, 0
        self._stream_low, self._stream_done_ids = games[0].gid, set()
        self._stream_rounds = self._stream_batches = self._stream_returned = 0
        self._stream_topup, self._chain_ev = stream_topup(G, copy_every, depth), None
        self.epochs = [self.settings(first_row=0)]
        self._stream_push()
        for _ in range(stream_lookahead(copy_every, depth)):
            self._stream_round()

    def _on(self, lane):
        return contextlib.nullcontext()

    def _read_back(self, lane):
        rows, lane.uncopied = lane.uncopied, []
        lane.inflight.append((rows, StubEvent(self.trace, rows)))


def stub_games(n, seed):
    rng = np.random.RandomState(seed)
    return [Game(PLAIN, rng, gid, int(rng.randint(1, 7)), int(rng.randint(-1, 2)), stalls=[0] if gid % 5 == 2 else [1] if gid % 7 == 3 else [])
            for gid in range(100, 100 + n)]


@pytest.mark.parametrize('copy_every,depth', [(1, 1), (2, 2), (3, 1)])
def test_the_collect_loop_on_a_stub_lane(copy_every, depth):
    """Games of one to six plies, stalls among them, through two slots: every collect returns at least n games in the order of the
    log's rows with the look-ahead unread, no slot ever waits for an id although the ring holds the least the top-up allows, the
    ring never holds more than its capacity -- and the calls that reach the device (moves, waits, pushes, resolved moves) are the
    same sequence on a second run: they depend on the log's content only."""
    traces = []
    for _ in range(2):
        games = stub_games(90, seed=copy_every * 10 + depth)
        sp = StubPlay(games, copy_every=copy_every, depth=depth)
        ahead, out = stream_lookahead(copy_every, depth), []
        for n in (1, 4, 2, 7, 3):
            got = sp.stream_collect(n)
            assert len(got) >= n
            lane = sp.lanes[0]
            assert sum(len(rows) for rows, _ in lane.inflight) + len(lane.uncopied) == ahead == sp._stream_rounds - copy_every * sp._stream_batches
            out.extend(got)
            claimed = 90 - len(lane.eng.pending) - len(lane.eng.writer.queue)
            assert sp._stream_pushed - claimed <= sp._stream_topup   # (the ring's capacity is never exceeded)
        by_id = dict((g.gid, g) for g in games)
        for t in out:
            assert t.moves == by_id[t.game_id].moves and np.array_equal(t.pis, np.array(by_id[t.game_id].pis)) and not t.epochs.any()
        assert sp.stalls_resolved > 0 and len(set(t.game_id for t in out)) == len(out)
        traces.append(list(sp.trace))
    assert traces[0] == traces[1] and any(c[0] == 'resolve' for c in traces[0]) and sum(c[0] == 'push' for c in traces[0]) > 3


def test_an_idle_slot_in_a_stream_is_an_error():
    sp = StubPlay(stub_games(30, seed=1), copy_every=1, depth=1)
    sp.lanes[0].eng.play_queue_push = lambda first, count: None   # (a top-up that never arrives)
    with pytest.raises(HipError, match='waited for a game id'):
        sp.stream_collect(20)


# ----------------------------------------------------------------------------------------------- the trainer
def _trainer():
    spec = importlib.util.spec_from_file_location('train_alphazero_stream_host', os.path.join(REPO, 'tools', 'train_alphazero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_trainer_refuses(monkeypatch):
    mod = _trainer()
    monkeypatch.delenv('RZ_TRAIN_HOST_MOVES', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(ValueError, match='selfplay_games_in_flight must be > 0'):
        mod.TrainPipeline(continuous_selfplay=True)
    with pytest.raises(ValueError, match='games-in-flight'):
        mod.main(['--continuous-selfplay'])
    with pytest.raises(ValueError, match='one rank'):
        mod.main(['--continuous-selfplay', '--games-in-flight', '4', '--gpus', '2'])
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='one rank'):
        mod.main(['--continuous-selfplay', '--games-in-flight', '4'])
    monkeypatch.delenv('WORLD_SIZE')
    monkeypatch.setenv('RZ_TRAIN_HOST_MOVES', '1')
    with pytest.raises(ValueError, match='RZ_TRAIN_HOST_MOVES'):
        mod.main(['--continuous-selfplay', '--games-in-flight', '4'])
    with pytest.raises(ValueError, match='RZ_TRAIN_HOST_MOVES'):
        mod.TrainPipeline(selfplay_games_in_flight=4, continuous_selfplay=True)
    assert not hasattr(mod.parse_args(['--games-in-flight', '4']), 'continuous_selfplay')   # (absent without the flag: the parsed defaults are the parent's)
    assert mod.parse_args(['--games-in-flight', '4', '--continuous-selfplay']).continuous_selfplay is True
