"""The learner's replay buffer in device memory (rz_replay_*, csrc/rz_replay.hip; an opt-in extension).

The reference keeps its augmented samples in a host ``deque`` and forms a mini-batch with ``random.sample`` + ``np.array`` + a
host-to-device copy (tools/train_alphazero.py:32,59-79,88-96).  ``DeviceReplay`` holds the POSITIONS of finished games -- two
bitboards, one meta word and a pi row each -- in a ring on the GPU, filled from the games' move lists (``add``), and one kernel
launch writes a mini-batch straight into torch tensors: the four observation planes, the symmetry-transformed pi and z
(``gather`` for given entry indices, ``sample`` for indices drawn on the device).

The contract: ``DeviceReplay(B, C)`` after any sequence of ``add`` calls holds exactly the entries of the trainer's host
``ReplayBuffer(8 * C, B)`` after ``extend_samples(t.training_samples())`` for the same games -- entry 8 j + k is symmetry k (in
``get_equi_data``'s order) of the j-th oldest position held, and ``gather([i])`` equals the float32 casts of the host entry ``i``
bit for bit.

The eight symmetries are TABLES, not arithmetic: ``symmetry_tables`` pushes ``arange(A)`` through the reference's own numpy
expressions and the kernels look the source cell of every output cell up.  There are two tables because the reference permutes
the planes and pi differently (the planes are rotated by +k quarter turns, pi goes through a flipud / rot90 / flipud sandwich:
SURVEY.md D-9): for an odd number of quarter turns the planes turn one way and pi the other.

``sample`` draws WITH replacement -- entry i of update ``step`` is ``replay_index(seed, step, i, len(buffer))``, a counter-based
uniform -- where the reference's ``random.sample`` draws without: a documented deviation; ``gather`` takes whatever indices the
caller drew.

Reanalyse (``ReplayReanalyser``, below): a stored pi row is frozen at the search that played the move -- the network of that time,
under Dirichlet noise, on a reused subtree -- while a position stays in the ring for many rounds.  ``ReplayReanalyser`` searches
stored positions again with the CURRENT network, from a fresh root without noise, and rewrites their pi rows in place; the two
device ends are ``DeviceReplay.position_roots`` (records -> roots of a search engine) and ``DeviceReplay.update_pi`` (visit counts -> pi
rows).  What is refreshed and what is not:

* the new row is the VISIT DISTRIBUTION ``N / sum(N)`` (``reanalysed_pi``), i.e. the reference's pi at temperature 1 up to rounding
  -- not its ``softmax(log(N + 1e-10))`` expression, which is not reproducible on the device: a documented deviation (bounded in
  tests/test_replay_reanalyse_host.py).  A ``pi_temperature`` or temperature schedule of the self-play run is NOT reapplied;
* z is never refreshed: it is the outcome of the game that was played -- what ``targets='value'`` / ``'both'`` refresh is q, the
  search's root value stored beside it ("Value targets from the search", below);
* the fast plies of a playout cap are not in the buffer, so they are not refreshed either.

Connect4 (``DeviceReplay((rows, cols), C, game='connect4')``; build-defined, the reference has no Connect4):

* a stored position is the position before a kept ply, as for Gomoku: two bitboards over CELLS (cell = row * cols + column, row 0
  at the bottom, as in ``Connect4Env``), the meta word and a pi row of ``n_actions = cols`` floats.  The meta word's "last move + 1"
  field holds the last CELL, not the column: plane 2 marks that cell, and a Connect4 root of the search engine takes the last
  stone's cell (``rz_set_roots`` stores it as it comes; the engine's own move step writes the cell there too);
* a game arrives as its COLUMNS; ``add`` refuses a column outside the board or played more often than the board has rows, and the
  device lets the stones drop (csrc/rz_replay_rules.h: ``cell_of_ply``; ``pack_positions`` drops them again in plain Python);
* the augmentation has TWO symmetries: entry ``2 j + k`` is the j-th oldest position held, ``k = 0`` as played and ``k = 1`` its
  left-right mirror -- every plane ``[:, :, ::-1]`` and ``pi[::-1]``; ``len(buffer) = 2 * positions``.  The rotations of a square
  board do not exist here: gravity breaks them.  As for Gomoku the tables come from pushing cell and column numbers through these
  numpy expressions (``symmetry_tables(..., game='connect4')``: ``src_state`` int16 [2][cells], ``src_pi`` int16 [2][cols]);
* ``sample``, ``reanalyse_sample``, ``reanalysed_pi`` and the ticket are exactly Gomoku's: the draw of ``sample`` runs over the
  ``len(buffer)`` entries -- ``replay_index(seed, step, i, 2 * positions)`` --, ``reanalyse_sample`` draws over positions;
* the contract: the entries are those of the trainer's host ``ReplayBuffer(2 * C, (rows, cols), game='connect4')`` for the same games.

Value targets from the search (opt-in, both games: ``DeviceReplay(..., search_values=True)`` or ``enable_search_values()``).  Under the
default selection rule the network steers the search through its value head alone, and z -- the outcome of ONE game played at
T = 1 -- is a noisy target for it; the root's -W / N is an average over the search's evaluations.  With the option a float32 ``q``
[capacity] sits beside the meta words: ``add`` stores ``Trajectory.root_values`` of the kept plies (NaN for a game without them),
and ``set_value_mix(lam)`` makes ``gather`` / ``sample`` write ``zs = mixed_value_targets(z, q, lam)`` = (1 - lam) z + lam q (z where q
is NaN).  ``ReplayReanalyser(..., targets='value' | 'both')`` rewrites q with the current network's search (``update_values``).
The two q are not the same quantity: the self-play q comes from a REUSED subtree searched under Dirichlet noise, the refreshed q from
a FRESH tree without noise at the reanalyser's ``n_playout`` simulations.  z itself is never rewritten.  With the option off nothing
is allocated and every kernel launched is the one it was; at lam = 0 the kernels without q run, so zs is z bit for bit.
"""
import ctypes

import numpy as np

from . import _hip
from ._hip import HipError
from ._rng import MASK as _MASK, mix64 as _mix64, mix64_u64 as _splitmix64

_REPLAY_SALT = np.uint64(0x7265706C61790000)   # ("replay": the sampler's own stream, apart from the move / noise / cap draws)
META_PARITY_BIT, META_Z_SHIFT = 9, 10          # the meta word: bits 0..8 last move + 1 (0: none), bit 9 ply parity, bits 10..11 z + 1


def _rows_cols(board_size, game):
    if game == 'connect4':
        rows, cols = board_size
        return int(rows), int(cols)
    if game != 'gomoku':
        raise ValueError('game %r: gomoku or connect4' % (game, ))
    return int(board_size), int(board_size)


def symmetry_tables(board_size, game='gomoku'):
    """-> (src_state, src_pi), int16 [8][A]: for output cell ``o`` of symmetry ``k`` the source cell of the planes and of pi, i.e.
    ``entry_state[c].flat == state[c].flat[src_state[k]]`` and ``entry_pi == pi[src_pi[k]]``.  Obtained by pushing the cell numbers
    through the numpy expressions the trainer's ReplayBuffer forms an entry with (get_equi_data's, train_alphazero.py:59-79).
    ``game='connect4'``, ``board_size`` (rows, cols): int16 [2][rows * cols] and [2][cols] -- the position as played and its
    left-right mirror, ``planes[:, :, ::-1]`` and ``pi[::-1]``."""
    if game == 'connect4':
        rows, cols = _rows_cols(board_size, game)
        cells, columns = np.arange(rows * cols, dtype=np.int16).reshape(1, rows, cols), np.arange(cols, dtype=np.int16)
        src_state = [np.ascontiguousarray(cells).reshape(-1), np.ascontiguousarray(cells[:, :, ::-1]).reshape(-1)]
        src_pi = [np.ascontiguousarray(columns), np.ascontiguousarray(columns[::-1])]
        return np.stack(src_state).astype(np.int16), np.stack(src_pi).astype(np.int16)
    size = _rows_cols(board_size, game)[0]
    cells = np.arange(size * size, dtype=np.int16)
    states, grids = cells.reshape(1, 1, size, size), cells.reshape(1, size, size)
    src_state, src_pi = [], []
    for k in range(8):
        quarter_turns, mirrored = k // 2 + 1, k % 2 == 1
        turned = np.rot90(states, quarter_turns, axes=(2, 3))
        pi_turned = np.rot90(grids[:, ::-1, :], quarter_turns, axes=(1, 2))
        if mirrored:
            src_state.append(np.ascontiguousarray(turned[:, :, :, ::-1]).reshape(-1))
            src_pi.append(np.ascontiguousarray(pi_turned[:, :, ::-1][:, ::-1, :]).reshape(-1))
        else:
            src_state.append(np.ascontiguousarray(turned).reshape(-1))
            src_pi.append(np.ascontiguousarray(pi_turned[:, ::-1, :]).reshape(-1))
    return np.stack(src_state).astype(np.int16), np.stack(src_pi).astype(np.int16)


def replay_indices(seed, step, n, n_entries):
    """Entries 0 .. n-1 of update ``step``: int64 [n] in [0, n_entries) -- the device's draw (k_replay_sample), the same bits.
    The high half of x * n_entries for the 64-bit x of a splitmix64 chain over (seed, step, i): integer only, every entry's
    probability is floor or ceil of 2^64 / n_entries over 2^64, i.e. within 2^-64 of uniform."""
    n_entries = int(n_entries)
    if not 0 < n_entries < (1 << 31):
        raise ValueError('n_entries %d not in 1 .. 2^31 - 1' % n_entries)
    with np.errstate(over='ignore'):
        x = _splitmix64(np.uint64(int(seed) & _MASK) ^ _REPLAY_SALT)
        x = _splitmix64(x ^ np.uint64(int(step) & _MASK))
        x = _splitmix64(x ^ np.arange(int(n), dtype=np.uint64))
    # mulhi64(x, n_entries) in 64-bit pieces: n_entries < 2^31, so neither product overflows
    m, lo32 = np.uint64(n_entries), np.uint64(0xFFFFFFFF)
    hi = (x >> np.uint64(32)) * m + (((x & lo32) * m) >> np.uint64(32))
    return (hi >> np.uint64(32)).astype(np.int64)


def replay_index(seed, step, i, n_entries):
    """Entry ``i`` of update ``step`` (replay_indices, one value, in Python integers)."""
    n_entries = int(n_entries)
    if n_entries <= 0:
        raise ValueError('n_entries %d must be positive' % n_entries)
    x = _mix64((int(seed) & _MASK) ^ int(_REPLAY_SALT))
    x = _mix64(x ^ (int(step) & _MASK))
    x = _mix64(x ^ (int(i) & _MASK))
    return (x * n_entries) >> 64


_REANALYSE_SALT = 0x617A7265616E616C   # "azreanal" (csrc/rz_replay_rules.h: kReanalyseSalt): a refresh and a mini-batch share no draw
_MAX_REQUEST = 1 << 20                 # positions resolved by one ``position_roots`` launch


def replay_reanalyse_draws(seed, step, n, positions):
    """The positions ``ReplayReanalyser.reanalyse_sample(n, step)`` refreshes in a buffer holding ``positions`` of them, in Python
    integers -- the device's bits (k_replay_positions; csrc/rz_replay_rules.h: reanalyse_position): position i of refresh ``step``
    is the high half of x * positions for the 64-bit x of the splitmix64 chain over (seed ^ "azreanal", step, i).  Uniform over
    POSITIONS (0 = the oldest held), with replacement: the symmetries of a position share one pi row.  -> int64 [n]."""
    positions = int(positions)
    if positions <= 0:
        raise ValueError('draws need at least one position')
    base = _mix64(_mix64((int(seed) & _MASK) ^ _REANALYSE_SALT) ^ (int(step) & _MASK))
    return np.array([(_mix64(base ^ (i & _MASK)) * positions) >> 64 for i in range(int(n))], dtype=np.int64).reshape(-1)


def reanalysed_pi(visits):
    """The pi rows ``DeviceReplay.update_pi`` writes for these visit counts (int [n, A]), in numpy -- the device's bits
    (csrc/rz_replay_rules.h: pi_of_visits): counts below 0 count as 0, the sum is an exact integer, ONE float64 division per entry,
    cast to float32.  -> (pi float32 [n, A], written bool [n]); a row whose counts sum to 0 is not written (its pi here: zeros)."""
    n = np.maximum(np.asarray(visits).astype(np.int64), 0)
    if n.ndim != 2:
        raise ValueError('visits: [n, A]')
    total = n.sum(axis=1)
    written = total > 0
    pi = np.zeros(n.shape, dtype=np.float32)
    pi[written] = (n[written].astype(np.float64) / total[written, None].astype(np.float64)).astype(np.float32)
    return pi, written


def mixed_value_targets(z, q, lam):
    """The value target (1 - lam) z + lam q in numpy -- the arbiter of the device's bits (csrc/rz_replay_rules.h: value_target;
    k_replay_gather / k_replay_sample with ``set_value_mix``) and the host route's own (Trajectory.training_samples(value_mix=)):
    float64, each product rounded before the sum (numpy never fuses them), cast to float32 once; z where q is NaN.  z in {-1, 0, 1}
    (any array), q float32 of the same shape, lam in [0, 1].  -> float32, the shape of z."""
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError('lam %r not in [0, 1]' % lam)
    z32, q32 = np.asarray(z, dtype=np.float32), np.asarray(q, dtype=np.float32)
    if z32.shape != q32.shape:
        raise ValueError('z of shape %r, q of shape %r' % (z32.shape, q32.shape))
    keep = np.float64(1.0 - lam) * z32.astype(np.float64)
    take = np.float64(lam) * q32.astype(np.float64)
    with np.errstate(invalid='ignore'):
        mixed = (keep + take).astype(np.float32)
    return np.where(np.isnan(q32), z32, mixed)


def kept_root_values(trajectories):
    """float32 [kept plies]: ``Trajectory.root_values`` of the plies ``DeviceReplay.add`` keeps (every ply, or the full-budget plies
    under a cap), in ``pack_positions``' order; NaN for the plies of a game without root values -- what ``read(values=True)`` returns."""
    out = []
    for t in trajectories:
        P = len(t.moves)
        keep = np.ones(P, dtype=bool) if t.full is None else np.asarray(t.full[:P], dtype=bool)
        q = np.full(P, np.nan, dtype=np.float32) if getattr(t, 'root_values', None) is None else np.asarray(t.root_values, dtype=np.float32)
        out.append(q[keep])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.float32)


def pack_positions(trajectories, board_size, game='gomoku'):
    """The raw records ``DeviceReplay.add`` stores for these games, formed on the host: (stones uint64 [N][2][4], meta int32 [N],
    pi float32 [N][A]) of the kept plies in order -- what ``DeviceReplay.read`` returns for them.  ``game='connect4'``,
    ``board_size`` (rows, cols): the moves are columns, and every stone drops onto its column's stack here, in plain Python."""
    rows, cols = _rows_cols(board_size, game)
    A = cols if game == 'connect4' else rows * cols
    stones, meta, pis = [], [], []
    for t in trajectories:
        P = len(t.moves)
        cells = list(t.moves)
        if game == 'connect4':
            height = [0] * cols
            for q, column in enumerate(t.moves):
                if not (0 <= column < cols and height[column] < rows):
                    raise ValueError('game %d: ply %d is no legal drop (column %d)' % (t.game_id, q, column))
                cells[q] = height[column] * cols + column
                height[column] += 1
        keep = np.ones(P, dtype=bool) if t.full is None else t.full[:P]
        z = t.z()
        for p in range(P):
            if not keep[p]:
                continue
            rec = [[0] * _hip.BOARD_WORDS, [0] * _hip.BOARD_WORDS]
            for q in range(p):
                m = cells[q]
                rec[(q ^ p) & 1][m >> 6] |= 1 << (m & 63)
            stones.append(rec)
            meta.append((cells[p - 1] + 1 if p else 0) | ((p & 1) << META_PARITY_BIT) | ((int(z[p]) + 1) << META_Z_SHIFT))
            pis.append(np.asarray(t.pis[p], dtype=np.float32))
    return (np.array(stones, dtype=np.uint64).reshape(-1, 2, _hip.BOARD_WORDS), np.array(meta, dtype=np.int32),
            np.array(pis, dtype=np.float32).reshape(-1, A))


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class DeviceReplay(object):
    """A ring of ``capacity_positions`` positions of Gomoku games on ``device``; ``len()`` is 8 x the positions held (entries, like
    the host buffer).  ``game='connect4'``: of Connect4 games, ``board_size`` (rows, cols), ``len()`` 2 x the positions held (the
    module docstring).  ``n_cells``, ``n_actions`` (the width of a pi row) and ``n_symmetries`` are the buffer's three sizes.
    No CPU fallback: HipError without a GPU."""

    def __init__(self, board_size, capacity_positions, device='cuda:0', seed=0, game='gomoku', search_values=False):
        import torch
        self.torch = torch
        self.lib = _hip.load()
        dev = torch.device(device)
        if dev.type != 'cuda' or not torch.cuda.is_available():
            raise HipError('the device replay buffer needs an MI355X (device=%r, cuda available=%s); there is no CPU fallback'
                           % (device, torch.cuda.is_available()))
        self.device = torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())
        self.game, self.capacity = game, int(capacity_positions)
        self.rows, self.cols = _rows_cols(board_size, game)
        self.board_size = (self.rows, self.cols) if game == 'connect4' else self.rows
        self.n_cells = self.rows * self.cols
        self.n_actions = self.cols if game == 'connect4' else self.n_cells
        self.n_symmetries = 2 if game == 'connect4' else 8
        self.seed = int(seed)
        self.step = 0   # the next update ``sample`` draws without a ``step``
        handle = ctypes.c_void_p()
        if game == 'connect4':
            _hip.check(self.lib.rz_replay_create_game(_hip.GAME_CONNECT4, self.rows, self.cols, self.capacity, self.device.index, ctypes.byref(handle)),
                       'rz_replay_create_game')
        else:
            _hip.check(self.lib.rz_replay_create(self.board_size, self.capacity, self.device.index, ctypes.byref(handle)), 'rz_replay_create')
        self.handle = handle
        self.src_state, self.src_pi = symmetry_tables(self.board_size, game)
        if game == 'connect4':
            _hip.check(self.lib.rz_replay_set_tables_game(self.handle, self.n_symmetries, self.n_cells, self.n_actions, _ptr(self.src_state),
                                                          _ptr(self.src_pi), self._stream()), 'rz_replay_set_tables_game')
        else:
            _hip.check(self.lib.rz_replay_set_tables(self.handle, _ptr(self.src_state), _ptr(self.src_pi), self._stream()), 'rz_replay_set_tables')
        self.search_values, self.value_mix = False, 0.0
        if search_values:
            self.enable_search_values()

    def enable_search_values(self):
        """Keep the search's root value q of every position beside its meta word (rz_replay_enable_values: a float32 [capacity]
        array, allocated here, every slot NaN) -- what ``set_value_mix`` mixes into zs and ``update_values`` refreshes.  Only while
        the buffer is empty: ValueError once positions were stored without one."""
        if self.search_values:
            return
        if self.ticket != 0:
            raise ValueError('enable_search_values: the buffer holds positions stored without a value (enable it on an empty buffer)')
        _hip.check(self.lib.rz_replay_enable_values(self.handle, self._stream()), 'rz_replay_enable_values')
        self.search_values = True

    def set_value_mix(self, lam):
        """lam in [0, 1] of the value target ``gather`` / ``sample`` write: zs = mixed_value_targets(z, q, lam).  0 (the default):
        zs is z, written by the kernels that never read q.  ValueError for lam outside [0, 1], and for lam > 0 on a buffer without
        search values."""
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:
            raise ValueError('value mix %r not in [0, 1]' % lam)
        if lam > 0.0 and not self.search_values:
            raise ValueError('value mix %r > 0 on a buffer without search values: DeviceReplay(..., search_values=True)' % lam)
        _hip.check(self.lib.rz_replay_set_value_mix(self.handle, lam), 'rz_replay_set_value_mix')
        self.value_mix = lam

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _state(self):
        count, cursor, cap = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _hip.check(self.lib.rz_replay_state(self.handle, ctypes.byref(count), ctypes.byref(cursor), ctypes.byref(cap)), 'rz_replay_state')
        return count.value, cursor.value, cap.value

    @property
    def positions(self):
        return self._state()[0]

    def __len__(self):
        return self.n_symmetries * self._state()[0]

    def add(self, trajectories):
        """The positions of finished games (selfplay.Trajectory; ``pis`` float64 or float32), in order: every ply, or under a
        playout cap the plies searched with the full budget (``full``, as ``training_samples()`` keeps them -- the other plies
        still place their stones).  One staging copy and one launch for all of them.  A buffer with search values takes
        ``Trajectory.root_values`` of the kept plies along, like the pi rows; a game without them stores NaN, so its target stays z.
        -> positions added."""
        trajectories = list(trajectories)
        A = self.n_actions
        offsets, moves, keeps, winners, rows = [0], [], [], [], []
        for t in trajectories:
            if getattr(t, 'game', 'gomoku') != self.game:
                raise ValueError('the device replay buffer holds %s positions, not %r' % ('Connect4' if self.game == 'connect4' else 'Gomoku', getattr(t, 'game', 'gomoku')))
            if (tuple(t.board_size) if self.game == 'connect4' else t.board_size) != self.board_size:
                raise ValueError('a game of board size %r in a buffer of %r' % (t.board_size, self.board_size))
            P = len(t.moves)
            keep = np.ones(P, dtype=np.uint8) if t.full is None else np.asarray(t.full[:P], dtype=np.uint8)
            if len(keep) != P:
                raise ValueError('game %d: %d budget flags for %d plies' % (t.game_id, len(keep), P))
            if P:
                pis = np.asarray(t.pis)
                if pis.shape != (P, A):
                    raise ValueError('game %d: pi of shape %r, not %r' % (t.game_id, pis.shape, (P, A)))
                rows.append(pis[keep != 0].astype(np.float32, copy=False))
            offsets.append(offsets[-1] + P)
            moves.extend(t.moves)
            keeps.append(keep)
            winners.append(t.winner)
        if not trajectories:
            return 0
        h_off = np.asarray(offsets, dtype=np.int32)
        h_moves = np.asarray(moves, dtype=np.int32)
        h_keep = np.ascontiguousarray(np.concatenate(keeps)) if keeps else np.zeros(0, dtype=np.uint8)
        h_win = np.asarray(winners, dtype=np.int32)
        h_pi = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((0, A), dtype=np.float32)
        if self.search_values:
            for t in trajectories:
                if getattr(t, 'root_values', None) is not None and len(t.root_values) != len(t.moves):
                    raise ValueError('game %d: %d root values for %d plies' % (t.game_id, len(t.root_values), len(t.moves)))
            h_q = np.ascontiguousarray(kept_root_values(trajectories), dtype=np.float32)
            _hip.check(self.lib.rz_replay_add_values(self.handle, len(trajectories), _ptr(h_off), _ptr(h_moves), _ptr(h_keep), _ptr(h_win),
                                                     _ptr(h_pi), _ptr(h_q), self._stream()), 'rz_replay_add_values')
            return int(h_keep.sum())
        _hip.check(self.lib.rz_replay_add(self.handle, len(trajectories), _ptr(h_off), _ptr(h_moves), _ptr(h_keep), _ptr(h_win), _ptr(h_pi),
                                          self._stream()), 'rz_replay_add')
        return int(h_keep.sum())

    def _outputs(self, n):
        t = self.torch
        return (t.empty((n, 4, self.rows, self.cols), dtype=t.float32, device=self.device), t.empty((n, self.n_actions), dtype=t.float32, device=self.device),
                t.empty((n, ), dtype=t.float32, device=self.device))

    def gather(self, indices):
        """Entries ``indices`` (a Python sequence, a numpy array or a device int64 tensor) -> (states float32 [n, 4, B, B], pis
        float32 [n, A], zs float32 [n]) on the device, one launch.  An index outside 0 .. len - 1 raises (host indices before the
        launch; device indices after it, from the kernel's flag -- that entry's rows are not written)."""
        t = self.torch
        if isinstance(indices, t.Tensor):
            if indices.device != self.device or indices.dtype != t.int64:
                raise ValueError('device indices: an int64 tensor on %s' % (self.device, ))
            idx = indices.contiguous().view(-1)
            states, pis, zs = self._outputs(idx.numel())
            st = self._stream()
            _hip.check(self.lib.rz_replay_gather(self.handle, None, idx.data_ptr(), idx.numel(), states.data_ptr(), pis.data_ptr(),
                                                 zs.data_ptr(), st), 'rz_replay_gather')
            flags = ctypes.c_int32()
            _hip.check(self.lib.rz_replay_poll_errors(self.handle, ctypes.byref(flags), st), 'rz_replay_poll_errors')
            if flags.value & _hip.REPLAY_BAD_INDEX:
                raise HipError('rz_replay_gather: an entry index from the device is outside 0 .. %d' % (len(self) - 1))
            return states, pis, zs
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
        states, pis, zs = self._outputs(len(idx))
        _hip.check(self.lib.rz_replay_gather(self.handle, _ptr(idx), None, len(idx), states.data_ptr(), pis.data_ptr(), zs.data_ptr(),
                                             self._stream()), 'rz_replay_gather')
        return states, pis, zs

    def sample(self, n, step=None):
        """``n`` entries drawn on the device, with replacement: entry i is ``replay_index(seed, step, i, len(self))``.  ``step``:
        the update's number; None = an internal counter, advanced by the call."""
        if step is None:
            step, self.step = self.step, self.step + 1
        states, pis, zs = self._outputs(int(n))
        _hip.check(self.lib.rz_replay_sample(self.handle, self.seed & _MASK, int(step) & _MASK, int(n), states.data_ptr(), pis.data_ptr(),
                                             zs.data_ptr(), self._stream()), 'rz_replay_sample')
        return states, pis, zs

    # ------------------------------------------------------------------ Reanalyse: the two device ends
    @property
    def ticket(self):
        """The number of positions EVER stored in this buffer (advanced by ``add``): what ``position_roots`` hands out and ``update_pi``
        compares."""
        out = ctypes.c_int64()
        _hip.check(self.lib.rz_replay_ticket(self.handle, ctypes.byref(out)), 'rz_replay_ticket')
        return out.value

    def position_roots(self, indices=None, n=None, seed=None, step=0, pad_to=1):
        """Positions ``indices`` (0 = the oldest held; a numpy array / sequence, checked before the launch, or a device int64 tensor,
        checked by the kernel) -- or, ``indices`` None, the ``n`` positions ``replay_reanalyse_draws(seed, step, n, self.positions)``
        names, drawn on the device -- as roots of a search engine, ONE launch: -> (where int32 [m] the ring slot of each, -1 for a
        bad device index; stones int64 [m, 2, WORDS] by player; to_move int32 [m]; last_move int32 [m]; ticket).  m = the request
        rounded up to a multiple of ``pad_to``; the rows past the request are padding -- where -1, an empty board -- that
        ``update_pi`` ignores.  A bad device index leaves its row as the padding is and sets the flag ``poll_errors`` reads."""
        t = self.torch
        h_idx = d_idx = None
        if indices is None:
            count = int(n)
        elif isinstance(indices, t.Tensor):
            if indices.device != self.device or indices.dtype != t.int64:
                raise ValueError('device indices: an int64 tensor on %s' % (self.device, ))
            keep = indices.contiguous().view(-1)
            count, d_idx = keep.numel(), ctypes.c_void_p(keep.data_ptr())
        else:
            keep = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
            count, h_idx = len(keep), _ptr(keep)
        pad_to = max(1, int(pad_to))
        m = (count + pad_to - 1) // pad_to * pad_to
        kw = dict(device=self.device)
        where = t.full((m, ), -1, dtype=t.int32, **kw)
        stones = t.zeros((m, 2, _hip.BOARD_WORDS), dtype=t.int64, **kw)
        to_move = t.zeros((m, ), dtype=t.int32, **kw)
        last_move = t.full((m, ), -1, dtype=t.int32, **kw)
        ticket = ctypes.c_int64()
        seed = self.seed if seed is None else int(seed)
        _hip.check(self.lib.rz_replay_positions(self.handle, h_idx, d_idx, seed & _MASK, int(step) & _MASK, count, where.data_ptr(),
                                                stones.data_ptr(), to_move.data_ptr(), last_move.data_ptr(), ctypes.byref(ticket),
                                                self._stream()), 'rz_replay_positions')
        return where, stones, to_move, last_move, ticket.value

    def update_pi(self, where, visits, ticket, n=None):
        """pi row of slot ``where[i]`` := ``reanalysed_pi(visits[i])`` for the first ``n`` rows (default: all of ``where``), one launch:
        where int32 [>= n] and visits int32 [>= n, A], contiguous device tensors.  A row whose where is negative or whose counts sum
        to 0 writes nothing; stones, meta and every other row stay as they are.  ``ticket``: of the ``position_roots`` call that gave
        ``where`` -- HipError, and nothing written, if an ``add`` came in between."""
        t = self.torch
        n = int(where.shape[0]) if n is None else int(n)
        for name, x, cols in (('where', where, None), ('visits', visits, self.n_actions)):
            if (not isinstance(x, t.Tensor) or x.device != self.device or x.dtype != t.int32 or not x.is_contiguous()
                    or x.dim() != (1 if cols is None else 2) or (cols is not None and x.shape[1] != cols)):
                raise ValueError('update_pi: %s must be a contiguous int32 tensor on %s%s' % (name, self.device, '' if cols is None else ', [n, %d]' % cols))
        if n < 0 or n > int(where.shape[0]) or n > int(visits.shape[0]):
            raise ValueError('update_pi: %d rows of %d slots and %d rows of counts' % (n, int(where.shape[0]), int(visits.shape[0])))
        _hip.check(self.lib.rz_replay_update_pi(self.handle, where.data_ptr(), n, visits.data_ptr(), int(ticket), self._stream()), 'rz_replay_update_pi')

    def update_values(self, where, root_values, ticket, n=None):
        """q of slot ``where[i]`` := float32(``root_values[i][0]``) for the first ``n`` rows (default: all of ``where``), one launch:
        where int32 [>= n] and root_values float64 [>= n, 2] (MCTSEngine.root_values_device), contiguous device tensors.  A row whose
        where is negative or whose value is NaN writes nothing; stones, meta, pi and every other row stay as they are.  ``ticket``:
        of the ``position_roots`` call that gave ``where`` -- HipError, and nothing written, if an ``add`` came in between."""
        t = self.torch
        if not self.search_values:
            raise ValueError('update_values: the buffer keeps no search values: DeviceReplay(..., search_values=True)')
        n = int(where.shape[0]) if n is None else int(n)
        for name, x, dtype, cols in (('where', where, t.int32, None), ('root_values', root_values, t.float64, 2)):
            if (not isinstance(x, t.Tensor) or x.device != self.device or x.dtype != dtype or not x.is_contiguous()
                    or x.dim() != (1 if cols is None else 2) or (cols is not None and x.shape[1] != cols)):
                raise ValueError('update_values: %s must be a contiguous %s tensor on %s%s' % (name, str(dtype).split('.')[-1], self.device, '' if cols is None else ', [n, %d]' % cols))
        if n < 0 or n > int(where.shape[0]) or n > int(root_values.shape[0]):
            raise ValueError('update_values: %d rows of %d slots and %d rows of values' % (n, int(where.shape[0]), int(root_values.shape[0])))
        _hip.check(self.lib.rz_replay_update_values(self.handle, where.data_ptr(), n, root_values.data_ptr(), int(ticket), self._stream()), 'rz_replay_update_values')

    def poll_errors(self):
        """The device's flag word (waits for the current stream), cleared by the call."""
        flags = ctypes.c_int32()
        _hip.check(self.lib.rz_replay_poll_errors(self.handle, ctypes.byref(flags), self._stream()), 'rz_replay_poll_errors')
        return flags.value

    def read(self, first=0, n=None, values=False):
        """The raw records of positions ``first`` .. ``first + n - 1`` (oldest = 0), a synchronous copy: (stones uint64 [n][2][4] --
        [0] the mover's, [1] the opponent's --, meta int32 [n], pi float32 [n][A]).  ``values=True`` (a buffer with search values):
        a 4-tuple, with q float32 [n] (NaN: none stored) behind them."""
        n = self.positions - first if n is None else int(n)
        stones = np.zeros((n, 2, _hip.BOARD_WORDS), dtype=np.uint64)
        meta = np.zeros(n, dtype=np.int32)
        pi = np.zeros((n, self.n_actions), dtype=np.float32)
        _hip.check(self.lib.rz_replay_read(self.handle, int(first), n, _ptr(stones), _ptr(meta), _ptr(pi), self._stream()), 'rz_replay_read')
        if values:
            if not self.search_values:
                raise ValueError('read(values=True): the buffer keeps no search values: DeviceReplay(..., search_values=True)')
            q = np.full(n, np.nan, dtype=np.float32)
            _hip.check(self.lib.rz_replay_read_values(self.handle, int(first), n, _ptr(q), self._stream()), 'rz_replay_read_values')
            return stones, meta, pi, q
        return stones, meta, pi

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.rz_replay_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class ReplayReanalyser(object):
    """Fresh searches of positions held by ``replay`` (a DeviceReplay) with ``net_module`` (a PolicyValueNet) as it is now; see the
    module docstring for what a refreshed row holds.

    It owns a private ``MCTSEngine`` of ``slots`` games without noise and a ``HipNetEvaluator`` of ``net_module``, built the way
    ``BatchedEvaluation.for_network`` builds its pair, apart from any self-play engine.  A request is resolved in ONE ``position_roots``
    launch and then worked off in chunks of ``slots`` rows, every chunk on the current torch stream:

      ``set_roots_device(reset_trees=True)`` -> ``set_active`` (all ones; in a short last chunk only its rows) -> ``simulate`` (the
      route the engine picks for the board: k_delta_res at 11 .. 16 rows, the resident k_trunk_split below) -> ``root_visits_device``
      -> ``update_pi`` (and / or ``root_values_device`` -> ``update_values``: ``targets``)

    Nothing waits for the GPU, the error poll for indices given as a device tensor apart; ``check()`` reads the engine's and the
    network's error flags when the caller wants them (it waits).  The trees of a chunk are thrown away by the next chunk's
    ``reset_trees``, so the prior flush ``set_roots_device`` triggers writes priors nobody reads -- matches have the same waste;
    profiles/ab_replay_reanalyse.py measures its share.

    ``update_pi`` carries the ticket ``position_roots`` gave out: if an ``add`` comes between them (from a ``timer`` hook, say) a slot may
    hold another position by then, and the call raises ``HipError`` instead of writing.  Two rows that name one position both write
    it; the search is deterministic, so they write the same bits.  ``timer``: None, or a callable ``timer(label)`` called on the
    stream between the stages ('start', 'positions', then per chunk 'roots', 'search', 'update').

    ``targets``: 'pi' (the default) refreshes the pi rows only; 'value' the stored root values q only (``update_values``, pi and meta
    untouched); 'both' the two from the same search.  'value' / 'both' need a buffer with search values (ValueError here).  A
    refreshed q is the root's -W / N of a FRESH tree without noise at ``n_playout`` simulations; the q self-play stored came from
    a reused subtree under noise.  z is never rewritten."""

    def __init__(self, net_module, replay, n_in_row, n_playout, slots=512, c_puct=5.0, seed=0, targets='pi', **engine_kw):
        from .engine import HipNetEvaluator, MCTSEngine
        if targets not in ('pi', 'value', 'both'):
            raise ValueError('targets %r: pi, value or both' % (targets, ))
        if targets != 'pi' and not replay.search_values:
            raise ValueError('targets=%r needs a buffer with search values: DeviceReplay(..., search_values=True)' % (targets, ))
        self.targets = targets
        self.torch, self.replay = replay.torch, replay
        self.device = replay.device
        self.n_playout, self.slots = int(n_playout), int(slots)
        if self.n_playout < 1 or self.slots < 1:
            raise ValueError('n_playout and slots must be positive')
        self.seed = int(seed)
        self.step = 0   # the next refresh ``reanalyse_sample`` draws without a ``step``
        # (the buffer's game: Connect4's network has rows x cols planes and a policy head of cols columns)
        net_shape = (replay.rows, replay.cols, replay.n_actions) if replay.game == 'connect4' else replay.board_size
        self.engine = MCTSEngine(replay.board_size, n_in_row, n_games=self.slots, n_playout=self.n_playout, c_puct=c_puct,
                                 device=str(self.device), add_noise=False, game=replay.game, **engine_kw)
        self.evaluator = HipNetEvaluator(net_module, net_shape, str(self.device), max_boards=self.slots)
        self._active_rows = None   # rows the engine's active flags select now (None: whatever the engine was created with)
        self.positions_done = 0
        self.sims_done = 0
        self.timer = None

    def close(self):
        eng = getattr(self, 'engine', None)
        if eng is not None:
            eng.close()
            self.engine = None
        hip = getattr(getattr(self, 'evaluator', None), 'hip', None)
        if hip is not None:
            hip.close()
            self.evaluator = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def refresh_weights(self):
        """Re-upload the network weights if the torch module changed (after a learner step)."""
        self.evaluator.refresh_if_changed(content=True)

    def check(self):
        """Raise if a search overflowed its arena or the network left its range (waits for the GPU) -> the engine's statistics."""
        self.evaluator.hip.check_flags()
        return self.engine.check()

    def _mark(self, label):
        if self.timer is not None:
            self.timer(label)

    def _chunk(self, a, rows, where, stones, to_move, last_move, ticket):
        """Rows a .. a + slots - 1 of a resolved request, of which the first ``rows`` are real: search them, write their pi back."""
        eng, G = self.engine, self.slots
        eng.set_roots_device(stones[a:a + G], to_move[a:a + G], last_move[a:a + G], reset_trees=True)
        if self._active_rows != rows:
            eng.set_active((np.arange(G) < rows).astype(np.uint8))
            self._active_rows = rows
        self._mark('roots')
        eng.simulate(self.evaluator, self.n_playout)
        self._mark('search')
        if self.targets != 'value':
            self.replay.update_pi(where[a:a + G], eng.root_visits_device(), ticket, n=rows)
        if self.targets != 'pi':   # (the same stream, no host wait: q := float32 of the fresh root's -W / N)
            self.replay.update_values(where[a:a + G], eng.root_values_device(), ticket, n=rows)
        self._mark('update')
        self.sims_done += self.n_playout * rows

    def _request(self, n, indices=None, step=0):
        """``n`` positions (given, or drawn on the device) resolved in one launch, then chunk by chunk."""
        if n == 0:
            return 0
        self._mark('start')
        where, stones, to_move, last_move, ticket = self.replay.position_roots(indices, n=n, seed=self.seed, step=step, pad_to=self.slots)
        if isinstance(indices, self.torch.Tensor) and self.replay.poll_errors() & _hip.REPLAY_BAD_INDEX:
            raise HipError('reanalyse: a position index from the device is outside 0 .. %d; nothing was refreshed' % (self.replay.positions - 1))
        self._mark('positions')
        for a in range(0, n, self.slots):
            self._chunk(a, min(self.slots, n - a), where, stones, to_move, last_move, ticket)
        self.positions_done += n
        return n

    def reanalyse(self, indices):
        """Refresh positions ``indices`` (0 = the oldest held, as in ``read``): a numpy array / sequence (checked before any launch)
        or a device int64 tensor (checked on the device: HipError, and nothing is refreshed).  -> their number."""
        if isinstance(indices, self.torch.Tensor):
            indices = indices.reshape(-1)
        else:
            indices = np.asarray(indices, dtype=np.int64).reshape(-1)
        n = int(indices.shape[0])
        return sum(self._request(min(_MAX_REQUEST, n - a), indices[a:a + _MAX_REQUEST]) for a in range(0, n, _MAX_REQUEST))

    def reanalyse_sample(self, n, step=None):
        """Refresh the ``n`` positions ``replay_reanalyse_draws(seed, step, n, replay.positions)`` names, drawn on the device (uniform
        over the positions held, with replacement).  ``step``: the refresh's number; None = an internal counter, advanced by the
        call.  -> n."""
        n = int(n)
        if not 0 <= n <= (1 << 24):
            raise ValueError('n outside 0 .. 2^24')
        if step is None:
            step, self.step = self.step, self.step + 1
        return self._request(n, step=step)

    def reanalyse_all(self):
        """Refresh every position held.  -> their number."""
        return self.reanalyse(np.arange(self.replay.positions, dtype=np.int64))
