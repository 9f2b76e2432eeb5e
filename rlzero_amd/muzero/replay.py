"""The MuZero learner's replay buffer in device memory (rz_mz_replay_*, csrc/rz_mz_replay.hip; an opt-in extension).

``selfplay.ReplayBuffer.sample`` forms a mini-batch in CPython -- a loop over the K + 1 unroll steps of every entry and, inside it,
a loop over ``td_steps`` rewards -- and the learner pushes six numpy arrays to the GPU.  ``MuZeroDeviceReplay`` holds the finished
episodes ON the GPU, in fixed-stride slots (slot e: up to ``max_episode_steps`` steps; obs / action / reward / root value / policy
as separate arrays) that form a ring over episodes, and one launch writes a mini-batch straight into torch tensors (``gather``
for given draws, ``sample`` for draws made on the device).  Episodes arrive as the packed records of ``play_cartpole``: from the
host (``add``) or straight from a launch's device arena (``ingest``).

The contract: after any sequence of ``add`` / ``ingest`` calls the buffer holds exactly the episodes of the host
``ReplayBuffer(capacity_episodes, ...)`` after ``add`` of the same episodes in the same order -- episode j is the j-th oldest,
empty episodes are skipped, the oldest is dropped when the buffer is full -- and ``gather(ep_idx, pos, filler)`` returns the six
arrays of ``ReplayBuffer.sample`` for those draws bit for bit.  The value targets are exact because the discounts are a TABLE:
``disc[i] = discount ** i`` as CPython evaluates it (``_value_target``'s expression), uploaded at creation; the device multiplies
and adds in fp64 in the host's order and casts to float32 once (csrc/rz_mz_target.h).

``sample`` draws episode, position and filler actions from a counter-based stream (``mz_replay_draws``: the same bits on the
host) -- the episode uniform over the episodes held, the position uniform over its length, the host buffer's distribution, but
not the host buffer's ``RandomState`` sequence.

Prioritized replay (``prioritized=True`` or ``enable_priorities()``; arXiv:1911.08265v2 appendix G with alpha = 1) draws a step
with probability w / sum(w), w the fixed-point integer of |root value - n-step return| of that step
(``mz_priority_weights``).  The weights and their prefix sums live on the device beside the store, so a Reanalyse that
rewrites root values moves the priorities with no read-back; ``sample_prioritized`` returns the mini-batch and the
importance weights (1 / (N P)) ** beta.  Integer sums are exact in any order: ``mz_prioritized_draws`` restates the device's
draws bit for bit.

``value_transform=True`` (rz_mz_replay_set_value_transform; for a ``MuZeroNet(value_transform=True)``): the launch that forms a
mini-batch -- ``gather``, ``sample`` and the gather of ``sample_prioritized`` -- writes ``tv = float32(h(z))`` and ``tr =
float32(h(u))``, z the fp64 n-step return as formed without it and u the stored reward (csrc/rz_mz_value.h), bit for bit what
``ReplayBuffer(value_transform=True).sample`` forms; rows past the episode's end stay 0.  The store stays raw, and the priorities
stay |root value - n-step return| in RAW units: ``priorities()`` is the same with and without the flag.
"""
import bisect
import ctypes

import numpy as np

from .. import _hip
from .._hip import HipError
from .._rng import MASK as _MASK, mix64 as _sm

_SAMPLE_SALT = 0x6D7A7265706C6179   # "mzreplay" (csrc/rz_mz_target.h: kSampleSalt)
_PRIO_SALT = 0x6D7A7072696F7269     # "mzpriori" (csrc/rz_mz_target.h: kPrioSalt)
MAX_OBS, MAX_ACTIONS, MAX_UNROLL, MAX_TD = 16, 8, 16, 64
FINAL_POLICY = 1                    # rz_mz_replay_add's flag: the visit columns of the episode's rows hold the float32 policy


def mz_replay_draws(seed, step, n, lengths, K, A):
    """The draws of ``sample(n, step)`` over episodes of these ``lengths`` (oldest first), in Python integers -- the device's
    bits (k_mzr_sample): counter c = i (K + 2) + j of update ``step`` gives the high half of x * m for the 64-bit x of the
    splitmix64 chain over (seed, step, c); j = 0 the episode (m = episodes held), j = 1 the position (m = its length),
    j = 2 + k the filler action of actions[i, k] (m = A).  -> (ep_idx int64 [n], pos int64 [n], filler int64 [n, K])."""
    lengths = [int(v) for v in lengths]
    if not lengths or min(lengths) <= 0:
        raise ValueError('draws need at least one episode, none of them empty')
    K, A = int(K), int(A)
    base = _sm(_sm((int(seed) & _MASK) ^ _SAMPLE_SALT) ^ (int(step) & _MASK))

    def draw(c, m):
        return (_sm(base ^ (c & _MASK)) * m) >> 64
    ep = np.zeros(n, dtype=np.int64)
    pos = np.zeros(n, dtype=np.int64)
    filler = np.zeros((n, K), dtype=np.int64)
    for i in range(int(n)):
        c = i * (K + 2)
        ep[i] = draw(c, len(lengths))
        pos[i] = draw(c + 1, lengths[ep[i]])
        for k in range(K):
            filler[i, k] = draw(c + 2 + k, A)
    return ep, pos, filler


def mz_priority_weights(rewards, root_values, td_steps, disc):
    """The integer priorities of one episode's steps (k_mzr_prio, csrc/rz_mz_target.h: priority_of, priority_weight), int64
    [len]: p = |root_values[t] - z_t| with z_t the n-step return as ``ReplayBuffer._value_target`` evaluates it, then
    w = max(1, int(p * 65536)) below p = 65536, 2 ** 32 from there on, 1 for a NaN.  ``disc``: the discount, or the table
    ``[discount ** i for i in range(td_steps + 1)]``."""
    rewards, root_values = np.asarray(rewards, dtype=np.float64), np.asarray(root_values, dtype=np.float64)
    td = int(td_steps)
    if np.ndim(disc) == 0:
        disc = [float(disc) ** i for i in range(td + 1)]
    disc = np.asarray(disc, dtype=np.float64)
    n = len(rewards)
    out = np.zeros(n, dtype=np.int64)
    for t in range(n):
        boot = t + td
        value = root_values[boot] * disc[td] if boot < n else 0.0
        for i, r in enumerate(rewards[t:boot]):
            value += r * disc[i]
        p = abs(float(root_values[t]) - float(value))
        if not p > 0.0:        # zero or a NaN
            out[t] = 1
        elif p >= 65536.0:
            out[t] = 1 << 32
        else:
            out[t] = max(1, int(p * 65536.0))
    return out


def mz_prioritized_draws(seed, step, n, weights_per_episode, K, A, targets=None):
    """The draws of ``prioritized_draws(n, step)`` over episodes with these integer step weights (oldest first), in Python
    integers -- the device's bits (k_mzr_draw_prio): entry i takes ONE target g = (x * total) >> 64 for the 64-bit x of the
    splitmix64 chain over (seed ^ "mzpriori", step, c = i (K + 2)), or ``targets[i]``; the episode is the first whose
    inclusive prefix of episode masses exceeds g, the position the first whose inclusive prefix inside the episode exceeds
    what is left of g; counter c + 1 is unused and c + 2 + k gives the filler of actions[i, k], uniform over A.
    -> (ep int64 [n], pos int64 [n], filler int64 [n, K], prob float64 [n] = w / total, one division)."""
    weights = [[int(w) for w in ws] for ws in weights_per_episode]
    if not weights or min(len(ws) for ws in weights) <= 0:
        raise ValueError('draws need at least one episode, none of them empty')
    K, A = int(K), int(A)
    cums, ecum, total = [], [], 0
    for ws in weights:   # the device's tables: the inclusive prefix inside every episode, and over the episodes' masses
        acc, cum = 0, []
        for w in ws:
            acc += w
            cum.append(acc)
        total += acc
        cums.append(cum)
        ecum.append(total)
    base = _sm(_sm((int(seed) & _MASK) ^ _PRIO_SALT) ^ (int(step) & _MASK))

    def chain(c):
        return _sm(base ^ (c & _MASK))
    n = int(n) if targets is None else len(targets)
    ep = np.zeros(n, dtype=np.int64)
    pos = np.zeros(n, dtype=np.int64)
    filler = np.zeros((n, K), dtype=np.int64)
    prob = np.zeros(n, dtype=np.float64)
    for i in range(n):
        c = i * (K + 2)
        g = (chain(c) * total) >> 64 if targets is None else int(targets[i])
        if not 0 <= g < total:
            raise ValueError('target %d outside 0 .. %d' % (g, total - 1))
        j = bisect.bisect_right(ecum, g)   # the first episode with ecum[j] > g (upper_bound_u64)
        t = bisect.bisect_right(cums[j], g - (ecum[j - 1] if j else 0))
        ep[i], pos[i] = j, t
        prob[i] = float(weights[j][t]) / float(total)
        for k in range(K):
            filler[i, k] = (chain(c + 2 + k) * A) >> 64
    return ep, pos, filler, prob


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class MuZeroDeviceReplay(object):
    """A ring of ``capacity_episodes`` episodes of up to ``max_episode_steps`` steps on ``device``; ``len()`` is the number of
    episodes held, like the host buffer.  No CPU fallback: HipError without a GPU."""

    def __init__(self, obs_dim, n_actions, capacity_episodes, max_episode_steps, unroll_steps=5, td_steps=10, discount=0.997,
                 device='cuda:0', seed=0, prioritized=False, value_transform=False):
        import torch
        self.torch = torch
        self.lib = _hip.load()
        dev = torch.device(device)
        if dev.type != 'cuda' or not torch.cuda.is_available():
            raise HipError('the MuZero device replay buffer needs an MI355X (device=%r, cuda available=%s); there is no CPU fallback'
                           % (device, torch.cuda.is_available()))
        self.device = torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())
        self.obs_dim, self.n_actions, self.capacity = int(obs_dim), int(n_actions), int(capacity_episodes)
        self.max_episode_steps, self.K, self.td_steps = int(max_episode_steps), int(unroll_steps), int(td_steps)
        self.discount = discount
        self.seed = int(seed)
        self.step = 0   # the next update ``sample`` draws without a ``step``
        self.row = self.obs_dim + 4 + self.n_actions   # doubles of a packed record
        # the very expression ReplayBuffer._value_target evaluates, entry by entry
        self.disc = np.array([discount ** i for i in range(max(self.td_steps, 0) + 1)], dtype=np.float64)
        handle = ctypes.c_void_p()
        _hip.check(self.lib.rz_mz_replay_create(self.obs_dim, self.n_actions, self.capacity, self.max_episode_steps, self.K, self.td_steps,
                                                _ptr(self.disc), self.device.index, ctypes.byref(handle)), 'rz_mz_replay_create')
        self.handle = handle
        self.value_transform = bool(value_transform)
        if self.value_transform:
            _hip.check(self.lib.rz_mz_replay_set_value_transform(self.handle, 1), 'rz_mz_replay_set_value_transform')
        self.prioritized = False
        if prioritized:
            self.enable_priorities()

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _state(self):
        count, cursor, cap = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _hip.check(self.lib.rz_mz_replay_state(self.handle, ctypes.byref(count), ctypes.byref(cursor), ctypes.byref(cap), None), 'rz_mz_replay_state')
        return count.value, cursor.value, cap.value

    def __len__(self):
        return self._state()[0]

    def lengths(self):
        """Steps of every episode held, oldest first, int32 [len(self)] (the handle's host copy: no device access)."""
        out = np.zeros(max(len(self), 1), dtype=np.int32)
        _hip.check(self.lib.rz_mz_replay_state(self.handle, None, None, None, _ptr(out)), 'rz_mz_replay_state')
        return out[:len(self)]

    # ------------------------------------------------------------------ episodes in
    def _check_lengths(self, lengths):
        lengths = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
        if len(lengths) and int(lengths.max()) > self.max_episode_steps:
            raise ValueError('an episode of %d steps in a buffer of max_episode_steps %d' % (int(lengths.max()), self.max_episode_steps))
        if len(lengths) and int(lengths.min()) < 0:
            raise ValueError('an episode of negative length')
        return lengths

    def add_packed(self, block, lengths, first_rows=None, flags=None):
        """Episodes as rows of packed records -- ``block`` float64 [rows, obs | action | reward | visit counts | root value | done],
        episode i = rows first_rows[i] .. + lengths[i] (None: one behind the other) -- in ONE staging copy and ONE launch.  The
        policy is formed on the device as visits / sum(visits) in fp64, cast to float32; ``flags[i] & FINAL_POLICY``: the episode's
        visit columns already hold the float32 policy.  -> episodes added (empty ones are skipped)."""
        lengths = self._check_lengths(lengths)
        block = np.asarray(block, dtype=np.float64)
        if block.ndim != 2 or block.shape[1] != self.row:
            raise ValueError('packed records of shape %r, not [rows, %d]' % (block.shape, self.row))
        if first_rows is None:
            if int(lengths.sum()) != block.shape[0]:
                raise ValueError('%d rows for episodes of %d steps in all' % (block.shape[0], int(lengths.sum())))
            rows = block
        else:   # cut the episodes out, one behind the other
            first_rows = np.ascontiguousarray(first_rows, dtype=np.int64).reshape(-1)
            if len(first_rows) != len(lengths) or (len(lengths) and (first_rows.min() < 0 or (first_rows + lengths).max() > block.shape[0])):
                raise ValueError('an episode\'s rows lie outside the block')
            within = np.arange(int(lengths.sum())) - np.repeat(np.cumsum(lengths) - lengths, lengths)
            rows = block[np.repeat(first_rows, lengths) + within]
        if len(lengths) == 0:
            return 0
        rows = np.ascontiguousarray(rows)
        h_len = lengths.astype(np.int32)
        h_flags = None if flags is None else np.ascontiguousarray(flags, dtype=np.int32)
        _hip.check(self.lib.rz_mz_replay_add(self.handle, len(h_len), _ptr(h_len), _ptr(h_flags) if h_flags is not None else None, _ptr(rows),
                                             self._stream()), 'rz_mz_replay_add')
        return int((lengths > 0).sum())

    def _rows_of(self, ep):
        """An Episode's steps as packed rows with its float32 policy in the visit columns (FINAL_POLICY)."""
        n, D, A = len(ep), self.obs_dim, self.n_actions
        rows = np.zeros((n, self.row), dtype=np.float64)
        if n:
            obs, pol = np.asarray(ep.obs), np.asarray(ep.policies)
            if obs.shape != (n, D) or pol.shape != (n, A):
                raise ValueError('an episode with obs %r and policies %r in a buffer of obs_dim %d, %d actions' % (obs.shape, pol.shape, D, A))
            rows[:, :D] = obs.astype(np.float32)
            rows[:, D] = np.asarray(ep.actions)
            rows[:, D + 1] = np.asarray(ep.rewards, dtype=np.float64)
            rows[:, D + 2:D + 2 + A] = pol.astype(np.float32)
            rows[:, D + 2 + A] = np.asarray(ep.root_values, dtype=np.float64)
        return rows

    def add(self, episodes):
        """Finished episodes in order -- an ``EpisodeSeq`` (its packed stretches go as they are, the policy formed on the device)
        or any iterable of ``Episode`` -- as the host buffer's ``add`` of each of them: one staging copy and one launch for all.
        -> episodes added."""
        from .selfplay import Episode, EpisodeSeq
        blocks, lengths, flags = [], [], []
        if isinstance(episodes, Episode):
            episodes = [episodes]
        if isinstance(episodes, EpisodeSeq):
            for fields, first_rows, lens in episodes._chunks:
                self._check_lengths(lens)
                if len(fields) == 3 and isinstance(fields[1], int):   # packed records
                    if (fields[1], fields[2]) != (self.obs_dim, self.n_actions):
                        raise ValueError('records of obs_dim %d, %d actions in a buffer of %d, %d' % (fields[1], fields[2], self.obs_dim, self.n_actions))
                    within = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
                    blocks.append(np.asarray(fields[0], dtype=np.float64)[np.repeat(first_rows, lens) + within])
                    flags.extend([0] * len(lens))
                else:
                    for a, m in zip(first_rows, lens):   # the fields of the move-by-move routes: the policy is float32 already
                        blocks.append(self._rows_of(Episode.from_arrays(*(f[int(a):int(a) + int(m)] for f in fields))))
                    flags.extend([FINAL_POLICY] * len(lens))
                lengths.extend(int(v) for v in lens)
        else:
            for ep in episodes:
                self._check_lengths([len(ep)])
                blocks.append(self._rows_of(ep))
                lengths.append(len(ep))
                flags.append(FINAL_POLICY)
        if not lengths:
            return 0
        return self.add_packed(np.concatenate(blocks) if blocks else np.zeros((0, self.row)), lengths, flags=flags)

    def ingest(self, arena, lengths, first_rows):
        """Episodes straight from DEVICE memory: ``arena`` a float64 tensor [rows, obs | action | reward | visits | root value | done]
        on this device (``play_cartpole``'s arena), episode i = rows first_rows[i] .. + lengths[i].  Only the entry table travels;
        the launch is ordered on the current stream, behind whatever filled the arena there.  -> episodes added."""
        t = self.torch
        lengths = self._check_lengths(lengths)
        first_rows = np.ascontiguousarray(first_rows, dtype=np.int64).reshape(-1)
        if not isinstance(arena, t.Tensor) or arena.device != self.device or arena.dtype != t.float64 or arena.dim() != 2 \
                or arena.shape[1] != self.row or not arena.is_contiguous():
            raise ValueError('the arena: a contiguous float64 tensor [rows, %d] on %s' % (self.row, self.device))
        if len(first_rows) != len(lengths):
            raise ValueError('%d first rows for %d episodes' % (len(first_rows), len(lengths)))
        held = lengths > 0
        if held.any() and (int(first_rows[held].min()) < 0 or int((first_rows + lengths)[held].max()) > arena.shape[0]):
            raise ValueError('an episode\'s rows lie outside the arena of %d rows' % arena.shape[0])
        if len(lengths) == 0:
            return 0
        h_len = lengths.astype(np.int32)
        _hip.check(self.lib.rz_mz_replay_ingest(self.handle, len(h_len), _ptr(h_len), _ptr(first_rows), arena.data_ptr(), int(arena.shape[0]),
                                                self.row, self._stream()), 'rz_mz_replay_ingest')
        return int(held.sum())

    # ------------------------------------------------------------------ mini-batches out
    def _outputs(self, n):
        t, K, A = self.torch, self.K, self.n_actions
        kw = dict(device=self.device)
        return (t.empty((n, self.obs_dim), dtype=t.float32, **kw), t.empty((n, K), dtype=t.int64, **kw),
                t.empty((n, K + 1), dtype=t.float32, **kw), t.empty((n, K + 1), dtype=t.float32, **kw),
                t.empty((n, K + 1, A), dtype=t.float32, **kw), t.empty((n, K + 1), dtype=t.float32, **kw))

    @staticmethod
    def _out_ptrs(out):
        return [x.data_ptr() for x in out]

    def gather(self, ep_idx, pos, filler):
        """The six arrays of ``ReplayBuffer.sample`` for the draws ``ep_idx`` [n] (0 = the oldest episode held), ``pos`` [n] and
        ``filler`` [n, K] (the action of actions[i, k] when step pos + k lies past the end) -> (obs float32 [n, D], actions int64
        [n, K], tv, tr float32 [n, K + 1], tp float32 [n, K + 1, A], mask float32 [n, K + 1]) on the device, one launch.  The
        draws: numpy arrays / sequences (checked before the launch) or int64 device tensors (checked by the kernel: a draw out of
        range raises afterwards, and that entry's rows are not written)."""
        t, K = self.torch, self.K
        if all(isinstance(x, t.Tensor) for x in (ep_idx, pos, filler)):
            for x in (ep_idx, pos, filler):
                if x.device != self.device or x.dtype != t.int64:
                    raise ValueError('device draws: int64 tensors on %s' % (self.device, ))
            n = ep_idx.numel()
            draws = t.cat((ep_idx.reshape(n, 1), pos.reshape(n, 1), filler.reshape(n, K)), dim=1).contiguous()
            out = self._outputs(n)
            st = self._stream()
            _hip.check(self.lib.rz_mz_replay_gather(self.handle, None, draws.data_ptr(), n, *self._out_ptrs(out), st), 'rz_mz_replay_gather')
            flags = ctypes.c_int32()
            _hip.check(self.lib.rz_mz_replay_poll_errors(self.handle, ctypes.byref(flags), st), 'rz_mz_replay_poll_errors')
            if flags.value & _hip.MZ_REPLAY_BAD_INDEX:
                raise HipError('rz_mz_replay_gather: a draw from the device is out of range (episode, position or filler action)')
            return out
        ep_idx = np.asarray(ep_idx, dtype=np.int64).reshape(-1)
        n = len(ep_idx)
        draws = np.ascontiguousarray(np.concatenate((ep_idx.reshape(n, 1), np.asarray(pos, dtype=np.int64).reshape(n, 1),
                                                     np.asarray(filler, dtype=np.int64).reshape(n, K)), axis=1))
        out = self._outputs(n)
        _hip.check(self.lib.rz_mz_replay_gather(self.handle, _ptr(draws), None, n, *self._out_ptrs(out), self._stream()), 'rz_mz_replay_gather')
        return out

    def sample(self, n, step=None):
        """``n`` entries drawn on the device: ``gather(*mz_replay_draws(seed, step, n, self.lengths(), K, A))`` in one launch with
        no draw crossing the bus.  ``step``: the update's number; None = an internal counter, advanced by the call."""
        if step is None:
            step, self.step = self.step, self.step + 1
        out = self._outputs(int(n))
        _hip.check(self.lib.rz_mz_replay_sample(self.handle, self.seed & _MASK, int(step) & _MASK, int(n), *self._out_ptrs(out), self._stream()),
                   'rz_mz_replay_sample')
        return out

    # ------------------------------------------------------------------ prioritized replay
    def enable_priorities(self):
        """Turns prioritized replay on: the per-step integer priorities, their prefix sums and the dirty marks are allocated on
        the device and every episode held is marked; from here on ``add`` / ``ingest`` / ``update`` mark what they write and the
        next prioritized draw refreshes the marked episodes on its own stream.  ``sample`` is not changed."""
        if not self.prioritized:
            _hip.check(self.lib.rz_mz_replay_enable_priorities(self.handle, self._stream()), 'rz_mz_replay_enable_priorities')
            self.prioritized = True

    def _need_priorities(self, what):
        if not self.prioritized:
            raise HipError('%s: priorities are off (MuZeroDeviceReplay(prioritized=True) or enable_priorities())' % what)

    def refresh_priorities(self):
        """The priorities of every episode written since the last refresh and the prefix over the episodes, two launches on the
        current stream (a prioritized draw does this by itself when anything was written)."""
        self._need_priorities('refresh_priorities')
        _hip.check(self.lib.rz_mz_replay_refresh_priorities(self.handle, self._stream()), 'rz_mz_replay_refresh_priorities')

    def priorities(self):
        """The integer priority of every step held: a list of int64 arrays, oldest episode first (``mz_priority_weights`` of
        each episode, bit for bit).  With ``value_transform`` they are still |root value - n-step return| in raw units: the
        same numbers as without it.  A synchronous copy (tests, debugging)."""
        self._need_priorities('priorities')
        n, T = len(self), self.max_episode_steps
        w = np.zeros((max(n, 1), T), dtype=np.int64)
        total = ctypes.c_int64()
        if n:
            _hip.check(self.lib.rz_mz_replay_read_priorities(self.handle, 0, n, _ptr(w), ctypes.byref(total), self._stream()),
                       'rz_mz_replay_read_priorities')
        out = [w[j, :int(m)].copy() for j, m in enumerate(self.lengths())]
        if sum(int(x.sum()) for x in out) != total.value:
            raise HipError('rz_mz_replay_read_priorities: the weights sum to %d, the device total is %d'
                           % (sum(int(x.sum()) for x in out), total.value))
        return out

    def _draw_prioritized(self, n, step, targets):
        t = self.torch
        self._need_priorities('prioritized draws')
        d_targets = None
        if targets is not None:
            if not isinstance(targets, t.Tensor):
                targets = t.from_numpy(np.ascontiguousarray(targets, dtype=np.int64).reshape(-1)).to(self.device)
            if targets.device != self.device or targets.dtype != t.int64:
                raise ValueError('targets: int64 on %s' % (self.device, ))
            targets = targets.reshape(-1).contiguous()
            n, d_targets = targets.numel(), targets.data_ptr()
        n = int(n)
        if step is None:
            step, self.step = self.step, self.step + 1
        draws = t.empty((n, self.K + 2), dtype=t.int64, device=self.device)
        prob = t.empty((n, ), dtype=t.float64, device=self.device)
        _hip.check(self.lib.rz_mz_replay_draw_prioritized(self.handle, self.seed & _MASK, int(step) & _MASK, n, d_targets, draws.data_ptr(),
                                                          prob.data_ptr(), self._stream()), 'rz_mz_replay_draw_prioritized')
        return draws, prob

    def prioritized_draws(self, n, step=None, targets=None):
        """``n`` steps drawn on the device in proportion to their priorities (``mz_prioritized_draws``: the same bits) ->
        device tensors (ep_idx int64 [n], pos int64 [n], filler int64 [n, K], prob float64 [n]).  ``targets`` (int64 [n], numpy
        or device): the entries' targets in 0 .. total - 1 instead of the stream's, e.g. stratified ones; one outside that
        range raises (and its row is all -1).  ``step`` None: ``sample``'s counter, advanced by the call.  Waits for the
        stream to read the flag word; ``sample_prioritized`` does not."""
        draws, prob = self._draw_prioritized(n, step, targets)
        if targets is not None and self.poll_errors() & _hip.MZ_REPLAY_BAD_INDEX:
            raise HipError('rz_mz_replay_draw_prioritized: a target is outside 0 .. total - 1')
        return draws[:, 0], draws[:, 1], draws[:, 2:], prob

    def sample_prioritized(self, n, step=None, beta=1.0):
        """A mini-batch drawn by priority -> (the six tensors of ``gather`` for the device's draws, weights float32 [n]): the
        draw launch, then the gather launch on the draws where they lie -- no flag is polled, the library made the draws --
        and weights = (n_steps * prob) ** -beta, the importance weights of the paper (n_steps: the steps held)."""
        draws, prob = self._draw_prioritized(n, step, None)
        out = self._outputs(int(n))
        _hip.check(self.lib.rz_mz_replay_gather(self.handle, None, draws.data_ptr(), int(n), *self._out_ptrs(out), self._stream()), 'rz_mz_replay_gather')
        n_steps = int(self.lengths().astype(np.int64).sum())
        return out, ((n_steps * prob) ** (-float(beta))).float()

    # ------------------------------------------------------------------ Reanalyse: stored steps out, fresh targets back
    def positions(self, ep_idx=None, pos=None, n=None, seed=None, step=0):
        """Entries resolved to physical steps and their stored observations, one launch (k_mzr_positions) -> (where int32 [n, 2]
        = (slot, position), obs float32 [n, D], ticket).  The entries: ``ep_idx`` / ``pos`` [n] (episode 0 = the oldest held) as
        numpy arrays / sequences (checked before the launch) or int64 device tensors (checked by the kernel: such an entry gets
        where = (-1, -1), a zeroed observation and the BAD_INDEX flag of ``poll_errors``), or, both None, the device's own ``n``
        draws of refresh ``step`` (reanalyse.py: mz_reanalyse_draws).  ``ticket`` counts the episodes ever stored here: ``update``
        takes it back and refuses if an ``add`` / ``ingest`` came in between."""
        t = self.torch
        h_draws = d_draws = keep = None
        if ep_idx is None:
            if pos is not None or n is None:
                raise ValueError('positions: draws (ep_idx and pos) or a number of entries to draw on the device')
            n = int(n)
        elif isinstance(ep_idx, t.Tensor) and isinstance(pos, t.Tensor):
            for x in (ep_idx, pos):
                if x.device != self.device or x.dtype != t.int64:
                    raise ValueError('device draws: int64 tensors on %s' % (self.device, ))
            n = ep_idx.numel()
            if pos.numel() != n:
                raise ValueError('%d episodes and %d positions' % (n, pos.numel()))
            keep = t.stack((ep_idx.reshape(n), pos.reshape(n)), dim=1).contiguous()
            d_draws = keep.data_ptr()
        else:
            ep_idx = np.asarray(ep_idx, dtype=np.int64).reshape(-1)
            n = len(ep_idx)
            keep = np.ascontiguousarray(np.stack((ep_idx, np.asarray(pos, dtype=np.int64).reshape(n)), axis=1))
            h_draws = _ptr(keep)
        where = t.empty((n, 2), dtype=t.int32, device=self.device)
        obs = t.empty((n, self.obs_dim), dtype=t.float32, device=self.device)
        ticket = ctypes.c_int64(-1)
        _hip.check(self.lib.rz_mz_replay_positions(self.handle, h_draws, d_draws, (self.seed if seed is None else int(seed)) & _MASK,
                                                   int(step) & _MASK, n, where.data_ptr(), obs.data_ptr(), ctypes.byref(ticket), self._stream()),
                   'rz_mz_replay_positions')
        return where, obs, ticket.value

    def update(self, where, visits, root_n, root_sum, ticket):
        """The policy and the root value of every step named by a valid row of ``where`` (int32 [n, 2], of ``positions``) from a
        fresh search's ``visits`` int32 [n, A], ``root_n`` int32 [n] and ``root_sum`` float64 [n], one launch (k_mzr_update):
        policy = float32(visits / sum(visits)), root value = root_sum / max(root_n, 1); nothing else is written, a row of
        (-1, -1) writes nothing.  HipError, and no launch, if episodes were stored since ``ticket`` was given out."""
        t = self.torch
        n = int(where.shape[0]) if where.dim() == 2 else -1
        for x, dtype, shape in ((where, t.int32, (n, 2)), (visits, t.int32, (n, self.n_actions)), (root_n, t.int32, (n, )),
                                (root_sum, t.float64, (n, ))):
            if not isinstance(x, t.Tensor) or x.device != self.device or x.dtype != dtype or tuple(x.shape) != shape or not x.is_contiguous():
                raise ValueError('update: contiguous tensors on %s -- where int32 [n, 2], visits int32 [n, %d], root_n int32 [n], '
                                 'root_sum float64 [n]' % (self.device, self.n_actions))
        _hip.check(self.lib.rz_mz_replay_update(self.handle, where.data_ptr(), n, visits.data_ptr(), root_n.data_ptr(), root_sum.data_ptr(),
                                                int(ticket), self._stream()), 'rz_mz_replay_update')

    def poll_errors(self):
        """The device's flag word (_hip.MZ_REPLAY_BAD_INDEX / MZ_REPLAY_BAD_ROWS), cleared by the call; waits for the stream."""
        flags = ctypes.c_int32()
        _hip.check(self.lib.rz_mz_replay_poll_errors(self.handle, ctypes.byref(flags), self._stream()), 'rz_mz_replay_poll_errors')
        return flags.value

    def read(self):
        """The episodes held, oldest first, as the host buffer keeps them: a list of ``Episode`` (obs float32 [n, D], actions
        int64 [n], rewards float64 [n], policies float32 [n, A], root_values float64 [n]).  A synchronous copy (tests, debugging)."""
        from .selfplay import Episode
        n, T, D, A = len(self), self.max_episode_steps, self.obs_dim, self.n_actions
        obs = np.zeros((n, T, D), dtype=np.float32)
        action = np.zeros((n, T), dtype=np.int32)
        reward = np.zeros((n, T), dtype=np.float64)
        value = np.zeros((n, T), dtype=np.float64)
        policy = np.zeros((n, T, A), dtype=np.float32)
        length = np.zeros(n, dtype=np.int32)
        if n:
            _hip.check(self.lib.rz_mz_replay_read(self.handle, 0, n, _ptr(obs), _ptr(action), _ptr(reward), _ptr(value), _ptr(policy), _ptr(length),
                                                  self._stream()), 'rz_mz_replay_read')
        return [Episode.from_arrays(obs[j, :m].copy(), action[j, :m].astype(np.int64), reward[j, :m].copy(), policy[j, :m].copy(), value[j, :m].copy())
                for j, m in enumerate(int(v) for v in length)]

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.rz_mz_replay_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
