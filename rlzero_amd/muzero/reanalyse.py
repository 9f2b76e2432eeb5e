"""MuZero Reanalyse (arXiv:1911.08265v2 appendix H; "MuZero Unplugged"): stored steps searched again with the CURRENT network,
their policy and root-value targets refreshed in the device replay buffer.

The policy and the root value of a stored step are those of the search that played it, with the network of that time; the value
bootstraps of ``MuZeroDeviceReplay.sample`` (``root_value[t + td_steps]``) and its policy targets go stale as the learner moves
on.  ``MuZeroReanalyser`` joins the two device ends of the store (csrc/rz_mz_replay.hip: k_mzr_positions hands stored
observations out, k_mzr_update takes visit counts and root statistics back) with a search of its own: a second, small
``MuZeroTree`` and hidden buffer, apart from any ``MuZeroSelfPlay``'s.  A request is resolved in ONE ``positions`` launch and then
worked off in chunks of ``batch`` rows, every chunk ordered on the current torch stream with no host synchronisation (the error
poll for draws given as device tensors apart):

  observations of the chunk -> ``net.initial_inference`` under ``no_grad``, softmax -> ``hidden[:, 0]`` -> ``init_roots`` without
  exploration noise -> the search (``rz_mz_search`` in one launch when the model fits it, else ``n_sims`` x select / recurrent
  inference / expand + backup) -> root visit counts, N and value sum -> ``update``

The inference and the search always run on ``batch`` rows, so the GEMM shapes never change: in a short last chunk the rows past
the end repeat the chunk's first observation, carry where = (-1, -1) and write nothing.  What a refreshed step holds is bit for bit
``float32(visits / visits.sum())`` and ``value_sum / max(N, 1)`` of ``MuZeroSelfPlay.search(obs, add_noise=False)`` on the same
rows.  Two entries that name one step both write it; the search is deterministic, so they write the same bits.

The class stores no episode itself.  ``update`` carries the ticket ``positions`` gave out: if the caller's ``add`` / ``ingest``
comes between them a slot may hold another episode by then, and the call raises ``HipError`` instead of writing.
"""
import numpy as np

from .._hip import MZ_REPLAY_BAD_INDEX, HipError
from .._rng import MASK as _MASK, mix64 as _sm

_REANALYSE_SALT = 0x6D7A7265616E616C   # "mzreanal" (csrc/rz_mz_target.h: kReanalyseSalt)
_MAX_REQUEST = 1 << 20                 # entries resolved by one ``positions`` launch (its staging copy: 16 bytes each)


def mz_reanalyse_draws(seed, step, n, lengths):
    """The draws of ``reanalyse_sample(n, step)`` over episodes of these ``lengths`` (oldest first), in Python integers -- the
    device's bits (k_mzr_positions): counter c = 2 i + j of refresh ``step`` gives the high half of x * m for the 64-bit x of the
    splitmix64 chain over (seed ^ "mzreanal", step, c); j = 0 the episode (m = episodes held), j = 1 the position (m = its
    length).  -> (ep_idx int64 [n], pos int64 [n])."""
    lengths = [int(v) for v in lengths]
    if not lengths or min(lengths) <= 0:
        raise ValueError('draws need at least one episode, none of them empty')
    base = _sm(_sm((int(seed) & _MASK) ^ _REANALYSE_SALT) ^ (int(step) & _MASK))

    def draw(c, m):
        return (_sm(base ^ (c & _MASK)) * m) >> 64
    ep = np.zeros(n, dtype=np.int64)
    pos = np.zeros(n, dtype=np.int64)
    for i in range(int(n)):
        ep[i] = draw(2 * i, len(lengths))
        pos[i] = draw(2 * i + 1, lengths[ep[i]])
    return ep, pos


class MuZeroReanalyser(object):
    """Fresh searches of steps held by ``replay`` (a MuZeroDeviceReplay) with ``net`` as it is now.  ``fused``: the search of a
    chunk in one launch (k_mz_search); None = whenever the model fits it (hidden size 64, <= 8 actions), as MuZeroSelfPlay
    decides -- the weights are uploaded again whenever the torch parameters changed.  ``timer``: None, or a callable
    ``timer(label)`` called on the stream between the stages of every chunk (profiles/ab_mz_reanalyse.py records events there)."""

    def __init__(self, net, replay, n_sims=50, batch=256, discount=0.997, pb_c_base=19652.0, pb_c_init=1.25, fused=None, seed=0):
        import torch
        from .tree import MuZeroTree
        self.torch = torch
        self.net, self.replay = net, replay
        self.device = replay.device
        self.n_actions, self.obs_dim = replay.n_actions, replay.obs_dim
        if (net.obs_dim, net.n_actions) != (self.obs_dim, self.n_actions):
            raise ValueError('a net of obs_dim %d, %d actions on a buffer of %d, %d' % (net.obs_dim, net.n_actions, self.obs_dim, self.n_actions))
        from .agent import check_value_transform
        check_value_transform(net, replay)
        self.n_sims, self.batch = int(n_sims), int(batch)
        if self.batch < 1 or self.n_sims < 1:
            raise ValueError('batch and n_sims must be positive')
        self.seed = int(seed)
        self.step = 0   # the next refresh ``reanalyse_sample`` draws without a ``step``
        self.fused = (net.hidden == 64 and self.n_actions <= 8) if fused is None else bool(fused)
        self.tree = MuZeroTree(self.batch, self.n_actions, self.n_sims, discount, pb_c_base, pb_c_init, device=str(self.device))
        # the net's flag (MuZeroNet(value_transform=True)): the search inverts the heads, so what is written back is a RAW root value
        self.value_transform = bool(getattr(net, 'value_transform', False))
        if self.value_transform:
            self.tree.set_value_transform(True)
        kw = dict(device=self.device)
        self.hidden = torch.zeros((self.batch, self.tree.slots_per_game, net.hidden), dtype=torch.float32, **kw)
        self.rows = torch.arange(self.batch, **kw)
        # a short last chunk is padded here: rows past the end repeat its first observation and write nothing
        self._obs = torch.zeros((self.batch, self.obs_dim), dtype=torch.float32, **kw)
        self._where = torch.full((self.batch, 2), -1, dtype=torch.int32, **kw)
        self._model_seen = None
        self.positions_done = 0
        self.sims_done = 0
        self.timer = None

    def close(self):
        self.tree.close()

    def _refresh_model(self):
        """(Re-)upload the model's weights for the fused search if the torch module changed (a learner step)."""
        seen = tuple((p.data_ptr(), p._version) for p in self.net.parameters())
        if seen != self._model_seen:
            self.tree.load_model(self.net)
            self._model_seen = seen

    def _mark(self, label):
        if self.timer is not None:
            self.timer(label)

    def _search(self):
        t, tree, net = self.torch, self.tree, self.net
        if self.fused:
            self._refresh_model()
            tree.search_fused(self.hidden, self.n_sims)
            return
        for _ in range(self.n_sims):
            parent, action, leaf = tree.select()
            state = self.hidden[self.rows, parent.long()]
            nxt, reward, logits, value = net.recurrent_inference(state, action.long())
            self.hidden[self.rows, leaf.long()] = nxt
            if self.value_transform:
                from .network import inverse_value_transform
                reward, value = inverse_value_transform(reward), inverse_value_transform(value)
            tree.expand_backup(reward.contiguous(), t.softmax(logits, dim=1).contiguous(), value.contiguous())

    def _chunk(self, where, obs, ticket):
        """One chunk of at most ``batch`` resolved entries: search their observations, write the results back."""
        t, tree, m = self.torch, self.tree, int(where.shape[0])
        if m < self.batch:
            self._obs[:m] = obs
            self._obs[m:] = obs[0]
            self._where[:m] = where
            self._where[m:] = -1
            where, obs = self._where, self._obs
        with t.no_grad():
            s0, logits, _ = self.net.initial_inference(obs)
            probs = t.softmax(logits, dim=1).contiguous()
            self.hidden[:, 0] = s0
            self._mark('inference')
            tree.init_roots(probs, None)
            self._search()
            self._mark('search')
            visits = tree.root_visits()
            root_n, root_sum, _, _ = tree.root_stats()
            self.replay.update(where, visits, root_n, root_sum, ticket)
            self._mark('update')
        self.sims_done += self.n_sims * self.batch

    def _request(self, n, ep_idx=None, pos=None, step=0):
        """``n`` entries (given, or drawn on the device) resolved in one launch, then chunk by chunk."""
        if n == 0:
            return 0
        self._mark('start')
        where, obs, ticket = self.replay.positions(ep_idx, pos, n=n if ep_idx is None else None, seed=self.seed, step=step)
        if ep_idx is not None and isinstance(ep_idx, self.torch.Tensor) and self.replay.poll_errors() & MZ_REPLAY_BAD_INDEX:
            raise HipError('reanalyse: a draw from the device is out of range (episode or position); nothing was refreshed')
        self._mark('positions')
        for a in range(0, n, self.batch):
            self._chunk(where[a:a + self.batch], obs[a:a + self.batch], ticket)
        self.tree.check()
        self.positions_done += n
        return n

    def reanalyse(self, ep_idx, pos):
        """Refresh the steps (``ep_idx[i]``, ``pos[i]``) -- episode 0 is the oldest held, as in ``gather`` -- given as numpy arrays
        / sequences (checked before any launch) or int64 device tensors (checked on the device: HipError, and nothing is
        refreshed).  -> the number of positions refreshed."""
        t = self.torch
        if isinstance(ep_idx, t.Tensor) != isinstance(pos, t.Tensor):
            raise ValueError('reanalyse: both draws on the host or both on the device')
        if not isinstance(ep_idx, t.Tensor):
            ep_idx = np.asarray(ep_idx, dtype=np.int64).reshape(-1)
            pos = np.asarray(pos, dtype=np.int64).reshape(-1)
        else:
            ep_idx, pos = ep_idx.reshape(-1), pos.reshape(-1)
        n = int(ep_idx.shape[0])
        if int(pos.shape[0]) != n:
            raise ValueError('%d episodes and %d positions' % (n, int(pos.shape[0])))
        return sum(self._request(min(_MAX_REQUEST, n - a), ep_idx[a:a + _MAX_REQUEST], pos[a:a + _MAX_REQUEST]) for a in range(0, n, _MAX_REQUEST))

    def reanalyse_sample(self, n, step=None):
        """Refresh ``n`` steps drawn on the device -- ``mz_reanalyse_draws(seed, step, n, replay.lengths())``: the episode uniform
        over those held, the position uniform over its length.  ``step``: the refresh's number; None = an internal counter,
        advanced by the call.  -> n."""
        n = int(n)
        if not 0 <= n <= (1 << 24):
            raise ValueError('n outside 0 .. 2^24')
        if step is None:
            step, self.step = self.step, self.step + 1
        return self._request(n, step=step)

    def reanalyse_all(self):
        """Refresh every step of every episode held (enumerated on the host from ``replay.lengths()``).  -> their number."""
        lengths = self.replay.lengths().astype(np.int64)
        if len(lengths) == 0:
            return 0
        ep_idx = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
        pos = np.arange(int(lengths.sum()), dtype=np.int64) - np.repeat(np.cumsum(lengths) - lengths, lengths)
        return self.reanalyse(ep_idx, pos)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
