"""ctypes binding of the MuZero search tree kernels (include/rlzero_hip.h, rz_mz_*)."""
import ctypes

import numpy as np

from .. import _hip
from ..engine import _ptr, check


class MuZeroTree(object):
    """Search trees of ``n_games`` environments on one GPU.  Step by step (``select`` / ``expand_backup``) the learned
    model is the caller's: see ``MuZeroSelfPlay.search`` for the simulation loop; ``search_fused``, ``play_cartpole`` and ``play_env``
    evaluate it inside the kernel (``load_model`` / ``load_representation`` first)."""

    def __init__(self, n_games, n_actions, n_sims, discount=0.997, pb_c_base=19652.0, pb_c_init=1.25,
                 device='cuda:0'):
        import torch
        self.torch = torch
        self.lib = _hip.load()
        self.device = torch.device(device)
        if self.device.type != 'cuda' or not torch.cuda.is_available():
            raise _hip.HipError('MuZeroTree needs an MI355X (device=%r): there is no CPU path' % (device, ))
        self.n_games, self.n_actions, self.n_sims = int(n_games), int(n_actions), int(n_sims)
        self.discount = float(discount)
        self.value_transform = False   # set_value_transform
        cfg = _hip.RzMzConfig(_hip.ABI_VERSION, self.n_games, self.n_actions, self.n_sims, self.discount,
                              float(pb_c_base), float(pb_c_init), self.device.index or 0, 0)
        self.handle = ctypes.c_void_p()
        check(self.lib.rz_mz_create(ctypes.byref(cfg), ctypes.byref(self.handle)), 'rz_mz_create')
        slots, nbytes = ctypes.c_int32(0), ctypes.c_int64(0)
        check(self.lib.rz_mz_geometry(self.handle, ctypes.byref(slots), ctypes.byref(nbytes)), 'rz_mz_geometry')
        self.slots_per_game, self.device_bytes = slots.value, nbytes.value
        kw = dict(device=self.device)
        G, A = self.n_games, self.n_actions
        self.parent = torch.zeros(G, dtype=torch.int32, **kw)
        self.action = torch.zeros(G, dtype=torch.int32, **kw)
        self.leaf = torch.zeros(G, dtype=torch.int32, **kw)
        self.visits = torch.zeros((G, A), dtype=torch.int32, **kw)
        self.child_f64 = torch.zeros((G, A), dtype=torch.float64, **kw)
        self.root_n = torch.zeros(G, dtype=torch.int32, **kw)
        self.root_sum = torch.zeros(G, dtype=torch.float64, **kw)
        self.vmin = torch.zeros(G, dtype=torch.float64, **kw)
        self.vmax = torch.zeros(G, dtype=torch.float64, **kw)
        # the very table CPython's math.log gives on this host
        import math
        tab = np.array([math.log((n + pb_c_base + 1) / pb_c_base) for n in range(self.n_sims + 2)], dtype=np.float64)
        check(self.lib.rz_mz_upload_log_table(self.handle, ctypes.c_void_p(tab.ctypes.data), tab.size),
              'rz_mz_upload_log_table')

    MODEL_PARAMS = ('dyn1.weight', 'dyn1.bias', 'dyn2.weight', 'dyn2.bias', 'rew1.weight', 'rew1.bias', 'rew2.weight',
                    'rew2.bias', 'pre1.weight', 'pre1.bias', 'pol.weight', 'pol.bias', 'val.weight', 'val.bias')

    def load_model(self, net):
        """Upload the dynamics / reward / prediction layers of a MuZeroNet (hidden size 64) for ``search_fused``; call
        again after every optimiser step."""
        sd = net.state_dict()
        arrays = [sd[name].detach().to('cpu', self.torch.float32).contiguous().numpy() for name in self.MODEL_PARAMS]
        ptrs = (ctypes.c_void_p * 14)(*[a.ctypes.data for a in arrays])
        check(self.lib.rz_mz_load_model(self.handle, ptrs, 14, int(net.hidden)), 'rz_mz_load_model')

    REPRESENTATION_PARAMS = ('rep1.weight', 'rep1.bias', 'rep2.weight', 'rep2.bias')

    def load_representation(self, net):
        """Upload the representation layers h(o) of a MuZeroNet (for ``play_cartpole`` / ``play_env``); call again after every
        optimiser step, like ``load_model``."""
        sd = net.state_dict()
        arrays = [sd[name].detach().to('cpu', self.torch.float32).contiguous().numpy() for name in self.REPRESENTATION_PARAMS]
        ptrs = (ctypes.c_void_p * 4)(*[a.ctypes.data for a in arrays])
        check(self.lib.rz_mz_load_representation(self.handle, ptrs, 4, int(net.obs_dim), int(net.hidden)),
              'rz_mz_load_representation')

    def play_cartpole(self, hidden, n_sims, n_moves, env, noise_seed, noise_frac, alpha, temperature, history, first_step,
                      arena, counters, entries):
        """``n_moves`` whole moves of the CartPoleBatch ``env`` in ONE launch (k_mz_search, MOVES stages): initial
        inference, root noise, ``n_sims`` simulations, action from the visit counts, environment step.  ``history`` =
        (ring float64 [G, ring_steps, 8 + A], episode_start int64 [G]): every move's record -- observation (4) | action |
        reward | visits (A) | root value | done -- lands in the ring at step % ring_steps (step = first_step + move); the
        records of every episode that ENDS are copied as one run into ``arena`` float64 [rows, 8 + A] and described in
        ``entries`` int64 [n, 4] (environment, end step, length, first arena row or -1); ``counters`` int64 [4] (zeroed
        here): arena rows claimed, entries, episodes that did not fit."""
        ring, episode_start = history
        counters.zero_()
        play = _hip.RzMzCartPolePlay(
            env.state.data_ptr(), env.steps.data_ptr(), env.episode_dev.data_ptr(), episode_start.data_ptr(),
            int(env.seed) & (2 ** 64 - 1), int(noise_seed) & (2 ** 64 - 1), float(noise_frac), float(alpha), float(temperature),
            ring.data_ptr(), int(ring.shape[1]), 0, int(first_step), arena.data_ptr(), int(arena.shape[0]),
            counters.data_ptr(), entries.data_ptr(), int(entries.shape[0]))
        check(self.lib.rz_mz_play_cartpole(self.handle, _ptr(hidden), int(n_sims), int(n_moves), ctypes.byref(play), self.stream()),
              'rz_mz_play_cartpole')

    def play_env(self, hidden, n_sims, n_moves, env, noise_seed, noise_frac, alpha, temperature, history, first_step,
                 arena, counters, entries, kind=None, max_episode_steps=None):
        """``play_cartpole`` for the environment batch ``env`` of any kind the library knows (``env.kind``: 'cartpole' | 'acrobot';
        rz_mz_play_env, k_mz_search<TREE_LDS, MOVES, Env>): ``n_moves`` whole moves in ONE launch.  A record is obs (D) | action |
        reward | visits (A) | root value | done, D + 4 + A float64; ``history`` = (ring [G, ring_steps, D + 4 + A], episode_start
        int64 [G]) with ring_steps >= max_episode_steps + n_moves; ``arena`` float64 [rows, D + 4 + A]; ``entries`` and ``counters``
        (zeroed here) as ``play_cartpole``'s.  ``kind`` / ``max_episode_steps``: None = the environment's (``_hip.MZ_ENV_KINDS``).
        The library refuses -- HipError, nothing launched -- an unknown kind, a tree or a loaded representation of another shape
        than the environment's, alpha < 0.1 and a ring too small."""
        ring, episode_start = history
        kind = _hip.MZ_ENV_KINDS[env.kind] if kind is None else int(kind)
        limit = int(env.max_episode_steps if max_episode_steps is None else max_episode_steps)
        t, G, row = self.torch, self.n_games, env.obs_dim + 4 + env.n_actions
        if env.n_envs != G or ring.dim() != 3 or tuple(ring.shape[::2]) != (G, row) or tuple(episode_start.shape) != (G, ) \
                or arena.dim() != 2 or arena.shape[1] != row or entries.dim() != 2 or entries.shape[1] != 4 or counters.numel() < 4 \
                or tuple(env.state.shape) != (G, 4) or hidden.numel() < G * self.slots_per_game * 64:
            raise ValueError('play_env: the ring, the arena, the entries, the states or the hidden states do not have the environment\'s shape')
        for x, dtype in ((ring, t.float64), (arena, t.float64), (episode_start, t.int64), (counters, t.int64), (entries, t.int64)):
            if x.dtype != dtype or not x.is_contiguous() or x.device.type != 'cuda':
                raise ValueError('play_env: contiguous float64 / int64 tensors on the device are expected')
        counters.zero_()
        play = _hip.RzMzWholePlay(
            env.state.data_ptr(), env.steps.data_ptr(), env.episode_dev.data_ptr(), episode_start.data_ptr(),
            int(env.seed) & (2 ** 64 - 1), int(noise_seed) & (2 ** 64 - 1), float(noise_frac), float(alpha), float(temperature),
            ring.data_ptr(), int(ring.shape[1]), 0, int(first_step), arena.data_ptr(), int(arena.shape[0]),
            counters.data_ptr(), entries.data_ptr(), int(entries.shape[0]), limit)
        check(self.lib.rz_mz_play_env(self.handle, kind, _ptr(hidden), int(n_sims), int(n_moves), ctypes.byref(play), self.stream()),
              'rz_mz_play_env')

    def env_move(self, env, noise_seed, temperature, history, step, arena, counters, entries, obs_out):
        """The move behind a finished search (``search_fused`` on the current stream) for the environment batch ``env`` of a kind
        the library knows (``env.kind``: 'cartpole' | 'acrobot'), one launch (k_mz_env_move): the action from the root's visit
        counts, the record into ``history`` = (ring float64 [G, ring_steps, D + 4 + A], episode_start int64 [G]) at ``step`` %
        ring_steps, the environment step, the hand-over of a finished episode to ``arena`` / ``entries`` / ``counters`` (laid out
        as ``play_cartpole``'s; NOT zeroed here: several moves share an arena) and the next observation to ``obs_out`` float32
        [G, D]."""
        ring, episode_start = history
        kind = _hip.MZ_ENV_KINDS[env.kind]
        t, G, row = self.torch, self.n_games, env.obs_dim + 4 + self.n_actions
        if env.n_actions != self.n_actions or env.n_envs != G or ring.dim() != 3 or tuple(ring.shape[::2]) != (G, row) \
                or tuple(obs_out.shape) != (G, env.obs_dim) or tuple(episode_start.shape) != (G, ) or arena.dim() != 2 or arena.shape[1] != row \
                or entries.dim() != 2 or entries.shape[1] != 4 or counters.numel() < 4:
            raise ValueError('env_move: the tree, the ring, the arena, the entries or the observations do not have the environment\'s shape')
        for x, dtype in ((ring, t.float64), (arena, t.float64), (obs_out, t.float32), (episode_start, t.int64), (counters, t.int64), (entries, t.int64)):
            if x.dtype != dtype or not x.is_contiguous() or x.device.type != 'cuda':
                raise ValueError('env_move: contiguous float64 / float32 / int64 tensors on the device are expected')
        play = _hip.RzMzEnvPlay(
            env.state.data_ptr(), env.steps.data_ptr(), env.episode_dev.data_ptr(), episode_start.data_ptr(),
            int(env.seed) & (2 ** 64 - 1), int(noise_seed) & (2 ** 64 - 1), float(temperature), int(env.max_episode_steps),
            ring.data_ptr(), int(ring.shape[1]), 0, int(step), arena.data_ptr(), int(arena.shape[0]), counters.data_ptr(),
            entries.data_ptr(), int(entries.shape[0]), obs_out.data_ptr())
        check(self.lib.rz_mz_env_move(self.handle, kind, ctypes.byref(play), self.stream()), 'rz_mz_env_move')

    def root_noise(self, episode, steps, noise_seed, alpha, out=None):
        """The whole moves' normalised root noise for the moves (environment g, ``episode[g]``, ``steps[g]``) -- int64 [G] on the
        device -- under ``noise_seed``: float64 [G, A] in the form ``init_roots`` takes (k_mz_root_noise).  alpha >= 0.1."""
        if out is None:
            out = self.torch.zeros((self.n_games, self.n_actions), dtype=self.torch.float64, device=self.device)
        check(self.lib.rz_mz_root_noise(self.handle, _ptr(episode), _ptr(steps), int(noise_seed) & (2 ** 64 - 1), float(alpha), _ptr(out),
                                        self.stream()), 'rz_mz_root_noise')
        return out

    def set_search_shape(self, games_per_workgroup=0):
        """Games per workgroup of ``search_fused`` (<= 16; 0 = chosen from the number of games and CUs)."""
        check(self.lib.rz_mz_set_search_shape(self.handle, int(games_per_workgroup)), 'rz_mz_set_search_shape')
        return self

    def set_value_transform(self, on=True):
        """The value transform of the searches inside the kernel (rz_mz_set_value_transform; ``search_fused``, ``play_cartpole``,
        ``play_env``): on, the network's reward and value of every simulation go through ``h^-1`` (csrc/rz_mz_value.h, fp64, one
        rounding to float32) before the trace and the backup, so the tree and the root values are in raw units; off (the default),
        they are used as they come.  ``expand_backup`` takes what it is given either way."""
        check(self.lib.rz_mz_set_value_transform(self.handle, 1 if on else 0), 'rz_mz_set_value_transform')
        self.value_transform = bool(on)
        return self

    def search_fused(self, hidden, n_sims, trace=False):
        """All ``n_sims`` simulations of every game in ONE launch (k_mz_search; init_roots and the root's hidden state
        in ``hidden[:, 0]`` first).  ``trace``: returns per simulation what the kernel selected and its network outputs:
        dict of tensors parent / action / leaf int32 [n_sims, G], reward / value float32 [n_sims, G], probs [n_sims, G, A]."""
        t = self.torch
        out = None
        args = [None] * 6
        if trace:
            kw = dict(device=self.device)
            G, A = self.n_games, self.n_actions
            out = {'parent': t.zeros((n_sims, G), dtype=t.int32, **kw), 'action': t.zeros((n_sims, G), dtype=t.int32, **kw),
                   'leaf': t.zeros((n_sims, G), dtype=t.int32, **kw), 'reward': t.zeros((n_sims, G), dtype=t.float32, **kw),
                   'probs': t.zeros((n_sims, G, A), dtype=t.float32, **kw), 'value': t.zeros((n_sims, G), dtype=t.float32, **kw)}
            args = [_ptr(out[k]) for k in ('parent', 'action', 'leaf', 'reward', 'probs', 'value')]
        check(self.lib.rz_mz_search(self.handle, _ptr(hidden), int(n_sims), *args, self.stream()), 'rz_mz_search')
        return out

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if self.handle:
            self.lib.rz_mz_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _mask(self, mask):
        return _ptr(mask) if mask is not None else None

    def init_roots(self, probs, noise=None, noise_frac=0.25, mask=None):
        """probs float32 [G, A] (device); noise float64 [G, A] Dirichlet samples or None; mask uint8 [G]."""
        check(self.lib.rz_mz_init_roots(self.handle, _ptr(probs), _ptr(noise) if noise is not None else None,
                                        float(noise_frac), self._mask(mask), self.stream()), 'rz_mz_init_roots')

    def select(self, mask=None):
        check(self.lib.rz_mz_select(self.handle, _ptr(self.parent), _ptr(self.action), _ptr(self.leaf),
                                    self._mask(mask), self.stream()), 'rz_mz_select')
        return self.parent, self.action, self.leaf

    def expand_backup(self, reward, probs, value, mask=None):
        check(self.lib.rz_mz_expand_backup(self.handle, _ptr(reward), _ptr(probs), _ptr(value), self._mask(mask),
                                           self.stream()), 'rz_mz_expand_backup')

    def root_visits(self):
        check(self.lib.rz_mz_root_children(self.handle, 0, _ptr(self.visits), self.stream()), 'rz_mz_root_children')
        return self.visits

    def root_children(self, what):
        """'value_sum' | 'reward' | 'prior' of the root's children, float64 [G, A]."""
        code = {'value_sum': 1, 'reward': 2, 'prior': 3}[what]
        check(self.lib.rz_mz_root_children(self.handle, code, _ptr(self.child_f64), self.stream()),
              'rz_mz_root_children')
        return self.child_f64.clone()

    def root_stats(self):
        """-> (N, value_sum, min, max) of the roots / their MinMaxStats."""
        check(self.lib.rz_mz_root_stats(self.handle, _ptr(self.root_n), _ptr(self.root_sum), _ptr(self.vmin),
                                        _ptr(self.vmax), self.stream()), 'rz_mz_root_stats')
        return self.root_n, self.root_sum, self.vmin, self.vmax

    # rz_mz_node (include/rlzero_hip.h): the 32-byte record of a tree node as the device keeps it
    NODE_DTYPE = np.dtype([('N', '<i4'), ('first_child', '<i4'), ('value_sum', '<f8'), ('prior', '<f8'), ('reward', '<f4'),
                           ('pad', '<i4')])

    def nodes(self):
        """-> (nodes, top): every game's node records, a numpy structured array [n_games, slots_per_game] (fields N,
        first_child, value_sum, prior, reward), and the slots handed out so far, int32 [n_games] (records at or past a game's
        top are stale).  Synchronises; launches nothing (tests, debugging).  After ``play_cartpole`` the trees are those of the
        launch's last move."""
        assert self.NODE_DTYPE.itemsize == 32
        nodes = np.zeros((self.n_games, self.slots_per_game), dtype=self.NODE_DTYPE)
        top = np.zeros(self.n_games, dtype=np.int32)
        check(self.lib.rz_mz_tree_nodes(self.handle, ctypes.c_void_p(nodes.ctypes.data), ctypes.c_void_p(top.ctypes.data)),
              'rz_mz_tree_nodes')
        return nodes, top

    def search_plan(self, whole_moves):
        """What a launch of ``search_fused`` (``whole_moves`` false) or ``play_env`` / ``play_cartpole`` (true; for this tree's action
        count) would be for the current shape
        (``set_search_shape``), from the host function the launch itself uses -> dict games_per_workgroup, tree_in_lds (bool),
        lds_bytes."""
        gpw, in_lds, lds = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        check(self.lib.rz_mz_search_plan(self.handle, 1 if whole_moves else 0, ctypes.byref(gpw), ctypes.byref(in_lds),
                                         ctypes.byref(lds)), 'rz_mz_search_plan')
        return {'games_per_workgroup': gpw.value, 'tree_in_lds': bool(in_lds.value), 'lds_bytes': lds.value}

    def check(self):
        flags = ctypes.c_int32(0)
        check(self.lib.rz_mz_error_flags(self.handle, ctypes.byref(flags)), 'rz_mz_error_flags')
        if flags.value:
            raise _hip.HipError('MuZero tree error flags 0x%x (tree arena full)' % flags.value)
