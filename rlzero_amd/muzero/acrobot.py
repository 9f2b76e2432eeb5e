"""Acrobot-v1 for many environments at once, on the device (float64 state, float32 observations).

Gymnasium's ``AcrobotEnv`` (``gymnasium/envs/classic_control/acrobot.py``: the "book" dynamics of Sutton and Barto, no torque
noise; two links of length 1 and mass 1, torque -1 / 0 / +1 on the joint between them, one classical RK4 step of 0.2 s per move,
the angles wrapped into [-pi, pi], the velocities bounded by 4 pi and 9 pi; reward -1 per step and 0 for the step that lifts the
tip one link above the base, which ends the episode) with the 500-step time limit of the ``Acrobot-v1`` registration.  Gymnasium is
not available offline; the constants and the order of the operations are the published ones, written out in csrc/rz_mz_env.h (the
definition the kernels run) and restated in scalar Python by the tests.  Finished environments are reset in place (auto-reset),
initial states are uniform in [-0.1, 0.1)^4 from the counter-based stream of ``cartpole.py`` keyed (seed, environment, episode).

The observation is not the state: (cos theta1, sin theta1, cos theta2, sin theta2, dtheta1, dtheta2), each formed in float64."""
import ctypes

import numpy as np

from .._rng import mix64_u64 as _splitmix64

MAX_EPISODE_STEPS = 500


def acrobot_initial_states(seed, env_ids, episodes):
    """float64 [n, 4] in [-0.1, 0.1): counter-based, reproducible on any host (``cartpole.initial_states`` with Acrobot's range)."""
    env_ids = np.atleast_1d(np.asarray(env_ids)).astype(np.uint64)
    episodes = np.atleast_1d(np.asarray(episodes)).astype(np.uint64)
    with np.errstate(over='ignore'):
        key = _splitmix64(_splitmix64(np.uint64(int(seed) & (2 ** 64 - 1)) ^ (env_ids << np.uint64(24))) ^ episodes)
        out = np.empty((len(env_ids), 4), dtype=np.float64)
        for j in range(4):
            u = (_splitmix64(key ^ np.uint64(j + 1)) >> np.uint64(11)).astype(np.float64) / float(1 << 53)
            out[:, j] = -0.1 + 0.2 * u
    return out


class AcrobotBatch(object):
    """The environments live on the device, as ``CartPoleBatch``'s do: ``state`` float64 [n, 4] (theta1, theta2, dtheta1,
    dtheta2), ``steps`` / ``episode_dev`` int64 [n]; a step of all of them (RK4, termination, auto-reset) is ONE kernel launch
    (csrc/rz_muzero_moves.h k_mz_env_step) and never synchronises with the host.  MuZero's device moves (MuZeroTree.env_move) step the
    same tensors in place."""
    n_actions = 3
    obs_dim = 6
    kind = 'acrobot'

    def __init__(self, n_envs, device='cuda:0', seed=0, max_episode_steps=MAX_EPISODE_STEPS):
        import torch
        from .. import _hip
        self.torch = torch
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('AcrobotBatch runs on the GPU (device=%r)' % (device, ))
        if int(max_episode_steps) < 1:
            raise ValueError('max_episode_steps must be >= 1')
        self.lib = _hip.load()
        self._kind = _hip.MZ_ENV_KINDS[self.kind]
        self.n_envs, self.seed, self.max_episode_steps = int(n_envs), int(seed), int(max_episode_steps)
        kw = dict(device=self.device)
        self.state = torch.zeros((n_envs, 4), dtype=torch.float64, **kw)
        self.steps = torch.zeros(n_envs, dtype=torch.int64, **kw)
        self.episode_dev = torch.zeros(n_envs, dtype=torch.int64, **kw)
        self._obs = torch.zeros((n_envs, self.obs_dim), dtype=torch.float32, **kw)
        self._reward = torch.zeros(n_envs, dtype=torch.float32, **kw)
        self._terminated = torch.zeros(n_envs, dtype=torch.uint8, **kw)
        self._truncated = torch.zeros(n_envs, dtype=torch.uint8, **kw)
        self.reset_all()

    @property
    def episode(self):
        """Episode index of every environment (host copy)."""
        return self.episode_dev.cpu().numpy()

    def reset_all(self):
        self.set_states(acrobot_initial_states(self.seed, np.arange(self.n_envs), self.episode))

    def set_states(self, states, mask=None):
        t = self.torch
        new = t.from_numpy(np.ascontiguousarray(states, dtype=np.float64)).to(self.device)
        if mask is None:
            self.state.copy_(new)
            self.steps.zero_()
        else:
            m = t.from_numpy(np.ascontiguousarray(mask, dtype=np.bool_)).to(self.device)
            self.state[m] = new[m]
            self.steps[m] = 0

    def _launch(self, actions):
        from ..engine import _ptr, check
        stream = ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)
        check(self.lib.rz_mz_env_step(self._kind, _ptr(self.state), _ptr(self.steps), _ptr(self.episode_dev),
                                      _ptr(actions) if actions is not None else None, self.n_envs, self.seed & (2 ** 64 - 1),
                                      self.max_episode_steps, _ptr(self._obs), _ptr(self._reward), _ptr(self._terminated),
                                      _ptr(self._truncated), stream), 'rz_mz_env_step')

    def observe(self):
        """float32 [n, 6] of the current states, formed by the kernel that forms a step's (one definition of the observation)."""
        self._launch(None)
        return self._obs.clone()

    def step(self, actions):
        """actions int64 [n] on the device (0, 1, 2 = torque -1, 0, +1) -> (obs float32 [n, 6] AFTER auto-reset, reward float32
        [n], terminated bool [n], truncated bool [n]); the observation of a finished environment is the first of its next
        episode."""
        actions = actions.to(self.torch.int64).contiguous()
        self._launch(actions)
        return self._obs.clone(), self._reward.clone(), self._terminated.bool(), self._truncated.bool()
