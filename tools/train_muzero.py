#!/usr/bin/env python3
"""MuZero on CartPole-v1 (BASELINE.json configs[4]) or Acrobot-v1 (--env acrobot): batched self-play on the GPU
(HIP search-tree kernels + the learned model on PyTorch-ROCm), replay buffer, K = 5 unrolled training.

The reference repository names MuZero (README.md:3) but has no script for it; this one follows the layout of
its ``tools/train_alphazero.py`` (a pipeline class with ``collect_selfplay_data`` / ``policy_update`` / ``run``).

    python tools/train_muzero.py --envs 256 --iterations 60
    python tools/train_muzero.py --envs 256 --iterations 60 --device-replay   # episodes and mini-batches stay on the GPU
    python tools/train_muzero.py --envs 256 --iterations 60 --device-replay --reanalyse all   # and their targets stay fresh
    python tools/train_muzero.py --envs 256 --iterations 60 --device-replay --prioritized-replay   # steps drawn by |value - return|
    python tools/train_muzero.py --envs 256 --iterations 60 --device-replay --fused-learner   # and every update is three HIP launches
    python tools/train_muzero.py --env acrobot --envs 256 --iterations 60 --device-replay --fused-learner   # Acrobot-v1, moves kept on the device
    python tools/train_muzero.py --env acrobot --whole-moves --envs 256 --iterations 60 --device-replay --fused-learner   # ... whole moves in one launch
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

NEEDS_DEVICE_REPLAY = '--reanalyse needs --device-replay: the steps are searched again and refreshed where they are stored, on the GPU'
ENVIRONMENTS = ('cartpole', 'acrobot')
PRIORITIES_NEED_DEVICE_REPLAY = ('--prioritized-replay needs --device-replay: the priorities are kept beside the stored steps, '
                                 'on the GPU')


def reanalyse_arg(text):
    """--reanalyse N|all -> 0 (off), a number of positions per iteration, or 'all'."""
    if text == 'all':
        return text
    n = int(text)
    if n < 0:
        raise argparse.ArgumentTypeError('a number of positions >= 0, or all')
    return n


class MuZeroPipeline(object):

    def __init__(self, n_envs=256, n_sims=50, unroll_steps=5, td_steps=10, discount=0.997, batch_size=256,
                 moves_per_iteration=20, updates_per_iteration=40, device='cuda:0', seed=0, device_replay=False, reanalyse=0,
                 reanalyse_batch=2048, prioritized_replay=False, priority_beta=1.0, fused_learner=False, env='cartpole',
                 max_episode_steps=None, whole_moves=None):
        """``device_replay``: finished episodes go to a MuZeroDeviceReplay (whole moves hand them over on the device) and every
        mini-batch is one launch there; otherwise the host ReplayBuffer, as before.
        ``reanalyse`` (needs ``device_replay``): before the updates of an iteration that many stored steps, drawn on the device
        (or, 'all', every step held), are searched again with the current network and their policy and root value refreshed
        (MuZeroReanalyser: a second, small search object; the self-play object and its counters are not touched).  0: off.
        ``prioritized_replay`` (needs ``device_replay``): mini-batches are drawn in proportion to |search value - n-step return|
        of the stored steps (MuZeroDeviceReplay.sample_prioritized) and the loss of an entry is scaled by its importance weight
        (1 / (N P)) ** ``priority_beta``; a Reanalyse moves the priorities with the root values it rewrites.
        ``fused_learner``: the updates run in the HIP learner (MuZeroAgent(fused_learner=True)): ``policy_update`` enqueues all of
        them and reads only the last result.  Works with either buffer and with every option above.
        ``env``: 'cartpole' (CartPoleBatch: whole moves in one launch) or 'acrobot' (AcrobotBatch: 3 actions, 6 observations, reward -1
        per step; moves kept on the device, MuZeroSelfPlay(device_moves=...)).  The agent, the buffers, Reanalyse and the learner are
        built for the environment's shape.  ``max_episode_steps`` (Acrobot only): its time limit, None = the environment's 500.
        ``whole_moves``: True asks for whole moves in one launch (MuZeroSelfPlay(fused_moves=True)) whatever the environment, and is
        refused with a ValueError where they cannot run; None = the environment's default route (CartPole: whole moves, Acrobot:
        device moves)."""
        if env not in ENVIRONMENTS:
            raise ValueError('unknown environment %r (known: %s)' % (env, ', '.join(ENVIRONMENTS)))
        if max_episode_steps is not None and env == 'cartpole':
            raise ValueError('max_episode_steps is Acrobot\'s: CartPole-v1\'s 500 steps are part of the whole-move kernel')
        self.env_name = env
        self.fused_learner = bool(fused_learner)
        self.prioritized_replay, self.priority_beta = bool(prioritized_replay), float(priority_beta)
        if self.prioritized_replay and not device_replay:
            raise ValueError(PRIORITIES_NEED_DEVICE_REPLAY)
        self.reanalyse = reanalyse if reanalyse == 'all' else int(reanalyse or 0)
        if self.reanalyse and not device_replay:
            raise ValueError(NEEDS_DEVICE_REPLAY)
        from rlzero_amd.muzero import (AcrobotBatch, CartPoleBatch, MuZeroAgent, MuZeroDeviceReplay, MuZeroReanalyser, MuZeroSelfPlay,
                                       ReplayBuffer)
        env_class = {'cartpole': CartPoleBatch, 'acrobot': AcrobotBatch}[env]
        shape = dict(obs_dim=env_class.obs_dim, n_actions=env_class.n_actions)
        self.agent = (MuZeroAgent(device=device, fused_learner=True, unroll_steps=unroll_steps, max_batch=batch_size, **shape)
                      if self.fused_learner else MuZeroAgent(device=device, **shape))
        if env == 'cartpole':
            self.env = CartPoleBatch(n_envs, device, seed=seed)
        else:
            self.env = AcrobotBatch(n_envs, device, seed=seed, **({} if max_episode_steps is None else dict(max_episode_steps=max_episode_steps)))
        route = {} if whole_moves is None else dict(fused_moves=bool(whole_moves))
        self.selfplay = MuZeroSelfPlay(self.agent.net, self.env, n_sims=n_sims, discount=discount, seed=seed, **route)
        self.device_replay = bool(device_replay)
        if self.device_replay:
            self.buffer = MuZeroDeviceReplay(self.agent.net.obs_dim, self.env.n_actions, 2000, int(self.env.max_episode_steps),
                                             unroll_steps=unroll_steps, td_steps=td_steps, discount=discount, device=device, seed=seed,
                                             prioritized=self.prioritized_replay)
        else:
            self.buffer = ReplayBuffer(unroll_steps=unroll_steps, td_steps=td_steps, discount=discount, seed=seed)
        self.reanalyser = None
        if self.reanalyse:
            self.reanalyser = MuZeroReanalyser(self.agent.net, self.buffer, n_sims=n_sims, batch=reanalyse_batch, discount=discount, seed=seed)
        self.batch_size = batch_size
        self.moves_per_iteration = moves_per_iteration
        self.updates_per_iteration = updates_per_iteration
        self.episode_len = 0.0
        self._episode_return, self._returns_of = 0.0, None

    def collect_selfplay_data(self):
        if self.device_replay:
            episodes = self.selfplay.collect(self.moves_per_iteration, replay=self.buffer)
            if episodes:
                self.episode_len = float(np.mean(episodes.lengths()))
                self._keep_for_returns(episodes)
            return len(episodes)
        episodes = self.selfplay.collect(self.moves_per_iteration)
        for ep in episodes:
            self.buffer.add(ep)
        if episodes:
            self.episode_len = float(np.mean([len(ep) for ep in episodes]))
            self._keep_for_returns(episodes)
        return len(episodes)

    def _keep_for_returns(self, episodes):
        # CartPole pays 1 per step: the return IS the length, and the iteration's episodes (8192 environments: 13 MB of records) are
        # not kept alive for a figure nobody has to form
        if self.env_name == 'cartpole':
            self._episode_return, self._returns_of = self.episode_len, None
        else:
            self._returns_of = episodes

    @property
    def episode_return(self):
        """Mean sum of rewards of the last iteration's finished episodes (CartPole: = episode_len), formed when it is read."""
        if self._returns_of is not None:
            self._episode_return, self._returns_of = float(np.mean(self._returns_of.returns())), None
        return self._episode_return

    def reanalyse_targets(self):
        """-> the number of stored steps refreshed (0 when off)."""
        if self.reanalyser is None:
            return 0
        return self.reanalyser.reanalyse_all() if self.reanalyse == 'all' else self.reanalyser.reanalyse_sample(self.reanalyse)

    def _batch(self):
        """-> (mini-batch, importance weights or None)."""
        if self.prioritized_replay:
            return self.buffer.sample_prioritized(self.batch_size, beta=self.priority_beta)
        if self.device_replay:
            return self.buffer.sample(self.batch_size), None
        return self.buffer.sample(self.batch_size, self.env.n_actions), None

    def policy_update(self):
        out = (0.0, 0.0, 0.0, 0.0)
        if self.fused_learner:   # every update enqueued behind the last; one read at the end
            last = None
            for _ in range(self.updates_per_iteration):
                batch, weights = self._batch()
                last = self.agent.learn_async(batch, weights=weights)
            if last is not None:
                out = tuple(last.tolist())
                self.agent.check()
            return out
        for _ in range(self.updates_per_iteration):
            if self.prioritized_replay:
                batch, weights = self.buffer.sample_prioritized(self.batch_size, beta=self.priority_beta)
                out = self.agent.learn(batch, weights=weights)
            elif self.device_replay:
                out = self.agent.learn(self.buffer.sample(self.batch_size))
            else:
                out = self.agent.learn(self.buffer.sample(self.batch_size, self.env.n_actions))
        return out

    def run(self, iterations):
        for i in range(iterations):
            n = self.collect_selfplay_data()
            if len(self.buffer) < 8:
                continue
            refreshed = self.reanalyse_targets()
            loss, lv, lr_, lp = self.policy_update()
            # (CartPole's line is the one its logs have always had: there the return IS the length)
            returns = '' if self.env_name == 'cartpole' else ' episode_return:{:.1f},'.format(self.episode_return)
            print('batch i:{}, episodes:{}, episode_len:{:.1f},{} loss:{:.4f}, value:{:.4f}, reward:{:.4f}, '
                  'policy:{:.4f}'.format(i + 1, n, self.episode_len, returns, loss, lv, lr_, lp)
                  + (', reanalysed:{}'.format(refreshed) if self.reanalyser is not None else ''), flush=True)
        return self.episode_len


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--env', choices=ENVIRONMENTS, default='cartpole',
                    help='the environment: CartPole-v1 (whole moves in one launch) or Acrobot-v1 (moves kept on the device)')
    ap.add_argument('--max-episode-steps', type=int, default=None, metavar='N', help='time limit of an Acrobot episode (default: 500)')
    ap.add_argument('--whole-moves', action='store_true',
                    help='whole moves in one launch for the chosen environment (CartPole\'s default; Acrobot: instead of device moves)')
    ap.add_argument('--envs', type=int, default=256)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--iterations', type=int, default=60)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--save', default='')
    ap.add_argument('--device-replay', action='store_true', help='keep the replay buffer and the target formation on the GPU')
    ap.add_argument('--batch-size', type=int, default=256)
    ap.add_argument('--updates-per-iteration', type=int, default=40)
    ap.add_argument('--reanalyse', type=reanalyse_arg, default=0, metavar='N|all',
                    help='per iteration, search N stored steps (or all of them) again with the current network and refresh their targets '
                         '(needs --device-replay; 0 = off)')
    ap.add_argument('--prioritized-replay', action='store_true',
                    help='draw mini-batches in proportion to |search value - n-step return| of the stored steps and scale the loss by the '
                         'importance weights (needs --device-replay)')
    ap.add_argument('--priority-beta', type=float, default=1.0, metavar='B', help='exponent of the importance weights (1 / (N P)) ** B')
    ap.add_argument('--fused-learner', action='store_true',
                    help='run every update in the HIP learner: forward, backward, clip and Adam in three launches, no host synchronisation')
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.reanalyse and not args.device_replay:
        ap.error(NEEDS_DEVICE_REPLAY)
    if args.prioritized_replay and not args.device_replay:
        ap.error(PRIORITIES_NEED_DEVICE_REPLAY)
    pipe = MuZeroPipeline(n_envs=args.envs, n_sims=args.sims, device=args.device, batch_size=args.batch_size,
                          updates_per_iteration=args.updates_per_iteration, device_replay=args.device_replay, reanalyse=args.reanalyse,
                          prioritized_replay=args.prioritized_replay, priority_beta=args.priority_beta, fused_learner=args.fused_learner,
                          env=args.env, max_episode_steps=args.max_episode_steps, whole_moves=True if args.whole_moves else None)
    pipe.run(args.iterations)
    if args.save:
        pipe.agent.save_model(args.save)
    return pipe


if __name__ == '__main__':
    main()
