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
    python tools/train_muzero.py --envs 256 --iterations 60 --device-replay --fused-learner --value-transform --eval-every 10   # rescaled targets, greedy evaluation
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
EVAL_SEED = 20191119   # the evaluation environments' seed: every evaluation of every run starts from the same states
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
                 max_episode_steps=None, whole_moves=None, value_transform=False, eval_envs=None):
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
        device moves).
        ``value_transform``: MuZero's invertible value rescaling h (arXiv:1911.08265v2 appendix F) on the scalar heads: the net is
        built with it (``MuZeroNet(value_transform=True)``), so every search inverts the heads' reward and value (inside the search
        kernel) and the buffer -- either one -- hands out h of the value and reward targets; Reanalyse reads the flag from the net.
        Off (the default), nothing changes.  ``eval_envs``: environments of ``evaluate`` (None: as many as train)."""
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
        self.value_transform = bool(value_transform)
        shape = dict(obs_dim=env_class.obs_dim, n_actions=env_class.n_actions, value_transform=self.value_transform)
        self.agent = (MuZeroAgent(device=device, fused_learner=True, unroll_steps=unroll_steps, max_batch=batch_size, **shape)
                      if self.fused_learner else MuZeroAgent(device=device, **shape))
        if env == 'cartpole':
            self.env = CartPoleBatch(n_envs, device, seed=seed)
        else:
            self.env = AcrobotBatch(n_envs, device, seed=seed, **({} if max_episode_steps is None else dict(max_episode_steps=max_episode_steps)))
        route = {} if whole_moves is None else dict(fused_moves=bool(whole_moves))
        self.selfplay = MuZeroSelfPlay(self.agent.net, self.env, n_sims=n_sims, discount=discount, seed=seed, **route)
        self._env_class, self._route, self._n_sims, self._discount, self._device = env_class, route, n_sims, discount, device
        self._max_episode_steps = max_episode_steps
        self.eval_envs = None if eval_envs is None else int(eval_envs)
        self._evaluator = None   # (MuZeroSelfPlay, its environments' count and seed): built by the first ``evaluate``
        self.device_replay = bool(device_replay)
        if self.device_replay:
            self.buffer = MuZeroDeviceReplay(self.agent.net.obs_dim, self.env.n_actions, 2000, int(self.env.max_episode_steps),
                                             unroll_steps=unroll_steps, td_steps=td_steps, discount=discount, device=device, seed=seed,
                                             prioritized=self.prioritized_replay, value_transform=self.value_transform)
        else:
            self.buffer = ReplayBuffer(unroll_steps=unroll_steps, td_steps=td_steps, discount=discount, seed=seed,
                                       value_transform=self.value_transform)
        from rlzero_amd.muzero.agent import check_value_transform
        check_value_transform(self.agent.net, self.buffer)
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

    def evaluate(self, n_envs=None, seed=EVAL_SEED):
        """A greedy evaluation of the current network -> dict(count, return_mean / return_min / return_max, length_mean /
        length_min / length_max) over exactly ``n_envs`` episodes (None: ``eval_envs``, else the training count).
        A second batch of environments of the training kind, seeded ``seed`` and restarted at every call -- every evaluation begins
        from the same ``n_envs`` initial states -- is played by a MuZeroSelfPlay of its own on the training route with
        temperature 0 (the arg-max of the visit counts) and no root noise, built once and reused (new weights reach it through its
        version check).  It plays until every environment has finished the episode that began with the evaluation's first move,
        at most max_episode_steps moves, and counts that one episode of each: later episodes of environments that finish early
        are discarded, because they would weight short episodes.  The training environments, their random streams and the replay
        are not touched.  ``self.eval_episodes``: the counted episodes, by environment."""
        from rlzero_amd.muzero import MuZeroSelfPlay
        n_envs = int(n_envs if n_envs is not None else (self.eval_envs if self.eval_envs is not None else self.env.n_envs))
        if n_envs < 1:
            raise ValueError('evaluate: n_envs must be >= 1')
        if self._evaluator is None or self._evaluator[1:] != (n_envs, int(seed)):
            if self._evaluator is not None:
                self._evaluator[0].close()
            kw = {} if self._max_episode_steps is None else dict(max_episode_steps=self._max_episode_steps)
            env = self._env_class(n_envs, self._device, seed=int(seed), **kw)
            sp = MuZeroSelfPlay(self.agent.net, env, n_sims=self._n_sims, discount=self._discount, temperature=0.0,
                                root_exploration_fraction=0.0, seed=int(seed), **self._route)
            self._evaluator = (sp, n_envs, int(seed))
        sp = self._evaluator[0]
        sp.restart_episodes()
        t0, limit = sp._t, int(sp.env.max_episode_steps)
        chunk = sp.moves_per_launch if (sp.fused_moves or sp.device_moves) else 1
        found = [None] * n_envs   # the episode of every environment that began at t0
        sp.entry_log = []
        try:
            played = 0
            while played < limit and any(ep is None for ep in found):
                k = min(chunk, limit - played)
                episodes = sp.collect(k)
                played += k
                lengths = episodes.lengths()
                where = np.concatenate([e for e, _ in sp.entry_log]) if sp.entry_log else np.zeros(0, dtype=np.int64)
                ends = np.concatenate([e for _, e in sp.entry_log]) if sp.entry_log else np.zeros(0, dtype=np.int64)
                del sp.entry_log[:]
                if len(where) != len(lengths):
                    raise RuntimeError('evaluate: %d finished episodes with %d entries' % (len(lengths), len(where)))
                for j in np.nonzero(ends - lengths == t0)[0]:
                    found[int(where[j])] = episodes[int(j)]
        finally:
            sp.entry_log = None
        if any(ep is None for ep in found):
            raise RuntimeError('evaluate: an environment did not finish its episode within max_episode_steps = %d moves' % limit)
        self.eval_episodes = found
        returns = np.array([float(np.sum(np.asarray(ep.rewards, dtype=np.float64))) for ep in found], dtype=np.float64)
        lengths = np.array([len(ep) for ep in found], dtype=np.int64)
        return dict(count=len(found), return_mean=float(returns.mean()), return_min=float(returns.min()), return_max=float(returns.max()),
                    length_mean=float(lengths.mean()), length_min=int(lengths.min()), length_max=int(lengths.max()))

    def _batch(self):
        """-> (mini-batch, importance weights or None)."""
        if self.prioritized_replay:
            return self.buffer.sample_prioritized(self.batch_size, beta=self.priority_beta)
        if self.device_replay:
            return self.buffer.sample(self.batch_size), None
        return self.buffer.sample(self.batch_size, self.env.n_actions), None

    def policy_update(self):
        from rlzero_amd.muzero.agent import check_value_transform
        check_value_transform(self.agent.net, self.buffer)   # (before any launch: the net and the buffer as they are NOW)
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

    def run(self, iterations, eval_every=0):
        """``eval_every`` N > 0: after every N-th iteration ``evaluate()`` and a line of its own; the other lines are unchanged."""
        for i in range(iterations):
            n = self.collect_selfplay_data()
            if eval_every and (i + 1) % eval_every == 0:
                ev = self.evaluate()
                print('eval i:{}, episodes:{}, return mean:{:.1f} min:{:.1f} max:{:.1f}, length mean:{:.1f} min:{} max:{}'.format(
                    i + 1, ev['count'], ev['return_mean'], ev['return_min'], ev['return_max'], ev['length_mean'], ev['length_min'],
                    ev['length_max']), flush=True)
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
    ap.add_argument('--value-transform', action='store_true',
                    help='train the scalar value and reward heads on h(x) = sign(x)(sqrt(|x| + 1) - 1) + 0.001 x of their targets and '
                         'invert them inside every search (arXiv:1911.08265v2 appendix F, without the categorical support)')
    ap.add_argument('--eval-every', type=int, default=0, metavar='N',
                    help='after every N-th iteration, a greedy evaluation (temperature 0, no root noise) on environments of its own '
                         'from fixed initial states, reported on a line of its own (0 = never)')
    ap.add_argument('--eval-envs', type=int, default=None, metavar='M', help='environments of an evaluation (default: --envs)')
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
                          env=args.env, max_episode_steps=args.max_episode_steps, whole_moves=True if args.whole_moves else None,
                          value_transform=args.value_transform, eval_envs=args.eval_envs)
    pipe.run(args.iterations, eval_every=args.eval_every)
    if args.save:
        pipe.agent.save_model(args.save)
    return pipe


if __name__ == '__main__':
    main()
