"""MuZero learner: K-step unrolled training of the learned model (arXiv:1911.08265v2, appendix G and the
pseudocode's ``update_weights``): value and reward by squared error (scalar heads), policy by cross-entropy
against the search visit distribution, gradient of the unrolled steps scaled by 1/K, the gradient flowing into
the dynamics function halved at every step.

``fused_learner=True`` (opt-in): the same update as three HIP launches without a host synchronisation (learner.py:
MuZeroFusedLearner; csrc/rz_mz_learn.hip).  ``learn`` below stays the definition of the arithmetic and the default."""
import torch
import torch.nn.functional as F

from .network import MuZeroNet


def check_value_transform(net, buffer):
    """ValueError unless the net and the buffer agree on the value transform: a net whose heads live in h's space must be trained
    on transformed targets and the other way round (a buffer without the attribute counts as one without the transform)."""
    want, got = bool(getattr(net, 'value_transform', False)), bool(getattr(buffer, 'value_transform', False))
    if want != got:
        raise ValueError('the net has value_transform=%s but the buffer (%s) has value_transform=%s: the targets of a mini-batch and '
                         'the heads they train must be in the same space' % (want, type(buffer).__name__, got))


def scale_gradient(x, scale):
    return x * scale + x.detach() * (1.0 - scale)


class MuZeroAgent(object):

    def __init__(self, obs_dim=4, n_actions=2, hidden=64, lr=3e-3, weight_decay=1e-4, device='cuda:0', fused_learner=False, unroll_steps=5,
                 max_batch=1024, value_transform=False):
        """``value_transform``: passed on to the net (``MuZeroNet(value_transform=...)``, the flag's owner): the mini-batches must
        then come from a buffer built with it (``learn(batch, buffer=...)`` checks), and a checkpoint carries the setting.
        ``fused_learner``: updates run in the HIP learner (hidden 64, obs_dim <= 16, n_actions <= 8, unroll_steps <= 16: a
        ValueError names the limit before anything is allocated); ``unroll_steps`` and ``max_batch`` size it (batches of K =
        unroll_steps and up to max_batch rows) and mean nothing to the PyTorch route.  The route is fixed for the agent's life; a
        checkpoint moves between the routes."""
        self.fused_learner = bool(fused_learner)
        if self.fused_learner:
            from .learner import check_limits
            check_limits(obs_dim, n_actions, hidden, unroll_steps)
        self.device = torch.device(device)
        self.n_actions = n_actions
        self.net = MuZeroNet(obs_dim, n_actions, hidden, value_transform=value_transform).to(self.device)
        self.optimizer = None
        self.fused = None
        if self.fused_learner:
            from .learner import MuZeroFusedLearner
            self.net.eval()
            self.fused = MuZeroFusedLearner(self.net, lr=lr, weight_decay=weight_decay, unroll_steps=unroll_steps, max_batch=max_batch)
        else:
            self.optimizer = torch.optim.Adam(self.net.parameters(), lr=lr, weight_decay=weight_decay)

    def learn_async(self, batch, weights=None, buffer=None):
        """One fused update enqueued on the current stream -> float32 [4] on the device: (loss, value loss, reward loss, policy
        loss).  Nothing is synchronised; read the result (or call ``check``) when it is needed.  ``buffer``: as ``learn``'s."""
        if self.fused is None:
            raise RuntimeError('learn_async is the fused learner\'s (MuZeroAgent(fused_learner=True)); this agent learns through PyTorch')
        if buffer is not None:
            check_value_transform(self.net, buffer)
        return self.fused.step(batch, weights)

    def check(self):
        """Fused route: raises if an update since the last call met an action outside 0 .. A-1 (it changed no parameter)."""
        if self.fused is not None:
            self.fused.check()

    def learn(self, batch, weights=None, buffer=None):
        """batch = ReplayBuffer.sample(...) (numpy arrays) or MuZeroDeviceReplay.sample(...) (device tensors, taken as they are)
        -> (loss, value loss, reward loss, policy loss) floats.  ``weights`` [b] (MuZeroDeviceReplay.sample_prioritized): the
        importance weights of prioritized replay, a factor on every entry's loss before the mean (appendix G); the three
        component losses returned stay unweighted.  ``buffer``: the buffer the batch came from; its ``value_transform`` must be
        the net's (a ValueError that names both, before anything is launched).  The batch itself is taken as it comes."""
        if buffer is not None:
            check_value_transform(self.net, buffer)
        if self.fused is not None:
            return tuple(self.learn_async(batch, weights).tolist())
        obs, actions, tv, tr, tp, mask = ((a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).to(self.device) for a in batch)
        K = actions.shape[1]
        net = self.net
        net.train()
        state, logits, value = net.initial_inference(obs)
        lv = F.mse_loss(value, tv[:, 0], reduction='none')
        lr_ = torch.zeros_like(lv)
        lp = -(tp[:, 0] * F.log_softmax(logits, dim=1)).sum(dim=1) * mask[:, 0]
        for k in range(1, K + 1):
            state, reward, logits, value = net.recurrent_inference(state, actions[:, k - 1])
            g = 1.0 / K
            lv = lv + scale_gradient(F.mse_loss(value, tv[:, k], reduction='none'), g)
            lr_ = lr_ + scale_gradient(F.mse_loss(reward, tr[:, k], reduction='none'), g)
            lp = lp + scale_gradient(-(tp[:, k] * F.log_softmax(logits, dim=1)).sum(dim=1) * mask[:, k], g)
            state = scale_gradient(state, 0.5)
        if weights is None:
            loss = (0.25 * lv + lr_ + lp).mean()
        else:
            weights = (weights if isinstance(weights, torch.Tensor) else torch.as_tensor(weights)).to(self.device, torch.float32)
            loss = ((0.25 * lv + lr_ + lp) * weights).mean()
        self.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 5.0)
        self.optimizer.step()
        net.eval()
        return float(loss.item()), float(lv.mean().item()), float(lr_.mean().item()), float(lp.mean().item())

    def save_model(self, path):
        """Either route writes torch's Adam ``state_dict`` (the fused one: views of its flat moments, ``step`` as torch stores it)."""
        opt = self.fused.optimizer_state_dict() if self.fused is not None else self.optimizer.state_dict()
        ck = {'model': self.net.state_dict(), 'optimizer': opt}
        if self.net.value_transform:   # (written only when on: a checkpoint without the option is what it always was)
            ck['value_transform'] = True
        torch.save(ck, path)

    def load_model(self, path):
        """Reads either route's file."""
        ck = torch.load(path, map_location=self.device)
        saved = bool(ck.get('value_transform', False))
        if saved != self.net.value_transform:
            raise ValueError('the checkpoint %s was saved with value_transform=%s, this agent\'s net has value_transform=%s: the reward '
                             'and value heads would be read in the wrong space' % (path, saved, self.net.value_transform))
        self.net.load_state_dict(ck['model'])
        if self.fused is not None:
            self.fused.load_optimizer_state_dict(ck['optimizer'])
        else:
            self.optimizer.load_state_dict(ck['optimizer'])
