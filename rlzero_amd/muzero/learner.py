"""The fused MuZero learner step (rz_mz_learner_*, csrc/rz_mz_learn.hip; an opt-in route beside ``MuZeroAgent.learn``).

``MuZeroAgent.learn`` unrolls nine 64-wide ``Linear`` layers K + 1 times on a mini-batch in PyTorch: several hundred launches of
a few microseconds, two reductions per unroll step, ``clip_grad_norm_``, Adam and four ``.item()`` synchronisations.
``MuZeroFusedLearner`` runs the same arithmetic in float32 in three launches -- forward, losses and backward of a tile of batch
rows per workgroup; the fixed-order sum of the workgroups' partial gradients with the loss means; the clip and torch's
single-tensor Adam -- on the current stream, with no host synchronisation and no PyTorch operator.  The parameters are read and
written in torch's own storage (a table of 18 pointers: no second copy of the model), the two moments live in two flat tensors
owned here.  After every step the parameters' version counters are raised, so ``MuZeroSelfPlay`` / ``MuZeroReanalyser`` upload the
new weights before their next search.  No CPU fallback: HipError without a GPU.
"""
import ctypes

from .. import _hip
from .._hip import HipError

HIDDEN, MAX_OBS, MAX_ACTIONS, MAX_UNROLL = 64, 16, 8, 16
LAYERS = ('rep1', 'rep2', 'dyn1', 'dyn2', 'rew1', 'rew2', 'pre1', 'pol', 'val')   # weight and bias of each: the 18 tensors, net.parameters()'s order


def check_limits(obs_dim, n_actions, hidden, unroll_steps):
    """The fused learner's limits (the device replay's); ValueError naming the one that is exceeded.  Touches no device."""
    if int(hidden) != HIDDEN:
        raise ValueError('the fused learner is built for hidden = %d only (got hidden = %d)' % (HIDDEN, hidden))
    if not 1 <= int(obs_dim) <= MAX_OBS:
        raise ValueError('the fused learner takes obs_dim (D) in 1 .. %d (got %d)' % (MAX_OBS, obs_dim))
    if not 1 <= int(n_actions) <= MAX_ACTIONS:
        raise ValueError('the fused learner takes n_actions (A) in 1 .. %d (got %d)' % (MAX_ACTIONS, n_actions))
    if not 1 <= int(unroll_steps) <= MAX_UNROLL:
        raise ValueError('the fused learner takes unroll_steps (K) in 1 .. %d (got %d)' % (MAX_UNROLL, unroll_steps))


def n_params(obs_dim, n_actions):
    """Elements of the flat gradient / moment vectors."""
    H = HIDDEN
    return H * obs_dim + H + 5 * (H * H + H) + H * n_actions + (n_actions + 2) * (H + 1)   # rep1; rep2 dyn1 dyn2 rew1 pre1; dyn1's action columns; heads


class MuZeroFusedLearner(object):
    """``grads(batch, weights)`` -> (flat raw gradient float32 [P], losses float32 [4]); ``step(batch, weights)`` -> losses
    float32 [4] = (loss, value, reward, policy), the parameters of ``net`` and the moments updated in place.  Everything is
    enqueued on the current stream; nothing waits for it."""

    def __init__(self, net, lr=3e-3, weight_decay=1e-4, unroll_steps=5, max_batch=1024, betas=(0.9, 0.999), eps=1e-8, max_norm=5.0):
        import torch
        self.torch = torch
        check_limits(net.obs_dim, net.n_actions, net.hidden, unroll_steps)
        self.net = net
        self.params = [p for name in LAYERS for p in (getattr(net, name).weight, getattr(net, name).bias)]
        if [id(p) for p in self.params] != [id(p) for p in net.parameters()]:
            raise ValueError('the network\'s parameters are not weight and bias of %s in this order' % ' '.join(LAYERS))
        dev = self.params[0].device
        if dev.type != 'cuda' or not torch.cuda.is_available():
            raise HipError('the fused MuZero learner needs an MI355X (the network is on %s, cuda available=%s); there is no CPU fallback'
                           % (dev, torch.cuda.is_available()))
        self.device = dev
        self.lib = _hip.load()
        self.D, self.A, self.K, self.max_batch = int(net.obs_dim), int(net.n_actions), int(unroll_steps), int(max_batch)
        self.lr, self.weight_decay, self.betas, self.eps, self.max_norm = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps), float(max_norm)
        cfg = _hip.RzMzLearnerConfig(_hip.ABI_VERSION, self.D, self.A, int(net.hidden), self.K, self.max_batch, dev.index, 0, self.lr, self.weight_decay,
                                     self.betas[0], self.betas[1], self.eps, self.max_norm)
        handle = ctypes.c_void_p()
        _hip.check(self.lib.rz_mz_learner_create(ctypes.byref(cfg), ctypes.byref(handle)), 'rz_mz_learner_create')
        self.handle = handle
        got = ctypes.c_int64()
        _hip.check(self.lib.rz_mz_learner_n_params(self.handle, ctypes.byref(got)), 'rz_mz_learner_n_params')
        self.n_params = got.value
        if self.n_params != sum(p.numel() for p in self.params) or self.n_params != n_params(self.D, self.A):
            raise HipError('the library counts %d parameters, the network has %d' % (self.n_params, sum(p.numel() for p in self.params)))
        self.exp_avg = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        self.step_count = 0
        self._bound = None
        self._bind()

    def _bind(self):
        """(Re-)bind the parameters' storage if it moved (``net.to(...)``; ``load_state_dict`` copies in place and moves nothing)."""
        t = self.torch
        ptrs = tuple(p.data_ptr() for p in self.params)
        if ptrs == self._bound:
            return
        for p in self.params:
            if p.dtype != t.float32 or not p.is_contiguous() or p.device != self.device:
                raise ValueError('the fused learner needs contiguous float32 parameters on %s' % (self.device, ))
        table = (ctypes.c_void_p * len(ptrs))(*ptrs)
        _hip.check(self.lib.rz_mz_learner_bind(self.handle, table, self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()), 'rz_mz_learner_bind')
        self._bound = ptrs

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _batch(self, batch, weights):
        """The six tensors (and the weights) as the kernel reads them: on the device, contiguous, float32 / int64.  A batch of
        ``MuZeroDeviceReplay`` passes through untouched."""
        t = self.torch
        obs, actions, tv, tr, tp, mask = ((a if isinstance(a, t.Tensor) else t.from_numpy(a)).to(self.device) for a in batch)
        n = int(obs.shape[0])
        want = ((obs, t.float32, (n, self.D)), (actions, t.int64, (n, self.K)), (tv, t.float32, (n, self.K + 1)), (tr, t.float32, (n, self.K + 1)),
                (tp, t.float32, (n, self.K + 1, self.A)), (mask, t.float32, (n, self.K + 1)))
        out = []
        for x, dtype, shape in want:
            if tuple(x.shape) != shape:
                raise ValueError('a batch tensor of shape %r where the fused learner (D %d, K %d, A %d) takes %r' % (tuple(x.shape), self.D, self.K, self.A, shape))
            if x.dtype != dtype or not x.is_contiguous():
                x = x.to(dtype).contiguous()
            out.append(x)
        if not 1 <= n <= self.max_batch:
            raise ValueError('a batch of %d rows; the fused learner was built for 1 .. max_batch = %d' % (n, self.max_batch))
        if weights is not None:
            weights = (weights if isinstance(weights, t.Tensor) else t.as_tensor(weights)).to(self.device, t.float32).reshape(-1).contiguous()
            if weights.numel() != n:
                raise ValueError('%d weights for %d rows' % (weights.numel(), n))
        return out, weights, n

    def grads(self, batch, weights=None):
        """The raw gradient (before the clip) in the flat order of ``net.parameters()`` and the four loss means; updates nothing."""
        t = self.torch
        self._bind()
        tensors, weights, n = self._batch(batch, weights)
        grad = t.empty(self.n_params, dtype=t.float32, device=self.device)
        out4 = t.empty(4, dtype=t.float32, device=self.device)
        _hip.check(self.lib.rz_mz_learner_grads(self.handle, *[x.data_ptr() for x in tensors], weights.data_ptr() if weights is not None else None, n,
                                                grad.data_ptr(), out4.data_ptr(), self._stream()), 'rz_mz_learner_grads')
        return grad, out4

    def step(self, batch, weights=None):
        """One update on the current stream -> float32 [4] (loss, value, reward, policy) on the device, not synchronised."""
        t = self.torch
        self._bind()
        tensors, weights, n = self._batch(batch, weights)
        out4 = t.empty(4, dtype=t.float32, device=self.device)
        _hip.check(self.lib.rz_mz_learner_step(self.handle, *[x.data_ptr() for x in tensors], weights.data_ptr() if weights is not None else None, n,
                                               self.step_count + 1, out4.data_ptr(), self._stream()), 'rz_mz_learner_step')
        self.step_count += 1
        # the storage changed behind autograd's back: whoever compares p._version (the searches' _refresh_model) must see it
        t.autograd.graph.increment_version(self.params)
        return out4

    def poll_errors(self):
        """The device's flag word (_hip.MZ_LEARNER_BAD_ACTION), cleared by the call; waits for the stream.  The updates the device
        dropped while the flag stood (the refused one and every one behind it) are taken off the step count."""
        flags, skipped = ctypes.c_int32(), ctypes.c_int32()
        _hip.check(self.lib.rz_mz_learner_poll_errors(self.handle, ctypes.byref(flags), ctypes.byref(skipped), self._stream()), 'rz_mz_learner_poll_errors')
        self.step_count -= skipped.value
        return flags.value

    def check(self):
        """Raises if a batch since the last call held an action outside 0 .. A-1 (such a batch updated nothing)."""
        if self.poll_errors() & _hip.MZ_LEARNER_BAD_ACTION:
            raise HipError('the fused MuZero learner met an action outside 0 .. %d; that update and those behind it were not applied' % (self.A - 1))

    # ------------------------------------------------------------------ torch's Adam state_dict, both ways
    def moment_views(self):
        """[(exp_avg view, exp_avg_sq view)] per parameter, shaped like it: views of the two flat tensors."""
        out, at = [], 0
        for p in self.params:
            out.append((self.exp_avg[at:at + p.numel()].view_as(p), self.exp_avg_sq[at:at + p.numel()].view_as(p)))
            at += p.numel()
        return out

    def optimizer_state_dict(self):
        """What ``torch.optim.Adam(...).state_dict()`` holds after the same steps (``step`` a float32 scalar on the host)."""
        t = self.torch
        twin = t.optim.Adam(self.params, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        sd = twin.state_dict()
        if self.step_count:
            sd['state'] = {i: {'step': t.tensor(float(self.step_count), dtype=t.float32), 'exp_avg': m, 'exp_avg_sq': v}
                           for i, (m, v) in enumerate(self.moment_views())}
        return sd

    def load_optimizer_state_dict(self, sd):
        """Takes the moments and the step count of either route's checkpoint.  The hyper-parameters stay this learner's; a
        checkpoint made with others is refused."""
        group = sd['param_groups'][0]
        mine = {'lr': self.lr, 'betas': self.betas, 'eps': self.eps, 'weight_decay': self.weight_decay}
        for key, value in mine.items():
            got = tuple(group[key]) if key == 'betas' else float(group[key])
            if got != value:
                raise ValueError('the checkpoint\'s optimizer has %s = %r, this fused learner %r' % (key, got, value))
        if len(sd['param_groups']) != 1 or len(group['params']) != len(self.params):
            raise ValueError('the checkpoint\'s optimizer does not hold one group of %d parameters' % len(self.params))
        state = sd['state']
        if not state:
            self.exp_avg.zero_(), self.exp_avg_sq.zero_()
            self.step_count = 0
            return
        steps = set()
        for key, (m, v) in zip(group['params'], self.moment_views()):
            entry = state[key]
            m.copy_(entry['exp_avg']), v.copy_(entry['exp_avg_sq'])
            steps.add(int(entry['step']))
        if len(steps) != 1:
            raise ValueError('the checkpoint\'s parameters are at different steps: %r' % sorted(steps))
        self.step_count = steps.pop()

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.rz_mz_learner_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
