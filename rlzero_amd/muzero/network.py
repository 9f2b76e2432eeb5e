"""The learned model of MuZero (arXiv:1911.08265v2, section 3 and appendix F/G) for vector observations:
representation h(o) -> s, dynamics g(s, a) -> (r, s'), prediction f(s) -> (p, v); hidden states are
scaled to [0, 1] per sample (appendix G, "Training"), reward and value are scalar heads.

``value_transform`` / ``inverse_value_transform``: the invertible rescaling of appendix F, h(x) = sign(x) (sqrt(|x| + 1) - 1) + eps x
with eps = 0.001, and its inverse -- the torch form of csrc/rz_mz_value.h (fp64, the same expressions in the same order: the same
bits).  A ``MuZeroNet(value_transform=True)`` states that its scalar heads are trained on h of their targets and that a search has
to take their outputs through h^-1 (R2D2's use of h; the paper's categorical support is not built)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


VALUE_EPS = 0.001   # csrc/rz_mz_value.h: kEps


def _sqrt64(x):
    """The IEEE square root of a float64 tensor.  On the GPU ``torch.sqrt`` is the correctly rounded one; torch's vectorised CPU
    kernel is not (about 2 % of random arguments are an ulp off), so a CPU tensor takes numpy's, which is the hardware's."""
    if x.device.type == 'cpu':
        import numpy as np
        return torch.from_numpy(np.sqrt(x.detach().numpy()))
    return torch.sqrt(x)


def value_transform(x):
    """h(x), element by element: widened to float64, evaluated as copysign(sqrt(|x| + 1) - 1, x) + eps * x, returned in x's dtype."""
    x64 = x.to(torch.float64)
    y = torch.copysign(_sqrt64(x64.abs() + 1.0) - 1.0, x64) + VALUE_EPS * x64
    return y.to(x.dtype)


def inverse_value_transform(y):
    """h^-1(y), element by element: widened to float64, a = |y|, s = sqrt(1 + 4 eps (a + 1 + eps)), u = (s - 1) / (2 eps),
    copysign(u * u - 1, y), returned in y's dtype."""
    y64 = y.to(torch.float64)
    a = y64.abs()
    s = _sqrt64(1.0 + (4.0 * VALUE_EPS) * (a + 1.0 + VALUE_EPS))
    # (a tensor divisor: by a Python scalar the GPU kernel multiplies by the reciprocal, which is not the division's bits)
    u = (s - 1.0) / torch.full((), 2.0 * VALUE_EPS, dtype=torch.float64, device=y.device)
    return torch.copysign(u * u - 1.0, y64).to(y.dtype)


def scale_hidden(s):
    lo = s.min(dim=1, keepdim=True)[0]
    hi = s.max(dim=1, keepdim=True)[0]
    return (s - lo) / (hi - lo).clamp_min(1e-5)


class MuZeroNet(nn.Module):

    def __init__(self, obs_dim=4, n_actions=2, hidden=64, value_transform=False):
        """``value_transform``: the flag's owner -- the reward and value heads live in h's space (the learner's targets are
        transformed by the buffers, every search inverts the heads' outputs); the layers and their outputs are the same either way."""
        super().__init__()
        self.obs_dim, self.n_actions, self.hidden = obs_dim, n_actions, hidden
        self.value_transform = bool(value_transform)
        self.rep1 = nn.Linear(obs_dim, hidden)
        self.rep2 = nn.Linear(hidden, hidden)
        self.dyn1 = nn.Linear(hidden + n_actions, hidden)
        self.dyn2 = nn.Linear(hidden, hidden)
        self.rew1 = nn.Linear(hidden, hidden)
        self.rew2 = nn.Linear(hidden, 1)
        self.pre1 = nn.Linear(hidden, hidden)
        self.pol = nn.Linear(hidden, n_actions)
        self.val = nn.Linear(hidden, 1)

    def representation(self, obs):
        return scale_hidden(self.rep2(F.relu(self.rep1(obs))))

    def dynamics(self, state, action):
        """state [b, hidden], action int64 [b] -> (next state, reward [b])."""
        x = torch.cat((state, F.one_hot(action, self.n_actions).to(state.dtype)), dim=1)
        h = F.relu(self.dyn1(x))
        nxt = scale_hidden(self.dyn2(h))
        reward = self.rew2(F.relu(self.rew1(h))).squeeze(1)
        return nxt, reward

    def prediction(self, state):
        """-> (policy logits [b, A], value [b])."""
        h = F.relu(self.pre1(state))
        return self.pol(h), self.val(h).squeeze(1)

    def initial_inference(self, obs):
        s = self.representation(obs)
        logits, value = self.prediction(s)
        return s, logits, value

    def recurrent_inference(self, state, action):
        nxt, reward = self.dynamics(state, action)
        logits, value = self.prediction(nxt)
        return nxt, reward, logits, value
