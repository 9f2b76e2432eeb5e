"""MuZero's categorical support for values and rewards (arXiv:1911.08265v2 appendix F): the Python twin of csrc/rz_mz_support.h, and
the arbiter of it -- the same operations in the same order in float64, so the C++ header gives the same bits on the host
(tests/test_mz_support_host.py).

A support of half-width ``S`` (1 .. 31) has ``B = 2 S + 1`` bins at the integers -S .. S.  ``two_hot`` spreads a number over the two
bins next to it; ``support_expectation`` reads a head's logits back as a number: softmax with the maximum subtracted, then
sum p_i (i - S), the sums taken in the header's one order (four chunks of 16 bins left to right, then (c0 + c1) + (c2 + c3)).
Both live in the transformed space of ``network.value_transform``: targets are ``two_hot(h(z))``, a search uses
``inverse_value_transform(support_expectation(logits))``.

``two_hot_torch`` / ``expectation_torch`` are the differentiable torch forms the model and the learner use (any float dtype)."""
import math

import numpy as np

MIN_SUPPORT, MAX_SUPPORT = 1, 31
_CHUNK, _CHUNKS = 16, 4


def check_support(S):
    """-> int(S); ValueError unless 1 <= S <= 31 (B = 2 S + 1 <= 63: one bin per lane of a wave in the search kernel)."""
    if isinstance(S, bool) or int(S) != S or not MIN_SUPPORT <= int(S) <= MAX_SUPPORT:
        raise ValueError('support must be an integer in %d .. %d (2 S + 1 bins, at most 63), not %r' % (MIN_SUPPORT, MAX_SUPPORT, S))
    return int(S)


def two_hot(y, S):
    """y (any shape) -> (lo_bin int64, w_lo float64, w_hi float64), element by element: y clamped to [-S, S] (nan: -S), lo =
    floor(y), w_hi = y - lo on bin lo_bin + 1, w_lo = 1 - w_hi on bin lo_bin = lo + S.  At y == S, lo_bin is the last bin and w_hi 0."""
    S = check_support(S)
    y = np.asarray(y, dtype=np.float64)
    s = np.float64(S)
    y = np.where(y > -s, y, -s)
    y = np.where(y < s, y, s)
    lo = np.floor(y)
    w_hi = y - lo
    return lo.astype(np.int64) + S, np.float64(1.0) - w_hi, w_hi


def two_hot_dense(y, S):
    """``two_hot`` as float64 [..., B] rows."""
    lo, w_lo, w_hi = two_hot(y, S)
    out = np.zeros(lo.shape + (2 * S + 1, ), dtype=np.float64)
    flat, lo_f, wl, wh = out.reshape(-1, 2 * S + 1), lo.reshape(-1), w_lo.reshape(-1), w_hi.reshape(-1)
    for r in range(flat.shape[0]):
        flat[r, lo_f[r]] = wl[r]
        if wh[r] > 0.0:
            flat[r, lo_f[r] + 1] = wh[r]
    return out


def _expectation_row(x, S):
    B = 2 * S + 1
    m = -math.inf
    for i in range(B):
        v = float(x[i])
        m = v if v > m else m
    den, num = [], []
    for c in range(_CHUNKS):
        d, u = 0.0, 0.0
        for j in range(_CHUNK):
            i = _CHUNK * c + j
            e = math.exp(float(x[i]) - m) if i < B else 0.0   # (math.exp: the host libm's, which the header calls)
            d = d + e
            u = u + e * float(i - S)
        den.append(d)
        num.append(u)
    return ((num[0] + num[1]) + (num[2] + num[3])) / ((den[0] + den[1]) + (den[2] + den[3]))


def support_expectation(logits, S):
    """logits [..., B] (widened to float64 value by value) -> float64 [...]: the header's ``expectation``, bit for bit."""
    S = check_support(S)
    x = np.asarray(logits)
    if x.shape[-1] != 2 * S + 1:
        raise ValueError('support %d has %d bins, the logits have %d' % (S, 2 * S + 1, x.shape[-1]))
    flat = x.reshape(-1, x.shape[-1])
    return np.array([_expectation_row(row, S) for row in flat], dtype=np.float64).reshape(x.shape[:-1])


def two_hot_torch(y, S):
    """torch: y [...] -> [..., B] two-hot rows in y's dtype (the clamp and floor of ``two_hot``); no gradient flows into a target."""
    import torch
    y = y.detach().clamp(-float(S), float(S))
    lo = torch.floor(y)
    w_hi = y - lo
    idx = lo.long() + S
    out = torch.zeros(y.shape + (2 * S + 1, ), dtype=y.dtype, device=y.device)
    out.scatter_(-1, idx.unsqueeze(-1), (1.0 - w_hi).unsqueeze(-1))
    out.scatter_add_(-1, (idx + 1).clamp_max(2 * S).unsqueeze(-1), w_hi.unsqueeze(-1))   # (at y == S: + 0 on the last bin)
    return out


def expectation_torch(logits, S):
    """torch: logits [..., B] -> [...] = sum softmax(logits)_i (i - S) in the logits' dtype (differentiable; torch's own order)."""
    import torch
    bins = torch.arange(-S, S + 1, dtype=logits.dtype, device=logits.device)
    return (torch.softmax(logits, dim=-1) * bins).sum(dim=-1)
