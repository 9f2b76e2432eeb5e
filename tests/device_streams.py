"""Host restatements of the device random streams that are not parity streams (no test lives here, no GPU, numpy only):

* the AlphaZero expansion noise -- ``gamma03`` in csrc/rz_tree.h, keyed by ``mix64(mix64(noise_key[g]) ^ ctr)`` with the child's
  sub-key ``hash32(lo ^ hi) + 0x9E3779B9 * (action + 1)``; drawn, summed over the wave and mixed ``0.75 p + 0.25 eta`` in
  rz_tree.h (the in-step expansion) and twice in rz_engine.hip's headers (rz_engine_deferred.h: deferred_priors_body; rz_engine_ml.h: the level-synchronous step);
* the MuZero whole-move root noise -- ``mz_gamma`` in csrc/rz_muzero_noise.h, the same scheme with the shape as an argument and a
  floor of 1e-30, keyed by three splitmix64 rounds over (noise_seed ^ g << 24, episode, steps);
* the MuZero action draw of the whole moves -- cumulative visits ^ (1 / T) against a 53-bit uniform keyed the same way behind
  the salt 0xA5A5A5A5.

Everything is plain float64 and integer arithmetic on the device's own counters and uniforms.  ``dtype=np.float32`` evaluates the
same formulas in float32: the restatement's own model of the rounding, used only to size tolerances."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
GOLDEN32 = 0x9E3779B9
BOOST_COUNTER = 0x5bd1e995
GAMMA03_C = 0.33903103   # the literal of gamma03 (rz_tree.h), not 1 / sqrt(9 d)
ROUNDS = 8
MZ_FLOOR = 1e-30
ACTION_SALT = 0xA5A5A5A5


# ---------------------------------------------------------------------------------------------------------------------- hashes
def hash32(x):
    """rz_tree.h hash32 / rz_muzero_noise.h mz_hash32 on uint32 arrays (kept in uint64 lanes, masked after every multiply)."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def mix64(x):
    """rz_play.h mix64 (= splitmix64's output function behind one increment) on uint64 arrays."""
    with np.errstate(over='ignore'):
        x = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def splitmix64(x):
    """rz_mz_env.h splitmix64: rlzero_amd/muzero/cartpole.py's, on uint64 arrays."""
    from rlzero_amd.muzero.cartpole import _splitmix64
    with np.errstate(over='ignore'):
        return _splitmix64(np.asarray(x, dtype=np.uint64))


def _u64(x):
    return np.asarray(x).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------- the sample
def gamma_counters(keys32):
    """Every 32-bit counter a sample of key ``keys32`` may hash: key + 3 t + {0, 1, 2} for the eight rounds and key + 0x5bd1e995
    for the boost -> uint64 [..., 25]."""
    k = _u64(keys32)[..., None]
    offs = np.concatenate([np.arange(3 * ROUNDS, dtype=np.uint64), np.array([BOOST_COUNTER], dtype=np.uint64)])
    return (k + offs) & M32


def gamma(keys32, alpha, dtype=np.float64, always_boost=False, floor=0.0):
    """Marsaglia-Tsang Gamma(alpha, 1) of the device (gamma03: ``alpha=0.3, always_boost=True``; mz_gamma: ``floor=1e-30``) for every
    key of ``keys32`` -> (sample, round that accepted (8: none did, the fallback g = d), smallest margin met on the way: |rhs - lhs| of
    an acceptance test, |v| where v <= 0 rejected).  Below shape 1 (or always, for gamma03) the sample of shape alpha + 1 is boosted by
    U ^ (1 / alpha)."""
    f = dtype
    keys = _u64(keys32) & M32
    boost = always_boost or alpha < 1.0
    alpha = f(np.float32(alpha)) if not always_boost else f(alpha)   # (mz_gamma takes its shape as a float; gamma03's 0.3 is a literal)
    shape = alpha + f(1.0) if boost else alpha
    d = f(shape - f(1.0) / f(3.0))
    c = f(f(1.0) / np.sqrt(f(9.0) * d))
    if always_boost:
        # gamma03 writes its constants out: d = 1.3f - 1.0f / 3.0f and c = 0.33903103f.  That c is 2.2e-6 below 1 / sqrt(9 d) =
        # 0.33903178: a proposal scaled by 1 - 2.2e-6 under an acceptance test that assumes the exact one.  As a distribution
        # it is invisible (test_marginals_are_gamma); sample by sample a draw with a small v = 1 + c x moves by up to 4e-5.
        assert alpha == f(0.3)
        d, c = f(f(1.3) - f(1.0) / f(3.0)), f(GAMMA03_C)
    ln2, two_pi, k2m24 = f(0.69314718) if f is np.float32 else f(np.log(2.0)), f(2.0 * np.pi), f(1.0 / 16777216.0)
    g = np.full(keys.shape, d, dtype=f)
    accepted = np.full(keys.shape, ROUNDS, dtype=np.int64)
    margin = np.full(keys.shape, np.inf, dtype=np.float64)
    live = np.ones(keys.shape, dtype=bool)
    with np.errstate(divide='ignore', invalid='ignore'):
        for t in range(ROUNDS):
            if not live.any():
                break
            k = keys + np.uint64(3 * t)
            h1, h2, h3 = hash32(k), hash32(k + np.uint64(1)), hash32(k + np.uint64(2))
            u1 = ((h1 >> np.uint64(8)) + np.uint64(1)).astype(f) * k2m24    # (0, 1]
            u2 = (h2 >> np.uint64(8)).astype(f) * k2m24                      # [0, 1): a turn of the cosine
            u3 = ((h3 >> np.uint64(8)) + np.uint64(1)).astype(f) * k2m24    # (0, 1]
            x = np.sqrt(f(-2.0) * ln2 * np.log2(u1)) * np.cos(two_pi * u2)
            v = f(1.0) + c * x
            neg = v <= 0
            v3 = v * v * v
            lhs = ln2 * np.log2(u3)
            rhs = f(0.5) * x * x + d - d * v3 + d * ln2 * np.log2(np.where(neg, f(1.0), v3))
            ok = live & ~neg & (lhs < rhs)
            m = np.where(neg, np.abs(v), np.abs(rhs - lhs)).astype(np.float64)
            margin = np.where(live, np.minimum(margin, m), margin)
            g = np.where(ok, d * v3, g)
            accepted = np.where(ok, t, accepted)
            live = live & ~ok
        if boost:
            ub = ((hash32(keys + np.uint64(BOOST_COUNTER)) >> np.uint64(8)) + np.uint64(1)).astype(f) * k2m24
            g = g * np.exp2(np.log2(ub) * f(f(1.0) / alpha))   # ub ^ (1 / alpha)
    if floor > 0.0:
        g = np.maximum(g, f(floor))
    return g.astype(f), accepted, margin


# ---------------------------------------------------------------------------------------------------------------------- AlphaZero
def default_noise_key(noise_seed, g):
    """k_set_noise_keys without keys: noise_seed ^ g << 20 (the engine keeps 31 bits of its seed)."""
    return np.uint64(int(noise_seed) & 0x7FFFFFFF) ^ (_u64(g) << np.uint64(20))


def alphazero_node_key(noise_key, ctr):
    """The 32-bit key of one expansion: hash32(lo ^ hi) of mix64(mix64(noise_key) ^ ctr)."""
    key = mix64(mix64(_u64(noise_key)) ^ _u64(ctr))
    return hash32((key & M32) ^ (key >> np.uint64(32)))


def alphazero_child_keys(noise_key, ctr, actions):
    """The key of every child: node key + 0x9E3779B9 * (action + 1), the action being the child's index 64 * j + lane -- not its rank."""
    a = _u64(actions)
    return (alphazero_node_key(noise_key, ctr) + np.uint64(GOLDEN32) * (a + np.uint64(1))) & M32


def alphazero_eta_many(noise_keys, ctrs, legal, dtype=np.float64):
    """The normalised noise of many expansions in one pass: ``noise_keys`` / ``ctrs`` [n], ``legal`` a list of n ascending action
    arrays -> (list of n eta arrays, list of n margin arrays)."""
    sizes = np.array([len(a) for a in legal], dtype=np.int64)
    if len(sizes) == 0:
        return [], []
    assert (sizes > 0).all()
    acts = np.concatenate([np.asarray(a, dtype=np.int64) for a in legal])
    keys = alphazero_child_keys(np.repeat(_u64(noise_keys), sizes), np.repeat(_u64(ctrs), sizes), acts)
    g, _, margin = gamma(keys, 0.3, dtype=dtype, always_boost=True)
    first = np.cumsum(sizes) - sizes
    total = np.add.reduceat(g, first)
    total = np.where(total > 0, total, dtype(1.0))
    eta = g / np.repeat(total, sizes)
    cut = np.cumsum(sizes)[:-1]
    return np.split(eta, cut), np.split(margin, cut)


def alphazero_eta(noise_key, ctr, legal_actions, dtype=np.float64):
    """The normalised noise of ONE expansion: eta over ``legal_actions`` (ascending) -> (eta, margins)."""
    eta, margin = alphazero_eta_many([noise_key], [ctr], [legal_actions], dtype)
    return eta[0], margin[0]


# ---------------------------------------------------------------------------------------------------------------------- MuZero
def muzero_move_key(noise_seed, g, episode, steps, salt=0):
    """splitmix(splitmix(splitmix(noise_seed ^ salt ^ g << 24) ^ episode) ^ steps) on arrays."""
    k = splitmix64(np.uint64(int(noise_seed) & 0xFFFFFFFFFFFFFFFF) ^ np.uint64(salt) ^ (_u64(g) << np.uint64(24)))
    return splitmix64(splitmix64(k ^ _u64(episode)) ^ _u64(steps))


def muzero_action_keys(noise_seed, g, episode, steps, A):
    """Per-action 32-bit keys hi + 0x9E3779B9 * (a + 1) + lo -> uint64 [..., A]."""
    key = muzero_move_key(noise_seed, g, episode, steps)[..., None]
    a = np.arange(A, dtype=np.uint64)
    return ((key >> np.uint64(32)) + np.uint64(GOLDEN32) * (a + np.uint64(1)) + (key & M32)) & M32


def muzero_eta(noise_seed, g, episode, steps, A, alpha, dtype=np.float64):
    """The whole-move root noise, normalised in float64 as the kernel does (each draw floored at 1e-30)
    -> (eta [..., A], margins [..., A], draws [..., A])."""
    keys = muzero_action_keys(noise_seed, g, episode, steps, A)
    draw, _, margin = gamma(keys, alpha, dtype=dtype, floor=MZ_FLOOR)
    d64 = draw.astype(np.float64)
    return d64 / d64.sum(axis=-1, keepdims=True), margin, draw


def muzero_action(noise_seed, g, episode, steps, visits, inv_T):
    """The action of one move of the whole moves (rz_muzero_search.h, "the move"): ``visits`` int [..., A] -> (action, gap), gap =
    min_a |cum_a - target| / total (how close the draw came to a boundary; inf for an arg-max).  inv_T <= 0: the first maximum."""
    visits = np.asarray(visits, dtype=np.float64)
    A = visits.shape[-1]
    w = visits if inv_T == 1.0 or inv_T <= 0.0 else np.power(visits, inv_T)
    arg = np.argmax(w, axis=-1)   # (the first maximum: the kernel's `>` keeps the lowest index)
    if inv_T <= 0.0:
        return arg, np.full(arg.shape, np.inf)
    total = np.zeros(w.shape[:-1])
    for a in range(A):   # (the kernel's order of additions)
        total = total + w[..., a]
    key = muzero_move_key(noise_seed, g, episode, steps, salt=ACTION_SALT)
    target = ((key >> np.uint64(11)).astype(np.float64) / 9007199254740992.0) * total
    cum = np.zeros_like(total)
    action = np.full(total.shape, A - 1, dtype=np.int64)   # the fallback: no cumulative sum above the target
    found = np.zeros(total.shape, dtype=bool)
    gap = np.full(total.shape, np.inf)
    for a in range(A):
        cum = cum + w[..., a]
        hit = ~found & (cum > target)
        action = np.where(hit, a, action)
        found |= hit
        gap = np.minimum(gap, np.abs(cum - target) / np.where(total > 0, total, 1.0))
    return action, gap


# ---------------------------------------------------------------------------------------------------------------------- yardsticks
def gamma_cdf(x, alpha):
    """P(Gamma(alpha, 1) <= x) in float64 (torch.special.gammainc)."""
    import torch
    x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    return torch.special.gammainc(torch.full_like(x, float(alpha)), x).numpy()


def floor_probability(alpha, floor=MZ_FLOOR):
    """P(Gamma(alpha, 1) < floor).  Far below the regularised integral's resolution the series' first term is the value:
    floor ^ alpha / Gamma(alpha + 1) (the next term is smaller by floor * alpha / (alpha + 1))."""
    import math
    return math.exp(alpha * math.log(floor) - math.lgamma(alpha + 1.0))


def relative_spread(ref64, ref32):
    """Largest |float32 - float64| / float64 evaluation of the restatement over the entries where float64 is positive."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    ref32 = np.asarray(ref32, dtype=np.float64)
    ok = ref64 > 0
    return float(np.max(np.abs(ref32[ok] - ref64[ok]) / ref64[ok])) if ok.any() else 0.0
