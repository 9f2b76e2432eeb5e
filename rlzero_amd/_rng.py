"""The 64-bit mix every keyed random stream of the package is built from, once: the host's copy of csrc/rz_rng.h (mix64), in the two
forms the restatements of the device's draws use.  The salts and the chains stay with the streams they name (selfplay.py, replay.py,
muzero/replay.py, muzero/reanalyse.py, muzero/cartpole.py, muzero/acrobot.py, mcts/rollout_mcts.py)."""
import numpy as np

MASK = (1 << 64) - 1
_INCREMENT, _MUL1, _MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB   # splitmix64's constants
_MASK_U64 = np.uint64(MASK)


def mix64(x):
    """The splitmix64 finaliser of a Python integer in 0 .. 2^64 - 1 -> a Python integer."""
    x = (x + _INCREMENT) & MASK
    z = x
    z = ((z ^ (z >> 30)) * _MUL1) & MASK
    z = ((z ^ (z >> 27)) * _MUL2) & MASK
    return z ^ (z >> 31)


def mix64_u64(x):
    """The same mix of a numpy ``uint64`` scalar or array, element by element (the sums and products wrap: call it under
    ``np.errstate(over='ignore')``)."""
    x = (x + np.uint64(_INCREMENT)) & _MASK_U64
    z = x
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(_MUL1)) & _MASK_U64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(_MUL2)) & _MASK_U64
    return z ^ (z >> np.uint64(31))
