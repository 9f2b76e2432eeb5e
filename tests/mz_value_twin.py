"""The Python twin of rlzero_amd/csrc/rz_mz_value.h: MuZero's invertible value transform in CPython floats (fp64, one rounding per
operation, ``math.sqrt`` / ``math.copysign``), the arbiter of the header, of the torch functions of rlzero_amd/muzero/network.py and
of what the kernels write (tests/test_mz_value_transform_host.py, tests/test_mz_value_transform_gpu.py)."""
import math

import numpy as np

EPS = 0.001


def value_h(x):
    x = float(x)
    return math.copysign(math.sqrt(abs(x) + 1.0) - 1.0, x) + EPS * x


def value_h_inv(y):
    y = float(y)
    a = abs(y)
    s = math.sqrt(1.0 + 4.0 * EPS * (a + 1.0 + EPS))
    u = (s - 1.0) / (2.0 * EPS)
    return math.copysign(u * u - 1.0, y)


def h_array(x):
    """value_h of every element, float64 in the input's shape."""
    x = np.asarray(x, dtype=np.float64)
    return np.array([value_h(v) for v in x.reshape(-1)], dtype=np.float64).reshape(x.shape)


def h_inv_array(y):
    y = np.asarray(y, dtype=np.float64)
    return np.array([value_h_inv(v) for v in y.reshape(-1)], dtype=np.float64).reshape(y.shape)


def h_f32(x):
    """What a float32 holder gets: widened, transformed, rounded once."""
    return h_array(np.asarray(x, dtype=np.float32).astype(np.float64)).astype(np.float32)


def h_inv_f32(y):
    return h_inv_array(np.asarray(y, dtype=np.float32).astype(np.float64)).astype(np.float32)
