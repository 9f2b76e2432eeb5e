"""The scalar twin of Acrobot-v1 (no test lives here, no GPU): pure Python, ``math.sin`` / ``math.cos``, float64, the expressions
of rlzero_amd/csrc/rz_mz_env.h in the same order -- Gymnasium's classic_control/acrobot.py, "book" dynamics, no torque noise, one
classical RK4 step of 0.2 s.  On one host CPython's float arithmetic and the header compiled without contraction call the same
libm and round every operation once, so the two agree bit for bit (tests/test_mz_env_host.py); the GPU's sin and cos are another
library's, so the kernels are held to 1e-9 (tests/test_mz_env_gpu.py).

``step(..., variant=...)`` breaks one rule on purpose ('no_k3', 'dt_over_4', 'no_half_pi', 'no_clamp'): the host test shows that
each lands far outside the GPU bound."""
import math

import numpy as np

M1 = M2 = 1.0
L1 = 1.0
LC1 = LC2 = 0.5
I1 = I2 = 1.0
G = 9.8
DT = 0.2
PI = 3.141592653589793
MAX_VEL_1 = 4.0 * PI
MAX_VEL_2 = 9.0 * PI
WRAPS = 16   # turns an angle is wrapped by at most (kAcroWraps)
VARIANTS = ('no_k3', 'dt_over_4', 'no_half_pi', 'no_clamp')


def dsdt(y, a, variant=None):
    theta1, theta2, dtheta1, dtheta2 = y
    cos, sin = math.cos, math.sin
    d1 = M1 * LC1 * LC1 + M2 * (L1 * L1 + LC2 * LC2 + 2.0 * L1 * LC2 * cos(theta2)) + I1 + I2
    d2 = M2 * (LC2 * LC2 + L1 * LC2 * cos(theta2)) + I2
    if variant == 'no_half_pi':
        phi2 = M2 * LC2 * G * cos(theta1 + theta2)
    else:
        phi2 = M2 * LC2 * G * cos(theta1 + theta2 - PI / 2.0)
    phi1 = (-M2 * L1 * LC2 * dtheta2 * dtheta2 * sin(theta2) - 2.0 * M2 * L1 * LC2 * dtheta2 * dtheta1 * sin(theta2)
            + (M1 * LC1 + M2 * L1) * G * cos(theta1 - PI / 2.0) + phi2)
    ddtheta2 = (a + d2 / d1 * phi1 - M2 * L1 * LC2 * dtheta1 * dtheta1 * sin(theta2) - phi2) / (M2 * LC2 * LC2 + I2 - d2 * d2 / d1)
    ddtheta1 = -(d2 * ddtheta2 + phi1) / d1
    return (dtheta1, dtheta2, ddtheta1, ddtheta2)


def wrap(x):
    for _ in range(WRAPS):
        if not x > PI:
            break
        x = x - 2.0 * PI
    for _ in range(WRAPS):
        if not x < -PI:
            break
        x = x + 2.0 * PI
    return x


def bound(x, m):
    return -m if x < -m else (m if x > m else x)


def integrate(state, action, variant=None):
    """The RK4 step before wrap and clamp -> the four raw values."""
    a = float(action - 1)
    y = tuple(float(v) for v in state)
    k1 = dsdt(y, a, variant)
    k2 = dsdt(tuple(y[i] + DT / 2.0 * k1[i] for i in range(4)), a, variant)
    k3 = dsdt(tuple(y[i] + DT / 2.0 * k2[i] for i in range(4)), a, variant)
    k4 = dsdt(tuple(y[i] + DT * k3[i] for i in range(4)), a, variant)
    if variant == 'no_k3':
        return tuple(y[i] + DT / 6.0 * (k1[i] + 2.0 * k2[i] + k4[i]) for i in range(4))
    if variant == 'dt_over_4':
        return tuple(y[i] + DT / 4.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) for i in range(4))
    return tuple(y[i] + DT / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) for i in range(4))


def height(state):
    return -math.cos(state[0]) - math.cos(state[1] + state[0])


def step(state, steps, action, max_episode_steps=500, variant=None):
    """-> (new state (4 floats), steps + 1, reward, terminated, truncated); the state is the terminal one (no reset here)."""
    raw = integrate(state, action, variant)
    if variant == 'no_clamp':
        new = (wrap(raw[0]), wrap(raw[1]), raw[2], raw[3])
    else:
        new = (wrap(raw[0]), wrap(raw[1]), bound(raw[2], MAX_VEL_1), bound(raw[3], MAX_VEL_2))
    steps = steps + 1
    terminated = height(new) > 1.0
    truncated = steps >= max_episode_steps
    return new, steps, (0.0 if terminated else -1.0), terminated, truncated


def decision_margin(state, action):
    """How close the step from ``state`` comes to one of its decisions: the smallest of |raw angle -/+ pi|, |height - 1| and
    |raw velocity -/+ its bound|.  A comparison between two implementations that agree to 1e-9 is meaningful only above that."""
    raw = integrate(state, action)
    new, _, _, _, _ = step(state, 0, action)
    m = [abs(abs(raw[0]) - PI), abs(abs(raw[1]) - PI), abs(abs(raw[2]) - MAX_VEL_1), abs(abs(raw[3]) - MAX_VEL_2), abs(height(new) - 1.0)]
    return min(m)


def observe(state):
    """float32 [6]: (cos theta1, sin theta1, cos theta2, sin theta2, dtheta1, dtheta2), each formed in float64."""
    return np.array([math.cos(state[0]), math.sin(state[0]), math.cos(state[1]), math.sin(state[1]), state[2], state[3]],
                    dtype=np.float64).astype(np.float32)


def crafted_states():
    """States that meet every decision of a step, as (name, state, action): an angle leaving [-pi, pi] on each side, each velocity
    bound hit on each side, and the height crossing 1.0 (the tip above the line: both links nearly upright)."""
    return [
        ('theta1 above pi', (3.1, 0.0, 3.0, 0.0), 1),
        ('theta1 below -pi', (-3.1, 0.0, -3.0, 0.0), 1),
        ('theta2 above pi', (0.0, 3.1, 0.0, 4.0), 1),
        ('theta2 below -pi', (0.0, -3.1, 0.0, -4.0), 1),
        ('dtheta1 above its bound', (-1.0, 1.33, 5.3, 24.7), 1),
        ('dtheta1 below minus its bound', (1.57, -0.17, -3.0, -16.4), 1),
        ('dtheta2 above its bound', (2.71, 2.56, -2.1, 23.5), 2),
        ('dtheta2 below minus its bound', (-0.14, -2.4, 3.8, -26.0), 0),
        ('height crosses 1', (1.17, -1.4, 7.6, 5.2), 0),
        ('height stays below 1', (0.05, -0.02, 0.01, 0.03), 1),
    ]
