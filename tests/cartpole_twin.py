"""CartPole-v1's step for the tests of the device rules (rlzero_amd/csrc/rz_mz_env.h): the reference is oracle/muzero_ref.RefCartPole
with the time limit as an argument; the crafted states that meet each of its decisions; and the same step with one rule broken, to
show what a bound catches (no test lives here, no GPU)."""
import math

from oracle.muzero_ref import RefCartPole

X_THRESHOLD = RefCartPole.x_threshold
THETA_THRESHOLD = RefCartPole.theta_threshold_radians
VARIANTS = ('tau_0.025', 'no_four_thirds', 'force_sign')


def step(state, steps, action, max_episode_steps=500, variant=None):
    """-> (new state (4 floats), steps + 1, reward, terminated, truncated); the state is the terminal one (no reset here).
    ``variant`` None: RefCartPole itself; else its expressions with one rule broken."""
    env = RefCartPole()
    env.reset(state)
    env.steps = int(steps)
    env.max_episode_steps = int(max_episode_steps)
    if variant is None:
        new, reward, terminated, truncated = env.step(int(action))
        return new, env.steps, reward, terminated, truncated
    assert variant in VARIANTS
    x, x_dot, theta, theta_dot = env.state
    tau = 0.025 if variant == 'tau_0.025' else env.tau
    ratio = 0.0 if variant == 'no_four_thirds' else 4.0 / 3.0
    force = env.force_mag if (action == 1) != (variant == 'force_sign') else -env.force_mag
    costheta, sintheta = math.cos(theta), math.sin(theta)
    temp = (force + env.polemass_length * (theta_dot * theta_dot) * sintheta) / env.total_mass
    thetaacc = (env.gravity * sintheta - costheta * temp) / (env.length * (ratio - env.masspole * (costheta * costheta) / env.total_mass))
    xacc = temp - env.polemass_length * thetaacc * costheta / env.total_mass
    new = (x + tau * x_dot, x_dot + tau * xacc, theta + tau * theta_dot, theta_dot + tau * thetaacc)
    terminated = bool(new[0] < -X_THRESHOLD or new[0] > X_THRESHOLD or new[2] < -THETA_THRESHOLD or new[2] > THETA_THRESHOLD)
    return new, int(steps) + 1, 1.0, terminated, int(steps) + 1 >= max_episode_steps


def decision_margin(state, action):
    """How close the step from ``state`` comes to ending the episode: the smaller of ||x| - 2.4| and ||theta| - 12 degrees| behind it."""
    new, _, _, _, _ = step(state, 0, action)
    return min(abs(abs(new[0]) - X_THRESHOLD), abs(abs(new[2]) - THETA_THRESHOLD))


def crafted_states():
    """(name, state, action, terminated): one step carries x across +2.4 and across -2.4 and theta across each threshold (12 degrees =
    0.2094), or stops short of it."""
    return [
        ('x above 2.4', (2.39, 1.0, 0.0, 0.0), 1, True),
        ('x below -2.4', (-2.39, -1.0, 0.0, 0.0), 0, True),
        ('theta above its threshold', (0.0, 0.0, 0.2, 1.0), 1, True),
        ('theta below minus its threshold', (0.0, 0.0, -0.2, -1.0), 0, True),
        ('x stays inside', (2.39, 0.1, 0.0, 0.0), 0, False),
        ('theta stays inside', (0.0, 0.0, -0.2, -0.1), 1, False),
        ('upright', (0.01, -0.02, 0.03, 0.04), 1, False),
    ]
