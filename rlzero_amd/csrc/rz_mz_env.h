// rz_mz_env.h -- the rules of the MuZero environments and of the moves kept on the device (rz_muzero_search.h: k_mz_search's MOVES stages; rz_muzero_moves.h:
// k_mz_env_step, k_mz_env_move, k_mz_root_noise; include/rlzero_hip.h: rz_mz_play_cartpole, rz_cartpole_step, rz_mz_env_step,
// rz_mz_env_move, rz_mz_root_noise): everything about them that is neither a kernel launch nor a memory access.  Plain C++, no HIP
// include, so that the CPU can run it against the scalar restatements of CartPole, Acrobot, the keys and the draw
// (tests/test_mz_env_host.py); the kernels call these functions.  fp64, one rounding per operation (-ffp-contract=off), the
// expressions in the order the restatements write them: on one host, with one libm, the two give the same bits.
//
// An environment is a TRAIT: a struct of static functions over its state record -- kState doubles, kObs floats of an observation,
// kActions actions, load / store, reset, step, observe -- and one kernel template serves every environment: k_mz_env_step, k_mz_env_move
// and the MOVES stages of the whole-move search, k_mz_search<TREE_LDS, MOVES, Env>.
//
// CartPole-v1: Gymnasium classic_control/cartpole.py v0.29 (Euler integrator, tau 0.02 s, force 10 N, the episode ends at |x| > 2.4
// or |theta| > 12 degrees, reward 1 per step), auto-reset -- the device twin of rlzero_amd/muzero/cartpole.py.
// Acrobot-v1: Gymnasium classic_control/acrobot.py (Sutton's "book" dynamics, no torque noise): two links, torque -1 / 0 / +1 on
// the joint between them, one classical RK4 step of 0.2 s per move, reward -1 per step until the tip is one link above the base.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rz_rng.h"

#if defined(__HIPCC__)
#define RZE_FN __host__ __device__ __forceinline__
#else
#define RZE_FN inline
#endif

#define RZ_MZE_MAX_STATE 8     /* doubles of an environment's state */
#define RZ_MZE_MAX_OBS 16      /* D: floats of an observation (the replay buffer's limit) */
#define RZ_MZE_MAX_ACTIONS 8   /* A (the fused search's limit) */
#define RZ_MZE_TERMINATED 1    /* bits a step returns */
#define RZ_MZE_TRUNCATED 2

namespace rzmze {

// splitmix64: the counter-based stream of rlzero_amd/muzero/cartpole.py (rz_rng.h: mix64)
RZE_FN uint64_t splitmix64(uint64_t x) { return rzrng::mix64(x); }
// the key of an episode's initial state, (seed, environment, episode), and the uniform of its sub-key j + 1 in [0, 1)
RZE_FN uint64_t reset_key(uint64_t seed, int env, long long episode) {
    return splitmix64(splitmix64(seed ^ ((uint64_t)env << 24)) ^ (uint64_t)episode);
}
RZE_FN double reset_uniform(uint64_t key, int j) { return rzrng::unit(splitmix64(key ^ (uint64_t)(j + 1))); }

// ------------------------------------------------------------------ CartPole-v1
struct MzCartPole {
    double x, x_dot, theta, theta_dot;
    long long steps, episode;
};

RZE_FN void cartpole_reset(MzCartPole &c, uint64_t seed, int env) {
    const uint64_t key = reset_key(seed, env, c.episode);
    double v[4];
    for (int j = 0; j < 4; ++j) v[j] = -0.05 + 0.1 * reset_uniform(key, j);
    c.x = v[0];
    c.x_dot = v[1];
    c.theta = v[2];
    c.theta_dot = v[3];
    c.steps = 0;
}

// one step (an action other than 1 pushes to the left; the reward is 1); -> RZ_MZE_TERMINATED | RZ_MZE_TRUNCATED (the state is the
// terminal one: the caller resets)
RZE_FN int cartpole_step(MzCartPole &c, int action, long long max_episode_steps) {
    const double gravity = 9.8, masspole = 0.1, total_mass = 0.1 + 1.0, length = 0.5, polemass_length = 0.1 * 0.5, tau = 0.02;
    const double theta_threshold = 12 * 2 * 3.141592653589793 / 360, x_threshold = 2.4;
    const double force = action == 1 ? 10.0 : -10.0;
    const double costheta = cos(c.theta), sintheta = sin(c.theta);
    const double temp = (force + polemass_length * (c.theta_dot * c.theta_dot) * sintheta) / total_mass;
    const double thetaacc = (gravity * sintheta - costheta * temp) / (length * (4.0 / 3.0 - masspole * (costheta * costheta) / total_mass));
    const double xacc = temp - polemass_length * thetaacc * costheta / total_mass;
    c.x = c.x + tau * c.x_dot;
    c.x_dot = c.x_dot + tau * xacc;
    c.theta = c.theta + tau * c.theta_dot;
    c.theta_dot = c.theta_dot + tau * thetaacc;
    c.steps += 1;
    const bool terminated = c.x < -x_threshold || c.x > x_threshold || c.theta < -theta_threshold || c.theta > theta_threshold;
    const bool truncated = c.steps >= max_episode_steps;
    return (terminated ? RZ_MZE_TERMINATED : 0) | (truncated ? RZ_MZE_TRUNCATED : 0);
}

struct EnvCartPole {
    typedef MzCartPole State;
    static constexpr int kState = 4, kObs = 4, kActions = 2;
    RZE_FN static void load(State &c, const double *s, long long steps, long long episode) { c = State{s[0], s[1], s[2], s[3], steps, episode}; }
    RZE_FN static void store(const State &c, double *s) {
        s[0] = c.x;
        s[1] = c.x_dot;
        s[2] = c.theta;
        s[3] = c.theta_dot;
    }
    RZE_FN static void reset(State &c, uint64_t seed, int env) { cartpole_reset(c, seed, env); }
    RZE_FN static int step(State &c, int action, long long max_episode_steps, double *reward) {
        *reward = 1.0;
        return cartpole_step(c, action, max_episode_steps);
    }
    RZE_FN static void observe(const State &c, float *obs) {
        obs[0] = (float)c.x;
        obs[1] = (float)c.x_dot;
        obs[2] = (float)c.theta;
        obs[3] = (float)c.theta_dot;
    }
};

// ------------------------------------------------------------------ Acrobot-v1
struct MzAcrobot {
    double theta1, theta2, dtheta1, dtheta2;
    long long steps, episode;
};

constexpr double kAcroM1 = 1.0, kAcroM2 = 1.0, kAcroL1 = 1.0, kAcroLc1 = 0.5, kAcroLc2 = 0.5, kAcroI1 = 1.0, kAcroI2 = 1.0, kAcroG = 9.8;
constexpr double kAcroDt = 0.2, kAcroPi = 3.141592653589793, kAcroMaxVel1 = 4.0 * 3.141592653589793, kAcroMaxVel2 = 9.0 * 3.141592653589793;
constexpr int kAcroWraps = 16;   // turns an angle is wrapped by at most (a step moves it by less than 2 pi; an infinite one must not spin)

RZE_FN void acrobot_reset(MzAcrobot &c, uint64_t seed, int env) {
    const uint64_t key = reset_key(seed, env, c.episode);
    double v[4];
    for (int j = 0; j < 4; ++j) v[j] = -0.1 + 0.2 * reset_uniform(key, j);
    c.theta1 = v[0];
    c.theta2 = v[1];
    c.dtheta1 = v[2];
    c.dtheta2 = v[3];
    c.steps = 0;
}

// the derivative of (theta1, theta2, dtheta1, dtheta2) under the torque a
RZE_FN void acrobot_dsdt(const double y[4], double a, double out[4]) {
    const double m1 = kAcroM1, m2 = kAcroM2, l1 = kAcroL1, lc1 = kAcroLc1, lc2 = kAcroLc2, I1 = kAcroI1, I2 = kAcroI2, g = kAcroG, pi = kAcroPi;
    const double theta1 = y[0], theta2 = y[1], dtheta1 = y[2], dtheta2 = y[3];
    const double d1 = m1 * lc1 * lc1 + m2 * (l1 * l1 + lc2 * lc2 + 2.0 * l1 * lc2 * cos(theta2)) + I1 + I2;
    const double d2 = m2 * (lc2 * lc2 + l1 * lc2 * cos(theta2)) + I2;
    const double phi2 = m2 * lc2 * g * cos(theta1 + theta2 - pi / 2.0);
    const double phi1 = -m2 * l1 * lc2 * dtheta2 * dtheta2 * sin(theta2) - 2.0 * m2 * l1 * lc2 * dtheta2 * dtheta1 * sin(theta2) +
                        (m1 * lc1 + m2 * l1) * g * cos(theta1 - pi / 2.0) + phi2;
    const double ddtheta2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * dtheta1 * dtheta1 * sin(theta2) - phi2) / (m2 * lc2 * lc2 + I2 - d2 * d2 / d1);
    const double ddtheta1 = -(d2 * ddtheta2 + phi1) / d1;
    out[0] = dtheta1;
    out[1] = dtheta2;
    out[2] = ddtheta1;
    out[3] = ddtheta2;
}

RZE_FN double acrobot_wrap(double x) {
    const double pi = kAcroPi;
    for (int i = 0; i < kAcroWraps && x > pi; ++i) x = x - 2.0 * pi;
    for (int i = 0; i < kAcroWraps && x < -pi; ++i) x = x + 2.0 * pi;
    return x;
}
RZE_FN double acrobot_bound(double x, double m) { return x < -m ? -m : (x > m ? m : x); }

// one step; -> RZ_MZE_TERMINATED | RZ_MZE_TRUNCATED (the state is the terminal one: the caller resets), *reward = 0 at the goal, else -1
RZE_FN int acrobot_step(MzAcrobot &c, int action, long long max_episode_steps, double *reward) {
    const double dt = kAcroDt, a = (double)(action - 1);
    const double y[4] = {c.theta1, c.theta2, c.dtheta1, c.dtheta2};
    double k1[4], k2[4], k3[4], k4[4], t[4];
    acrobot_dsdt(y, a, k1);
    for (int i = 0; i < 4; ++i) t[i] = y[i] + dt / 2.0 * k1[i];
    acrobot_dsdt(t, a, k2);
    for (int i = 0; i < 4; ++i) t[i] = y[i] + dt / 2.0 * k2[i];
    acrobot_dsdt(t, a, k3);
    for (int i = 0; i < 4; ++i) t[i] = y[i] + dt * k3[i];
    acrobot_dsdt(t, a, k4);
    for (int i = 0; i < 4; ++i) t[i] = y[i] + dt / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
    c.theta1 = acrobot_wrap(t[0]);
    c.theta2 = acrobot_wrap(t[1]);
    c.dtheta1 = acrobot_bound(t[2], kAcroMaxVel1);
    c.dtheta2 = acrobot_bound(t[3], kAcroMaxVel2);
    c.steps += 1;
    const bool terminated = -cos(c.theta1) - cos(c.theta2 + c.theta1) > 1.0;
    const bool truncated = c.steps >= max_episode_steps;
    *reward = terminated ? 0.0 : -1.0;
    return (terminated ? RZ_MZE_TERMINATED : 0) | (truncated ? RZ_MZE_TRUNCATED : 0);
}

RZE_FN void acrobot_observe(const MzAcrobot &c, float obs[6]) {
    obs[0] = (float)cos(c.theta1);
    obs[1] = (float)sin(c.theta1);
    obs[2] = (float)cos(c.theta2);
    obs[3] = (float)sin(c.theta2);
    obs[4] = (float)c.dtheta1;
    obs[5] = (float)c.dtheta2;
}

struct EnvAcrobot {
    typedef MzAcrobot State;
    static constexpr int kState = 4, kObs = 6, kActions = 3;
    RZE_FN static void load(State &c, const double *s, long long steps, long long episode) {
        c.theta1 = s[0];
        c.theta2 = s[1];
        c.dtheta1 = s[2];
        c.dtheta2 = s[3];
        c.steps = steps;
        c.episode = episode;
    }
    RZE_FN static void store(const State &c, double *s) {
        s[0] = c.theta1;
        s[1] = c.theta2;
        s[2] = c.dtheta1;
        s[3] = c.dtheta2;
    }
    RZE_FN static void reset(State &c, uint64_t seed, int env) { acrobot_reset(c, seed, env); }
    RZE_FN static int step(State &c, int action, long long max_episode_steps, double *reward) { return acrobot_step(c, action, max_episode_steps, reward); }
    RZE_FN static void observe(const State &c, float *obs) { acrobot_observe(c, obs); }
};

// ------------------------------------------------------------------ the move behind a search (k_mz_search's MOVES stages, k_mz_env_move)
// weights visits ^ (1 / T) (the visits themselves at 1 / T = 1 or <= 0), their sum in action order and the first maximum
RZE_FN int move_weights(const int *visits, int A, double inv_temperature, double *wgt, double *total) {
    double sum = 0.0, best = -1.0;
    int arg = 0;
    for (int a = 0; a < A; ++a) {
        wgt[a] = inv_temperature == 1.0 || inv_temperature <= 0.0 ? (double)visits[a] : pow((double)visits[a], inv_temperature);
        sum += wgt[a];
        if (wgt[a] > best) {
            best = wgt[a];
            arg = a;
        }
    }
    *total = sum;
    return arg;
}
// the cumulative search against the uniform of `key` (53 bits): the first action whose cumulative weight exceeds u * total
RZE_FN int move_draw(const double *wgt, int A, double total, uint64_t key) {
    const double target = rzrng::unit(key) * total;
    double cum = 0.0;
    for (int a = 0; a < A; ++a) {
        cum += wgt[a];
        if (cum > target) return a;
    }
    return A - 1;
}
// the key of a move's draws: three rounds over (noise_seed ^ salt ^ g << 24, episode, steps)
RZE_FN uint64_t move_key(uint64_t noise_seed, uint64_t salt, int g, long long episode, long long steps) {
    return splitmix64(splitmix64(splitmix64(noise_seed ^ salt ^ ((uint64_t)g << 24)) ^ (uint64_t)episode) ^ (uint64_t)steps);
}

// the 32-bit key of action a's Dirichlet draw under the move's key (salt 0)
RZE_FN uint32_t noise_key(uint64_t key, int a) { return (uint32_t)(key >> 32) + 0x9E3779B9u * (uint32_t)(a + 1) + (uint32_t)key; }

// a move's record of D + 4 + A doubles: obs (D, from 0) | action | reward | visits (A) | root value | done
struct RecordLayout {
    int action, reward, visits, root_value, done, row;
};
RZE_FN constexpr RecordLayout record_layout(int D, int A) { return RecordLayout{D, D + 1, D + 2, D + 2 + A, D + 3 + A, D + 4 + A}; }

}  // namespace rzmze
