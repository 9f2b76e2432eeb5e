// rz_mz_target.h -- the MuZero learner's unrolled targets (rz_mz_replay.hip: k_mzr_gather, k_mzr_sample; include/rlzero_hip.h:
// rz_mz_replay_*): everything about them that is neither a kernel launch nor a memory access.  Plain C++, no HIP include, so that
// the CPU can test it against rlzero_amd/muzero/selfplay.py: ReplayBuffer.sample (tests/test_mz_replay_host.py); the kernels call
// these functions.  The arithmetic is fp64 multiply and add in the order of ReplayBuffer._value_target, the discounts come from a
// table the host filled with `discount ** i` (no pow here), and the value is cast to float32 once: with -ffp-contract=off the
// host's bits.  Reanalyse's arithmetic and draws (k_mzr_positions, k_mzr_update) follow, tested the same way
// (tests/test_mz_reanalyse_host.py), and at the end the integer priorities, the draws and the search of prioritized replay
// (k_mzr_prio, k_mzr_draw_prio; tests/test_mz_prioritized_host.py).
#pragma once
#include <stdint.h>

#include "rz_mz_value.h"
#include "rz_rng.h"

#if defined(__HIPCC__)
#define RZT_FN __host__ __device__ __forceinline__
#else
#define RZT_FN inline
#endif

#define RZ_MZR_MAX_OBS 16      /* D: floats of an observation */
#define RZ_MZR_MAX_ACTIONS 8   /* A */
#define RZ_MZR_MAX_UNROLL 16   /* K */
#define RZ_MZR_MAX_TD 64       /* td_steps */

namespace rzmzt {

// ---- the draws of k_mzr_sample (rlzero_amd/muzero/replay.py: mz_replay_draws, the same bits)
using rzrng::mix64;     // (rz_rng.h)
using rzrng::mulhi64;

constexpr uint64_t kSampleSalt = 0x6D7A7265706C6179ull;   // "mzreplay": the sampler's own stream, apart from rz_replay's

// counter c of entry i of update `step`: c = i * (K + 2) + j -- j = 0 the episode, j = 1 the position, j = 2 + k the filler action
// of unroll step k
RZT_FN uint64_t draw_counter(uint64_t i, int K, int j) { return i * (uint64_t)(K + 2) + (uint64_t)j; }
// the high half of x * n for the 64-bit x of the chain over (seed, step, c): in 0 .. n - 1, within 2^-64 of uniform
RZT_FN int64_t draw(uint64_t seed, uint64_t step, uint64_t c, uint64_t n) {
    uint64_t x = mix64(seed ^ kSampleSalt);
    x = mix64(x ^ step);
    x = mix64(x ^ c);
    return (int64_t)mulhi64(x, n);
}

// ---- ReplayBuffer._value_target(ep, t): the n-step return from step t, bootstrapped from the root value td steps on if the
// episode still runs there.  disc[i] = discount ** i, i = 0 .. td.
RZT_FN double value_target(const double *reward, const double *root_value, int len, int t, int td, const double *disc) {
    const int boot = t + td;
    double value = boot < len ? root_value[boot] * disc[td] : 0.0;
    const int end = boot < len ? boot : len;
    for (int i = 0; t + i < end; ++i) value += reward[t + i] * disc[i];
    return value;
}

// ---- row k of an entry at position `pos` of an episode of `len` steps (the inside / outside rules of ReplayBuffer.sample)
struct Row {
    float value;        // tv[b, k]
    float reward;       // tr[b, k]
    float mask;         // mask[b, k]
    int policy_step;    // tp[b, k] = policy[policy_step], or the uniform policy when -1
    int64_t action;     // actions[b, k - 1] (k > 0)
};
// `filler`: the action drawn for actions[b, k - 1] when step pos + k - 1 lies past the end
// VT (rz_mz_replay_set_value_transform): the value and the reward of a row inside the episode go through rz_mz_value.h's value_h in
// fp64 -- the n-step return exactly as formed without it, the stored reward -- before their one cast to float32; rows past the end
// stay 0.  Nothing else of a row changes.
template <bool VT>
RZT_FN float target_f32(double x) {
    return VT ? (float)rzmzv::value_h(x) : (float)x;
}
template <bool VT = false>
RZT_FN Row unroll_row(const double *reward, const double *root_value, const int32_t *action, int len, int pos, int k, int td,
                      const double *disc, int64_t filler) {
    Row r;
    const int i = pos + k;
    const bool in = i < len;
    r.value = in ? target_f32<VT>(value_target(reward, root_value, len, i, td, disc)) : 0.0f;
    r.mask = in ? 1.0f : 0.0f;
    r.policy_step = in ? i : -1;
    r.reward = 0.0f;
    r.action = 0;
    if (k > 0) {   // the action taken at step i - 1 and its reward: still real at i == len
        const bool prev = i - 1 < len;
        r.action = prev ? (int64_t)action[i - 1] : filler;
        r.reward = prev ? target_f32<VT>(reward[i - 1]) : 0.0f;
    }
    return r;
}
// np.full(.., 1.0 / n_actions, dtype=float32)
RZT_FN float uniform_policy(int A) { return (float)(1.0 / (double)A); }

// ---- a stored step from a packed record: float64 [obs (D) | action | reward | visits (A) | root value | done].  The policy is
// EpisodeSeq.fields_of_packed's visits / sum(visits) in fp64 (visit counts are integers: the sum is exact in any order), cast
// to float32; `final_policy`: the columns already hold the float32 policy (an Episode of the move-by-move routes), only cast.
RZT_FN float policy_of_row(const double *row, int D, int A, int a, bool final_policy) {
    const double *vis = row + D + 2;
    if (final_policy) return (float)vis[a];
    double sum = 0.0;
    for (int b = 0; b < A; ++b) sum += vis[b];
    return (float)(vis[a] / sum);
}

// ---- Reanalyse (k_mzr_positions, k_mzr_update; rlzero_amd/muzero/reanalyse.py): a stored step searched again, its policy and
// root value replaced.
// The policy of fresh visit counts: fields_of_packed's expression on integers (their sum is exact); a root that was never
// visited gets the uniform policy.
RZT_FN float policy_of_visits(const int32_t *visits, int A, int a) {
    int64_t sum = 0;
    for (int b = 0; b < A; ++b) sum += visits[b];
    if (sum == 0) return uniform_policy(A);
    return (float)((double)visits[a] / (double)sum);
}
// MuZeroSelfPlay.search's vsum / n.clamp_min(1)
RZT_FN double root_value_of(int32_t n, double value_sum) { return value_sum / (double)(n > 1 ? n : 1); }

constexpr uint64_t kReanalyseSalt = 0x6D7A7265616E616Cull;   // "mzreanal": a refresh and a mini-batch of one update number share no draw

// counter c = 2 i + j of refresh `step` -- j = 0 the episode (n = episodes held), j = 1 the position (n = its length); the chain
// of `draw` under the salt above (rlzero_amd/muzero/reanalyse.py: mz_reanalyse_draws, the same bits)
RZT_FN int64_t reanalyse_draw(uint64_t seed, uint64_t step, uint64_t i, int j, uint64_t n) {
    uint64_t x = mix64(seed ^ kReanalyseSalt);
    x = mix64(x ^ step);
    x = mix64(x ^ (2 * i + (uint64_t)j));
    return (int64_t)mulhi64(x, n);
}

// ---- Prioritized replay (k_mzr_prio, k_mzr_scan, k_mzr_draw_prio; rlzero_amd/muzero/replay.py: mz_priority_weights,
// mz_prioritized_draws): arXiv:1911.08265v2 appendix G with alpha = 1 -- step t is drawn with probability p_t / sum p, where
// p_t = |root value - n-step return| of the SAME stored step.  The priorities are FIXED-POINT integers (16 fraction bits), so that
// sums are exact in any order and a parallel scan gives the bits of a Python loop.
RZT_FN double priority_of(const double *reward, const double *root_value, int len, int t, int td, const double *disc) {
    return __builtin_fabs(root_value[t] - value_target(reward, root_value, len, t, td, disc));
}
// p * 2^16 truncated (the product by a power of two is exact), at least 1 -- every stored step stays drawable -- and 2^32 from
// p = 2^16 on, which bounds the total of 2^30 steps below 2^62; a NaN gives 1.
RZT_FN uint64_t priority_weight(double p) {
    if (!(p > 0.0)) return 1;   // zero, a NaN (and anything negative: fabs gives none)
    if (p >= 65536.0) return 1ull << 32;
    const uint64_t w = (uint64_t)(p * 65536.0);
    return w > 1 ? w : 1;
}

constexpr uint64_t kPrioSalt = 0x6D7A7072696F7269ull;   // "mzpriori": the prioritized sampler's own stream

// Entry i of update `step`, over the counters of `draw_counter`: j = 0 ONE uniform over 0 .. total - 1 that decides episode and
// position together, j = 1 unused, j = 2 + k the filler action of unroll step k (uniform over A, as in `draw`).
RZT_FN uint64_t prio_chain(uint64_t seed, uint64_t step, uint64_t c) {
    uint64_t x = mix64(seed ^ kPrioSalt);
    x = mix64(x ^ step);
    return mix64(x ^ c);
}
RZT_FN uint64_t prio_target(uint64_t seed, uint64_t step, uint64_t i, int K, uint64_t total) {
    return mulhi64(prio_chain(seed, step, draw_counter(i, K, 0)), total);
}
RZT_FN int64_t prio_filler(uint64_t seed, uint64_t step, uint64_t i, int K, int k, uint64_t A) {
    return (int64_t)mulhi64(prio_chain(seed, step, draw_counter(i, K, 2 + k)), A);
}
// the first index of cum[0 .. n - 1] (non-decreasing) with cum[idx] > g; n if there is none
RZT_FN int64_t upper_bound_u64(const uint64_t *cum, int64_t n, uint64_t g) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (cum[mid] > g) hi = mid; else lo = mid + 1;
    }
    return lo;
}

}  // namespace rzmzt
