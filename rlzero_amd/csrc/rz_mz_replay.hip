// rz_mz_replay.hip -- the MuZero learner's replay buffer in device memory (include/rlzero_hip.h: rz_mz_replay_*, ABI 35; Reanalyse: ABI 36; prioritized
// replay: ABI 37).
//
// Finished episodes live on the GPU in fixed-stride slots -- slot e holds up to T steps, structure of arrays -- in a ring over
// EPISODES, and a mini-batch of unrolled targets is ONE launch: k_mzr_gather / k_mzr_sample write the observation, the K actions
// and the K + 1 value / reward / policy targets and masks of every entry straight into the learner's tensors, bit for bit what
// rlzero_amd/muzero/selfplay.py: ReplayBuffer.sample forms on the host (the rules and the arithmetic: rz_mz_target.h).  Episodes
// arrive as packed float64 records, the format of rz_mz_play_cartpole: from a staged host block (k_mzr_add) or straight from a
// launch's device arena (k_mzr_ingest: only a small entry table travels).  Reanalyse (k_mzr_positions, k_mzr_update) hands stored
// observations out to a fresh search and takes its visit counts and root value back into the steps they came from.  Prioritized
// replay (k_mzr_prio, k_mzr_scan, k_mzr_draw_prio; opt-in) keeps an integer priority per stored step and its prefix sums on the
// device and draws steps in proportion to them.
//
// Bounds: every slot is reduced modulo the capacity, every length is clamped to 0 .. T where it is read, every step index is compared
// with that length before a read, rows of a block are checked against its row count (on the host and again in the kernel), and an
// index from the device is checked by the kernel before anything is read -- such an entry is not written and a flag is set.
//
// This file is the host side of ONE translation unit: the kernels lie in headers beside it, one per family, each of which compiles
// alone (tests/test_csrc_headers.py) and describes its kernels where they are defined.
//   rz_mz_replay_dev.h      no kernel: MzrDev, MzrOut, the launch shape and the flags, mzr_slot, mzr_length
//   rz_mz_replay_store.h    the way in: k_mzr_add, k_mzr_ingest (mzr_store)
//   rz_mz_replay_batch.h    the mini-batch: k_mzr_gather, k_mzr_sample (mzr_emit)
//   rz_mz_replay_refresh.h  Reanalyse: k_mzr_positions, k_mzr_update
//   rz_mz_replay_prio.h     prioritized replay: MzrPrio, k_mzr_mark, k_mzr_mark_where, k_mzr_prio, k_mzr_scan, k_mzr_draw_prio
// The rules the kernels and the host share are plain C++ in rz_mz_target.h, the ring of episodes is rz_ring.h's; both are tested on
// the CPU.  Below: struct rz_mz_replay, the entry table of an add, the argument checks and every extern "C" entry point.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "rlzero_hip.h"
#include "rz_host.h"
#include "rz_mz_target.h"
#include "rz_ring.h"

// (this order is the order of the kernels in the code object; the template instantiations follow in the order the code below names them)
#include "rz_mz_replay_dev.h"
#include "rz_mz_replay_store.h"
#include "rz_mz_replay_batch.h"
#include "rz_mz_replay_refresh.h"
#include "rz_mz_replay_prio.h"

struct rz_mz_replay {
    MzrDev dev = {};
    int device = 0;
    rz_ring ring;   // of episodes; ring.stored is the ticket of rz_mz_replay_positions / rz_mz_replay_update
    std::vector<int32_t> lengths;      // [E] by slot: the host's copy of dev.length
    double *d_disc = nullptr;
    DevPool pool;    // the store
    Staging stage;   // what the host hands to a launch
    // prioritized replay (rz_mz_replay_enable_priorities): nothing of it exists until it is enabled
    MzrPrio prio = {};
    DevPool prio_pool;
    bool prio_on = false;
    bool prio_stale = false;   // a slot was written since the prefixes were formed: the next prioritized draw refreshes first
    bool value_transform = false;   // rz_mz_replay_set_value_transform: mini-batches come from k_mzr_gather<true> / k_mzr_sample<true>
};

namespace {

int mr_ready(rz_mz_replay *r) {
    if (r == nullptr) return rz_fail(RZ_ERR_ARG, "MuZero replay handle is NULL");
    return rz_on_device(r->device);
}

// The entry table of `n` episodes (empty ones skipped; of more than the capacity only the last E get a slot) in `table`; -> the
// number of entries, or a negative code.  first_rows NULL: the episodes lie one behind the other.  Every run of rows is checked
// against n_rows here.
int mr_table(rz_mz_replay *r, int32_t n, const int32_t *h_lengths, const int32_t *h_flags, const int64_t *h_first_rows, int64_t n_rows,
             std::vector<int32_t> &table, long long *held) {
    long long kept = 0, next = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (h_lengths[i] < 0) return rz_fail(RZ_ERR_ARG, "an episode of negative length");
        if (h_lengths[i] > r->dev.T) return rz_fail(RZ_ERR_ARG, "an episode is longer than max_episode_steps");
        const long long first = h_first_rows ? h_first_rows[i] : next;
        if (h_lengths[i] > 0 && (first < 0 || first > 0x7fffffffLL || first + h_lengths[i] > n_rows))
            return rz_fail(RZ_ERR_ARG, "an episode's rows lie outside the block");
        next = first + h_lengths[i];
        kept += h_lengths[i] > 0;
    }
    const long long skip = r->ring.skip(kept);
    table.clear();
    long long t = 0;
    next = 0;
    for (int32_t i = 0; i < n; ++i) {
        const long long first = h_first_rows ? h_first_rows[i] : next;
        next = first + h_lengths[i];
        if (h_lengths[i] == 0) continue;
        if (t >= skip) {
            const int32_t entry[kEntryWords] = {h_lengths[i], (int32_t)first, (int32_t)r->ring.slot(t), h_flags ? h_flags[i] : 0};
            table.insert(table.end(), entry, entry + kEntryWords);
        }
        ++t;
    }
    *held = kept;
    return (int)(table.size() / kEntryWords);
}

void mr_commit(rz_mz_replay *r, const std::vector<int32_t> &table, long long kept) {
    for (size_t e = 0; e < table.size() / kEntryWords; ++e) r->lengths[(size_t)table[kEntryWords * e + 2]] = table[kEntryWords * e];
    r->ring.commit(kept);
}

int mr_outputs(rz_mz_replay *r, int64_t n, const MzrOut &O) {
    if (n < 0 || n > (1LL << 24)) return rz_fail(RZ_ERR_ARG, "n outside 0 .. 2^24");
    return n > 0 ? rz_outputs(O.obs, O.actions, O.tv, O.tr, O.tp, O.mask) : RZ_OK;
}

inline unsigned mr_blocks(const rz_mz_replay *r, int64_t n) { return (unsigned)((n * (r->dev.K + 1) + kThreads - 1) / kThreads); }

// priorities on: the slots `first` .. + n - 1 (modulo E) were written by a kernel launched on `s` before this call
int mr_mark(rz_mz_replay *r, long long first, long long n, hipStream_t s) {
    if (!r->prio_on || n <= 0) return RZ_OK;
    if (n > r->dev.E) n = r->dev.E;
    hipLaunchKernelGGL(k_mzr_mark, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, r->prio, r->dev.E, first, n);
    RZ_TRY(rz_launched("k_mzr_mark"));
    r->prio_stale = true;
    return RZ_OK;
}
// the slots of an entry table: contiguous modulo E from its first entry's
int mr_mark_table(rz_mz_replay *r, const std::vector<int32_t> &table, hipStream_t s) {
    if (!r->prio_on || table.empty()) return RZ_OK;
    return mr_mark(r, table[2], (long long)(table.size() / kEntryWords), s);
}

// the prefixes of every slot written since they were last formed, then the prefix over the episodes: two launches on `s`
int mr_refresh(rz_mz_replay *r, hipStream_t s) {
    if (r->ring.count > 0) {
        const long long oldest = r->ring.oldest();
        hipLaunchKernelGGL(k_mzr_prio, dim3((unsigned)r->ring.count), dim3(kThreads), 0, s, r->dev, r->prio, oldest, r->ring.count);
        hipLaunchKernelGGL(k_mzr_scan, dim3(1), dim3(kScanThreads), 0, s, r->prio, r->dev.E, oldest, r->ring.count);
        RZ_TRY(rz_launched("k_mzr_prio / k_mzr_scan"));
    }
    r->prio_stale = false;
    return RZ_OK;
}

}  // namespace

extern "C" {

int rz_mz_replay_create(int32_t obs_dim, int32_t n_actions, int64_t capacity_episodes, int32_t max_episode_steps, int32_t unroll_steps,
                        int32_t td_steps, const double *h_disc, int32_t device, rz_mz_replay **out) {
    if (out == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (obs_dim < 1 || obs_dim > RZ_MZR_MAX_OBS) return rz_fail(RZ_ERR_ARG, "obs_dim outside 1 .. 16");
    if (n_actions < 1 || n_actions > RZ_MZR_MAX_ACTIONS) return rz_fail(RZ_ERR_ARG, "n_actions outside 1 .. 8");
    if (unroll_steps < 1 || unroll_steps > RZ_MZR_MAX_UNROLL) return rz_fail(RZ_ERR_ARG, "unroll_steps outside 1 .. 16");
    if (td_steps < 1 || td_steps > RZ_MZR_MAX_TD) return rz_fail(RZ_ERR_ARG, "td_steps outside 1 .. 64");
    if (max_episode_steps < 1 || max_episode_steps > 65536) return rz_fail(RZ_ERR_ARG, "max_episode_steps outside 1 .. 65536");
    if (capacity_episodes < 1 || capacity_episodes > (1LL << 22) || capacity_episodes * max_episode_steps > (1LL << 30))
        return rz_fail(RZ_ERR_ARG, "capacity_episodes outside 1 .. 2^22, or more than 2^30 steps in all");
    if (h_disc == nullptr) return rz_fail(RZ_ERR_ARG, "NULL discount table");
    RZ_TRY(rz_claim_device(device));
    rz_mz_replay *r = new (std::nothrow) rz_mz_replay();
    if (!r) return rz_fail(RZ_ERR_OOM, "host allocation failed");
    r->device = device;
    MzrDev &R = r->dev;
    R.E = (int)capacity_episodes, R.T = max_episode_steps, R.D = obs_dim, R.A = n_actions, R.K = unroll_steps, R.td = td_steps;
    r->ring.capacity = R.E;
    r->lengths.assign((size_t)R.E, 0);
    const size_t steps = (size_t)R.E * R.T, n_disc = (size_t)td_steps + 1;
    const long long n_steps = (long long)steps;
    DevPool &pool = r->pool;
    bool ok = pool.alloc(&R.obs, n_steps * R.D) == RZ_OK && pool.alloc(&R.action, n_steps) == RZ_OK && pool.alloc(&R.reward, n_steps) == RZ_OK &&
              pool.alloc(&R.root_value, n_steps) == RZ_OK && pool.alloc(&R.policy, n_steps * R.A) == RZ_OK && pool.alloc(&R.length, R.E) == RZ_OK &&
              pool.alloc(&r->d_disc, (long long)n_disc) == RZ_OK && pool.alloc(&R.err, 1) == RZ_OK;
    if (!ok) {
        rz_mz_replay_destroy(r);
        return rz_fail(RZ_ERR_OOM, "hipMalloc failed (MuZero replay store)");
    }
    R.disc = r->d_disc;
    ok = hipMemset(R.err, 0, sizeof(int32_t)) == hipSuccess && hipMemset(R.obs, 0, steps * R.D * sizeof(float)) == hipSuccess &&
         hipMemset(R.action, 0, steps * sizeof(int32_t)) == hipSuccess && hipMemset(R.reward, 0, steps * sizeof(double)) == hipSuccess &&
         hipMemset(R.root_value, 0, steps * sizeof(double)) == hipSuccess && hipMemset(R.policy, 0, steps * R.A * sizeof(float)) == hipSuccess &&
         hipMemset(R.length, 0, (size_t)R.E * sizeof(int32_t)) == hipSuccess &&
         hipMemcpy(r->d_disc, h_disc, n_disc * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
         r->stage.create("MuZero replay") == RZ_OK && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        rz_mz_replay_destroy(r);
        return rz_fail(RZ_ERR_HIP, "initialisation of the MuZero replay store failed");
    }
    *out = r;
    return RZ_OK;
}

int rz_mz_replay_destroy(rz_mz_replay *r) {
    if (r == nullptr) return RZ_OK;
    (void)hipSetDevice(r->device);
    (void)hipDeviceSynchronize();
    r->stage.destroy();
    delete r;   // (the pools free the store and the priority tables)
    return RZ_OK;
}

int rz_mz_replay_state(rz_mz_replay *r, int64_t *count, int64_t *cursor, int64_t *capacity, int32_t *h_lengths) {
    if (r == nullptr) return rz_fail(RZ_ERR_ARG, "MuZero replay handle is NULL");
    if (count) *count = r->ring.count;
    if (cursor) *cursor = r->ring.cursor;
    if (capacity) *capacity = r->ring.capacity;
    if (h_lengths) {
        for (long long j = 0; j < r->ring.count; ++j) h_lengths[j] = r->lengths[(size_t)r->ring.window_start(j)];
    }
    return RZ_OK;
}

int rz_mz_replay_add(rz_mz_replay *r, int32_t n_episodes, const int32_t *h_lengths, const int32_t *h_flags, const double *h_rows, void *stream) {
    RZ_ENTER(mr_ready, r);
    if (n_episodes < 0) return rz_fail(RZ_ERR_ARG, "n_episodes < 0");
    if (n_episodes == 0) return RZ_OK;
    if (h_lengths == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    long long total = 0;
    for (int32_t i = 0; i < n_episodes; ++i) total += h_lengths[i] > 0 ? h_lengths[i] : 0;
    if (total > 0x7fffffffLL) return rz_fail(RZ_ERR_ARG, "more than 2^31 - 1 rows in one call");
    std::vector<int32_t> table;
    long long kept = 0;
    const int n = mr_table(r, n_episodes, h_lengths, h_flags, nullptr, total, table, &kept);
    if (n < 0) return n;
    if (kept == 0) return RZ_OK;
    if (h_rows == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    const int W = r->dev.D + 4 + r->dev.A;
    for (long long row = 0; row < total; ++row) {
        const double a = h_rows[row * W + r->dev.D];
        if (!(a >= 0.0 && a < (double)r->dev.A && a == (double)(int)a)) return rz_fail(RZ_ERR_ARG, "an action is outside 0 .. A-1");
    }
    // staging: entry table | rows
    const size_t o_rows = align16(table.size() * sizeof(int32_t)), bytes = o_rows + (size_t)total * W * sizeof(double);
    hipStream_t s = (hipStream_t)stream;
    RZ_TRY(r->stage.reserve(bytes, s));
    char *h = (char *)r->stage.h, *d = (char *)r->stage.d;
    memcpy(h, table.data(), table.size() * sizeof(int32_t));
    memcpy(h + o_rows, h_rows, (size_t)total * W * sizeof(double));
    RZ_TRY(r->stage.upload(bytes, s));
    hipLaunchKernelGGL(k_mzr_add, dim3((unsigned)n), dim3(kThreads), 0, s, r->dev, (const int32_t *)d, (const double *)(d + o_rows), total);
    RZ_TRY(r->stage.launched(s, "k_mzr_add"));
    mr_commit(r, table, kept);
    return mr_mark_table(r, table, s);
}

int rz_mz_replay_ingest(rz_mz_replay *r, int32_t n_episodes, const int32_t *h_lengths, const int64_t *h_first_rows, const double *d_arena,
                        int64_t arena_rows, int32_t row_doubles, void *stream) {
    RZ_ENTER(mr_ready, r);
    if (n_episodes < 0) return rz_fail(RZ_ERR_ARG, "n_episodes < 0");
    if (n_episodes == 0) return RZ_OK;
    if (h_lengths == nullptr || h_first_rows == nullptr || d_arena == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    if (row_doubles != r->dev.D + 4 + r->dev.A) return rz_fail(RZ_ERR_ARG, "the arena's rows are not obs_dim + 4 + n_actions doubles");
    if (arena_rows < 0 || arena_rows > 0x7fffffffLL) return rz_fail(RZ_ERR_ARG, "arena_rows outside 0 .. 2^31 - 1");
    std::vector<int32_t> table;
    long long kept = 0;
    const int n = mr_table(r, n_episodes, h_lengths, nullptr, h_first_rows, arena_rows, table, &kept);
    if (n < 0) return n;
    if (kept == 0) return RZ_OK;
    const size_t bytes = table.size() * sizeof(int32_t);
    hipStream_t s = (hipStream_t)stream;
    RZ_TRY(r->stage.reserve(bytes, s));
    memcpy(r->stage.h, table.data(), bytes);
    RZ_TRY(r->stage.upload(bytes, s));
    hipLaunchKernelGGL(k_mzr_ingest, dim3((unsigned)n), dim3(kThreads), 0, s, r->dev, (const int32_t *)r->stage.d, d_arena, (long long)arena_rows);
    RZ_TRY(r->stage.launched(s, "k_mzr_ingest"));
    mr_commit(r, table, kept);
    return mr_mark_table(r, table, s);
}

int rz_mz_replay_gather(rz_mz_replay *r, const int64_t *h_draws, const int64_t *d_draws, int64_t n, float *d_obs, int64_t *d_actions, float *d_tv,
                        float *d_tr, float *d_tp, float *d_mask, void *stream) {
    RZ_ENTER(mr_ready, r);
    const MzrOut O = {d_obs, (long long *)d_actions, d_tv, d_tr, d_tp, d_mask};
    RZ_TRY(mr_outputs(r, n, O));
    RZ_ONE_OF(h_draws, d_draws);
    if (n == 0) return RZ_OK;
    if (r->ring.count == 0) return rz_fail(RZ_ERR_ARG, "the MuZero replay buffer is empty");
    hipStream_t s = (hipStream_t)stream;
    const long long oldest = r->ring.oldest();
    const long long *draws = (const long long *)d_draws;
    const int K = r->dev.K;
    if (h_draws != nullptr) {
        for (int64_t i = 0; i < n; ++i) {
            const int64_t *dr = h_draws + i * (K + 2);
            if (dr[0] < 0 || dr[0] >= r->ring.count) return rz_fail(RZ_ERR_ARG, "an episode index is outside 0 .. count - 1");
            if (dr[1] < 0 || dr[1] >= r->lengths[(size_t)r->ring.window_start(dr[0])]) return rz_fail(RZ_ERR_ARG, "a position is outside its episode");
            for (int j = 0; j < K; ++j)
                if (dr[2 + j] < 0 || dr[2 + j] >= r->dev.A) return rz_fail(RZ_ERR_ARG, "a filler action is outside 0 .. A-1");
        }
        const size_t bytes = (size_t)n * (K + 2) * sizeof(int64_t);
        RZ_TRY(r->stage.reserve(bytes, s));
        memcpy(r->stage.h, h_draws, bytes);
        RZ_TRY(r->stage.upload(bytes, s));
        draws = (const long long *)r->stage.d;
    }
    if (r->value_transform) hipLaunchKernelGGL(k_mzr_gather<true>, dim3(mr_blocks(r, n)), dim3(kThreads), 0, s, r->dev, O, draws, oldest, r->ring.count, (long long)n);
    else hipLaunchKernelGGL(k_mzr_gather<false>, dim3(mr_blocks(r, n)), dim3(kThreads), 0, s, r->dev, O, draws, oldest, r->ring.count, (long long)n);
    return h_draws != nullptr ? r->stage.launched(s, "k_mzr_gather") : rz_launched("k_mzr_gather");
}

int rz_mz_replay_sample(rz_mz_replay *r, uint64_t seed, uint64_t step, int64_t n, float *d_obs, int64_t *d_actions, float *d_tv, float *d_tr,
                        float *d_tp, float *d_mask, void *stream) {
    RZ_ENTER(mr_ready, r);
    const MzrOut O = {d_obs, (long long *)d_actions, d_tv, d_tr, d_tp, d_mask};
    RZ_TRY(mr_outputs(r, n, O));
    if (r->ring.count == 0) return rz_fail(RZ_ERR_ARG, "the MuZero replay buffer is empty");
    if (n == 0) return RZ_OK;
    if (r->value_transform)
        hipLaunchKernelGGL(k_mzr_sample<true>, dim3(mr_blocks(r, n)), dim3(kThreads), 0, (hipStream_t)stream, r->dev, O, (unsigned long long)seed,
                           (unsigned long long)step, r->ring.oldest(), r->ring.count, (long long)n);
    else
        hipLaunchKernelGGL(k_mzr_sample<false>, dim3(mr_blocks(r, n)), dim3(kThreads), 0, (hipStream_t)stream, r->dev, O, (unsigned long long)seed,
                           (unsigned long long)step, r->ring.oldest(), r->ring.count, (long long)n);
    return rz_launched("k_mzr_sample");
}

int rz_mz_replay_set_value_transform(rz_mz_replay *r, int32_t on) {
    if (r == nullptr) return rz_fail(RZ_ERR_ARG, "MuZero replay handle is NULL");
    if (on != 0 && on != 1) return rz_fail(RZ_ERR_ARG, "value transform: 0 (off) or 1 (on)");
    r->value_transform = on != 0;
    return RZ_OK;
}

int rz_mz_replay_positions(rz_mz_replay *r, const int64_t *h_draws, const int64_t *d_draws, uint64_t seed, uint64_t step, int64_t n,
                            int32_t *d_where, float *d_obs, int64_t *ticket, void *stream) {
    RZ_ENTER(mr_ready, r);
    if (n < 0 || n > (1LL << 24)) return rz_fail(RZ_ERR_ARG, "n outside 0 .. 2^24");
    if (ticket == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    if (h_draws != nullptr && d_draws != nullptr) return rz_fail(RZ_ERR_ARG, "at most one of h_draws / d_draws");
    *ticket = r->ring.ticket();
    if (n == 0) return RZ_OK;
    RZ_TRY(rz_outputs(d_where, d_obs));
    if (r->ring.count == 0) return rz_fail(RZ_ERR_ARG, "the MuZero replay buffer is empty");
    hipStream_t s = (hipStream_t)stream;
    const long long oldest = r->ring.oldest();
    const long long *draws = (const long long *)d_draws;
    if (h_draws != nullptr) {
        for (int64_t i = 0; i < n; ++i) {
            const int64_t *dr = h_draws + 2 * i;
            if (dr[0] < 0 || dr[0] >= r->ring.count) return rz_fail(RZ_ERR_ARG, "an episode index is outside 0 .. count - 1");
            if (dr[1] < 0 || dr[1] >= r->lengths[(size_t)r->ring.window_start(dr[0])]) return rz_fail(RZ_ERR_ARG, "a position is outside its episode");
        }
        const size_t bytes = (size_t)n * 2 * sizeof(int64_t);
        RZ_TRY(r->stage.reserve(bytes, s));
        memcpy(r->stage.h, h_draws, bytes);
        RZ_TRY(r->stage.upload(bytes, s));
        draws = (const long long *)r->stage.d;
    }
    const unsigned blocks = (unsigned)((n * r->dev.D + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_mzr_positions, dim3(blocks), dim3(kThreads), 0, s, r->dev, draws, (unsigned long long)seed, (unsigned long long)step, oldest,
                       r->ring.count, (long long)n, d_where, d_obs);
    return h_draws != nullptr ? r->stage.launched(s, "k_mzr_positions") : rz_launched("k_mzr_positions");
}

int rz_mz_replay_update(rz_mz_replay *r, const int32_t *d_where, int64_t n, const int32_t *d_visits, const int32_t *d_root_n,
                        const double *d_root_sum, int64_t ticket, void *stream) {
    RZ_ENTER(mr_ready, r);
    if (n < 0 || n > (1LL << 24)) return rz_fail(RZ_ERR_ARG, "n outside 0 .. 2^24");
    // an add or ingest since rz_mz_replay_positions may have given a slot to another episode: the search's result has no home
    if (!r->ring.ticket_current(ticket)) return rz_fail(RZ_ERR_ARG, "stale ticket: episodes were stored since rz_mz_replay_positions");
    if (n == 0) return RZ_OK;
    if (d_where == nullptr || d_visits == nullptr || d_root_n == nullptr || d_root_sum == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    const unsigned blocks = (unsigned)((n * (r->dev.A + 1) + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_mzr_update, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, r->dev, d_where, (long long)n, d_visits, d_root_n,
                       d_root_sum);
    RZ_TRY(rz_launched("k_mzr_update"));
    if (r->prio_on) {   // a changed root value moves the priority of its step and of the step td before it: both in this slot
        hipLaunchKernelGGL(k_mzr_mark_where, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, r->dev, r->prio,
                           d_where, (long long)n);
        RZ_TRY(rz_launched("k_mzr_mark_where"));
        r->prio_stale = true;
    }
    return RZ_OK;
}

int rz_mz_replay_read(rz_mz_replay *r, int64_t first, int64_t n, float *h_obs, int32_t *h_action, double *h_reward, double *h_root_value,
                      float *h_policy, int32_t *h_length, void *stream) {
    RZ_ENTER(mr_ready, r);
    if (first < 0 || n < 0 || first + n > r->ring.count) return rz_fail(RZ_ERR_ARG, "episodes outside 0 .. count - 1");
    hipStream_t s = (hipStream_t)stream;
    const MzrDev &R = r->dev;
    const long long E = R.E, start = r->ring.window_start(first);
    const long long n1 = n < E - start ? n : E - start;   // up to the ring's end, then from its start
    const size_t T = (size_t)R.T, D = (size_t)R.D, A = (size_t)R.A;
    bool ok = true;
    for (int part = 0; part < 2; ++part) {
        const long long from = part == 0 ? start : 0, cnt = part == 0 ? n1 : n - n1, at = part == 0 ? 0 : n1;
        if (cnt <= 0) continue;
        const size_t c = (size_t)cnt;
        if (h_obs) ok = ok && hipMemcpyAsync(h_obs + at * T * D, R.obs + from * T * D, c * T * D * sizeof(float), hipMemcpyDeviceToHost, s) == hipSuccess;
        if (h_action) ok = ok && hipMemcpyAsync(h_action + at * T, R.action + from * T, c * T * sizeof(int32_t), hipMemcpyDeviceToHost, s) == hipSuccess;
        if (h_reward) ok = ok && hipMemcpyAsync(h_reward + at * T, R.reward + from * T, c * T * sizeof(double), hipMemcpyDeviceToHost, s) == hipSuccess;
        if (h_root_value) ok = ok && hipMemcpyAsync(h_root_value + at * T, R.root_value + from * T, c * T * sizeof(double), hipMemcpyDeviceToHost, s) == hipSuccess;
        if (h_policy) ok = ok && hipMemcpyAsync(h_policy + at * T * A, R.policy + from * T * A, c * T * A * sizeof(float), hipMemcpyDeviceToHost, s) == hipSuccess;
        if (h_length) ok = ok && hipMemcpyAsync(h_length + at, R.length + from, c * sizeof(int32_t), hipMemcpyDeviceToHost, s) == hipSuccess;
    }
    if (!ok || hipStreamSynchronize(s) != hipSuccess) return rz_fail(RZ_ERR_HIP, "read-back failed (MuZero replay)");
    return RZ_OK;
}

int rz_mz_replay_poll_errors(rz_mz_replay *r, int32_t *flags, void *stream) {
    RZ_ENTER(mr_ready, r);
    if (flags == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(flags, r->dev.err, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemsetAsync(r->dev.err, 0, sizeof(int32_t), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return rz_fail(RZ_ERR_HIP, "reading the MuZero replay flags failed");
    return RZ_OK;
}

int rz_mz_replay_enable_priorities(rz_mz_replay *r, void *stream) {
    RZ_ENTER(mr_ready, r);
    if (r->prio_on) return RZ_OK;
    const MzrDev &R = r->dev;
    if ((long long)R.E * R.T > (1LL << 30)) return rz_fail(RZ_ERR_ARG, "priorities need at most 2^30 steps in all (the total stays below 2^62)");
    MzrPrio P = {};
    DevPool pool;   // the handle's once every table is there and zeroed; until then a failure frees what there is
    const size_t E = (size_t)R.E;
    const bool ok = pool.alloc(&P.cum, (long long)R.E * R.T) == RZ_OK && pool.alloc(&P.mass, R.E) == RZ_OK && pool.alloc(&P.ecum, R.E) == RZ_OK &&
                    pool.alloc(&P.total, 1) == RZ_OK && pool.alloc(&P.dirty, R.E) == RZ_OK;
    hipStream_t s = (hipStream_t)stream;
    if (!ok || hipMemsetAsync(P.cum, 0, E * R.T * sizeof(uint64_t), s) != hipSuccess || hipMemsetAsync(P.mass, 0, E * sizeof(uint64_t), s) != hipSuccess ||
        hipMemsetAsync(P.ecum, 0, E * sizeof(uint64_t), s) != hipSuccess || hipMemsetAsync(P.total, 0, sizeof(uint64_t), s) != hipSuccess ||
        hipMemsetAsync(P.dirty, 0, E * sizeof(int32_t), s) != hipSuccess)
        return rz_fail(ok ? RZ_ERR_HIP : RZ_ERR_OOM, "allocating the priority tables failed (MuZero replay)");
    r->prio_pool.ptrs.swap(pool.ptrs);
    r->prio = P;
    r->prio_on = true;
    r->prio_stale = true;
    return mr_mark(r, r->ring.oldest(), r->ring.count, s);   // every episode held
}

int rz_mz_replay_refresh_priorities(rz_mz_replay *r, void *stream) {
    RZ_ENTER(mr_ready, r);
    if (!r->prio_on) return rz_fail(RZ_ERR_ARG, "priorities are off (rz_mz_replay_enable_priorities)");
    return mr_refresh(r, (hipStream_t)stream);
}

int rz_mz_replay_read_priorities(rz_mz_replay *r, int64_t first, int64_t n, int64_t *h_w, int64_t *h_total, void *stream) {
    RZ_ENTER(mr_ready, r);
    if (!r->prio_on) return rz_fail(RZ_ERR_ARG, "priorities are off (rz_mz_replay_enable_priorities)");
    if (first < 0 || n < 0 || first + n > r->ring.count) return rz_fail(RZ_ERR_ARG, "episodes outside 0 .. count - 1");
    if (n > 0 && h_w == nullptr) return rz_fail(RZ_ERR_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    RZ_TRY(mr_refresh(r, s));
    const MzrDev &R = r->dev;
    const long long E = R.E, start = r->ring.window_start(first);
    const long long n1 = n < E - start ? n : E - start;   // up to the ring's end, then from its start
    const size_t T = (size_t)R.T;
    std::vector<uint64_t> cum((size_t)n * T);
    uint64_t total = 0;
    bool ok = true;
    for (int part = 0; part < 2; ++part) {
        const long long from = part == 0 ? start : 0, cnt = part == 0 ? n1 : n - n1, at = part == 0 ? 0 : n1;
        if (cnt <= 0) continue;
        ok = ok && hipMemcpyAsync(cum.data() + at * T, r->prio.cum + from * T, (size_t)cnt * T * sizeof(uint64_t), hipMemcpyDeviceToHost, s) == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(&total, r->prio.total, sizeof(uint64_t), hipMemcpyDeviceToHost, s) == hipSuccess;
    if (!ok || hipStreamSynchronize(s) != hipSuccess) return rz_fail(RZ_ERR_HIP, "read-back failed (MuZero replay priorities)");
    for (int64_t j = 0; j < n; ++j) {
        const int len = r->lengths[(size_t)r->ring.window_start(first + j)];
        for (int t = 0; t < R.T; ++t)
            h_w[(size_t)j * T + t] = t < len ? (int64_t)(cum[(size_t)j * T + t] - (t > 0 ? cum[(size_t)j * T + t - 1] : 0)) : 0;
    }
    if (h_total) *h_total = (int64_t)total;
    return RZ_OK;
}

int rz_mz_replay_draw_prioritized(rz_mz_replay *r, uint64_t seed, uint64_t step, int64_t n, const int64_t *d_targets, int64_t *d_draws, double *d_prob,
                                  void *stream) {
    RZ_ENTER(mr_ready, r);
    if (!r->prio_on) return rz_fail(RZ_ERR_ARG, "priorities are off (rz_mz_replay_enable_priorities)");
    if (n < 0 || n > (1LL << 24)) return rz_fail(RZ_ERR_ARG, "n outside 0 .. 2^24");
    if (r->ring.count == 0) return rz_fail(RZ_ERR_ARG, "the MuZero replay buffer is empty");
    if (n == 0) return RZ_OK;
    RZ_TRY(rz_outputs(d_draws, d_prob));
    hipStream_t s = (hipStream_t)stream;
    if (r->prio_stale) {
        RZ_TRY(mr_refresh(r, s));
    }
    hipLaunchKernelGGL(k_mzr_draw_prio, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, r->dev, r->prio, (unsigned long long)seed,
                       (unsigned long long)step, (const long long *)d_targets, r->ring.oldest(), r->ring.count, (long long)n, (long long *)d_draws, d_prob);
    return rz_launched("k_mzr_draw_prio");
}

}  // extern "C"
