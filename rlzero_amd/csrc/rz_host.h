// rz_host.h -- the host-side runtime the six translation units share (rz_engine, rz_net, rz_muzero, rz_replay, rz_mz_replay, rz_mz_learn): the error
// message, the checks every entry point opens with, the check of a caller's buffer that kernels write, the two ways to own device memory
// and the staging pair.  Host code only (every source keeps its kernels in headers of their own): no kernel,
// nothing a kernel reads.  One copy of each, so that a new subsystem takes its plumbing from here instead of copying a neighbour's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <vector>

#include "rlzero_hip.h"

void rz_set_error(const char *msg);  // rz_engine.hip (its host side, like g_err): sets the thread-local message rz_last_error() returns

constexpr size_t kRzErrBytes = 512;  // the size of that message (g_err)

// ---------------------------------------------------------------- errors and the checks of an entry point

__attribute__((format(printf, 2, 3))) inline int rz_fail(int code, const char *fmt, ...) {
    char buf[kRzErrBytes];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    rz_set_error(buf);
    return code;
}

// a HIP call whose failure is the entry point's: the call's text and the runtime's reason
#define RZ_HIP(call)                                                                            \
    do {                                                                                        \
        hipError_t err__ = (call);                                                              \
        if (err__ != hipSuccess)                                                                \
            return rz_fail(err__ == hipErrorOutOfMemory ? RZ_ERR_OOM : RZ_ERR_HIP, "%s failed: %s", \
                           #call, hipGetErrorString(err__));                                    \
    } while (0)

// an int return code that is the caller's unless it is RZ_OK
#define RZ_TRY(expr)                     \
    do {                                 \
        int rc__ = (expr);               \
        if (rc__ != RZ_OK) return rc__;  \
    } while (0)

// the first line of an entry point: its handle's guard (the NULL check with the handle's name, then rz_on_device)
#define RZ_ENTER(guard, ...) RZ_TRY(guard(__VA_ARGS__))

#define RZ_NEED(p)                                                          \
    do {                                                                    \
        if ((p) == nullptr) return rz_fail(RZ_ERR_ARG, "%s is NULL", #p);   \
    } while (0)

// the host copy and the device copy of one argument (indices, draws): exactly one of the two is given
#define RZ_ONE_OF(h, d)                                                                                   \
    do {                                                                                                  \
        if (((h) == nullptr) == ((d) == nullptr)) return rz_fail(RZ_ERR_ARG, "exactly one of %s / %s", #h, #d); \
    } while (0)

// the buffers a launch writes: none of them is NULL
template <typename... T>
int rz_outputs(const T *...p) {
    if (((p == nullptr) || ...)) return rz_fail(RZ_ERR_ARG, "NULL output buffer");
    return RZ_OK;
}

// the calling thread works on `device` from here on
inline int rz_on_device(int device) {
    int cur = -1;
    RZ_HIP(hipGetDevice(&cur));
    if (cur != device) RZ_HIP(hipSetDevice(device));
    return RZ_OK;
}

// the creation of a handle on `device`: the ordinal names a device, and the calling thread works on it from here on
inline int rz_claim_device(int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return rz_fail(RZ_ERR_ARG, "bad device ordinal");
    if (hipSetDevice(device) != hipSuccess) return rz_fail(RZ_ERR_HIP, "hipSetDevice failed");
    return RZ_OK;
}

inline int rz_launched(const char *what) {
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return rz_fail(RZ_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(err));
    return RZ_OK;
}

// ---------------------------------------------------------------- a caller's buffer that kernels write directly

// A buffer in HOST memory (pinned) must be addressable from `device`: asked, not assumed.  `p` becomes the address the device uses; an
// address the runtime does not know is treated as device memory and stays as it is.  `entry` and `arg` name the entry point and its
// argument in the message.
template <typename T>
int rz_device_address(T *&p, int device, const char *entry, const char *arg) {
    hipPointerAttribute_t attr = {};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
    } else if (attr.type == hipMemoryTypeHost) {
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, p, 0) != hipSuccess || dp == nullptr) {
            (void)hipGetLastError();
            return rz_fail(RZ_ERR_ARG, "%s: %s is host memory that device %d cannot address (pass device memory)", entry, arg, device);
        }
        p = static_cast<T *>(dp);
    }
    return RZ_OK;
}

// ---------------------------------------------------------------- device memory: two owners for two lifetimes

// A device allocation its holder owns: move-only, freed with the holder.  Reads as the pointer it holds.  For a buffer that is
// resized or replaced while its holder lives.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr, bytes = 0; }
    bool alloc(size_t n) { release(); return hipMalloc((void **)&p, n) == hipSuccess ? (bytes = n, true) : (p = nullptr, false); }
    bool fill(int byte) { return hipMemset(p, byte, bytes) == hipSuccess; }
};

// Allocations that live as long as their holder and whose pointers sit in a struct passed to kernels by value: the pool only remembers
// what to free.  `bytes` counts what was asked for (an empty array still gets 8 bytes of its own).
struct DevPool {
    std::vector<void *> ptrs;
    long long bytes = 0;
    DevPool() = default;
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    ~DevPool() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    int alloc(T **out, long long count) {
        void *p = nullptr;
        const size_t n = (size_t)count * sizeof(T);
        hipError_t err = hipMalloc(&p, n ? n : 8);
        if (err != hipSuccess) return rz_fail(RZ_ERR_OOM, "hipMalloc(%zu bytes) failed: %s", n, hipGetErrorString(err));
        ptrs.push_back(p);
        bytes += (long long)n;
        *out = (T *)p;
        return RZ_OK;
    }
};

// ---------------------------------------------------------------- the staging pair

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// One pinned host block and one device block of the same size, reused from call to call.  A call fills `h` after reserve(), sends it
// with upload(), launches what reads `d` and reports the launch with launched().  Three waits keep the reuse safe: the host half is
// written again only after `copied` (the last upload has left it), the pair grows only after `consumed` (nothing reads the device half
// any more), and the stream waits for `consumed` before a new upload overwrites the device half.
struct Staging {
    void *h = nullptr, *d = nullptr;
    size_t bytes = 0;
    hipEvent_t copied = nullptr, consumed = nullptr;
    bool in_flight = false;
    const char *owner = "";   // for the messages: "replay", "MuZero replay"

    int check(hipError_t err, int code, const char *what, const char *where) const {
        return err == hipSuccess ? RZ_OK : rz_fail(code, "%s failed (%s%s): %s", what, owner, where, hipGetErrorString(err));
    }
    int create(const char *owner_name) {
        owner = owner_name;
        RZ_TRY(check(hipEventCreateWithFlags(&copied, hipEventDisableTiming), RZ_ERR_HIP, "hipEventCreate", " staging"));
        return check(hipEventCreateWithFlags(&consumed, hipEventDisableTiming), RZ_ERR_HIP, "hipEventCreate", " staging");
    }
    // (the owner has synchronised the device)
    void destroy() {
        if (copied) (void)hipEventDestroy(copied);
        if (consumed) (void)hipEventDestroy(consumed);
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        *this = Staging();
    }
    // the pair with room for `n` bytes, its host half free to be written; `stream` waits for the device half's last reader
    int reserve(size_t n, hipStream_t stream) {
        if (in_flight) RZ_TRY(check(hipEventSynchronize(copied), RZ_ERR_HIP, "hipEventSynchronize", " staging"));
        if (n > bytes) {
            if (in_flight) RZ_TRY(check(hipEventSynchronize(consumed), RZ_ERR_HIP, "hipEventSynchronize", " staging"));
            in_flight = false;
            if (h) (void)hipHostFree(h);
            if (d) (void)hipFree(d);
            h = d = nullptr;
            bytes = 0;
            const size_t want = n + n / 2 + 4096;
            RZ_TRY(check(hipHostMalloc(&h, want, hipHostMallocDefault), RZ_ERR_OOM, "hipHostMalloc", " staging"));
            RZ_TRY(check(hipMalloc(&d, want), RZ_ERR_OOM, "hipMalloc", " staging"));
            bytes = want;
        }
        if (in_flight) RZ_TRY(check(hipStreamWaitEvent(stream, consumed, 0), RZ_ERR_HIP, "hipStreamWaitEvent", " staging"));
        return RZ_OK;
    }
    int upload(size_t n, hipStream_t stream) {
        RZ_TRY(check(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, stream), RZ_ERR_HIP, "staging copy", ""));
        return check(hipEventRecord(copied, stream), RZ_ERR_HIP, "hipEventRecord", "");
    }
    // after the launch (or copy) on `stream` that reads the device half
    int launched(hipStream_t stream, const char *what) {
        RZ_TRY(rz_launched(what));
        RZ_TRY(check(hipEventRecord(consumed, stream), RZ_ERR_HIP, "hipEventRecord", ""));
        in_flight = true;
        return RZ_OK;
    }
};
