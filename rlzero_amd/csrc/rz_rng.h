// rz_rng.h -- the 64-bit mix every keyed random stream of the library is built from, once: the splitmix64 finaliser, the high half of a
// 64-bit product (a draw in 0 .. n - 1 from 64 bits, integer only) and the 53 high bits of a word as a double in [0, 1).  Plain C++,
// no HIP include, so that the CPU can test it against Python integers (tests/test_rng_host.py); rlzero_amd/_rng.py is the same mix
// for the host's restatements.  The SALTS and the chains stay with the streams they name: rz_play.h (moves, resignation, playout
// cap, noise keys), rz_replay_rules.h (mini-batches, Reanalyse), rz_mz_target.h (MuZero's draws) and rz_mz_env.h (resets, action
// draws) name these functions inside their own namespaces.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RZN_FN __host__ __device__ __forceinline__
#else
#define RZN_FN inline
#endif

namespace rzrng {

RZN_FN uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// floor(a * b / 2^64): for a uniform 64-bit a a value in 0 .. b - 1 whose probability is floor or ceil of 2^64 / b over 2^64
RZN_FN uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// the 53 high bits of x over 2^53: every value is a double, 0 <= unit < 1
RZN_FN double unit(uint64_t x) { return (double)(x >> 11) * (1.0 / 9007199254740992.0); }

}  // namespace rzrng
