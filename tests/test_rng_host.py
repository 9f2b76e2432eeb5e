"""The one 64-bit mix (rlzero_amd/csrc/rz_rng.h: mix64, mulhi64, unit; rlzero_amd/_rng.py: the host's two forms of it) and the
mini-batch draw built on it (rlzero_amd/csrc/rz_replay_rules.h: replay_index -- what k_replay_sample calls) on the CPU.

A driver with its own main is compiled against the headers with ROCm's clang++ (by tests/host_driver.py),
once plain and once with -fsanitize=address,undefined -fno-sanitize-recover=all, and run as a stand-alone program.  mix64 and
mulhi64 are held to Python integers (the arithmetic written out below, no import of the package's) at 0, 1, 2^32 - 1, 2^32, 2^63,
2^64 - 1 and a few hundred random 64-bit words; unit at the two ends of its range; replay_index to rlzero_amd.replay.replay_index
and replay_indices for n_entries from 1 to 2^31 - 1 over a few steps and seeds, one of them above 2^63.  The last test holds the two
forms of rlzero_amd/_rng.py to each other and to tests/device_streams.py (an independent copy on purpose) on the same words."""
import numpy as np

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import device_streams
import host_driver
from rlzero_amd import _rng
from rlzero_amd.replay import replay_index, replay_indices

M64 = (1 << 64) - 1
EDGES = [0, 1, (1 << 32) - 1, 1 << 32, 1 << 63, M64]

DRIVER = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "rz_replay_rules.h"
#include "rz_rng.h"

template <typename T>
static std::vector<T> load(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (bytes && fread(v.data(), 1, (size_t)bytes, f) != (size_t)bytes) exit(2);
    fclose(f);
    return v;
}
template <typename T>
static void store(const char *path, const std::vector<T> &v) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror(path); exit(2); }
    fclose(f);
}

// mix   x.u64 [n]               -> mix64(x).u64 [n], unit(x).f64 [n]
// mulhi ab.u64 [n][2]           -> mulhi64(a, b).u64 [n]
// index rows.u64 [n][4]: seed, step, i, n_entries -> rzrr::replay_index.i64 [n]
int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "mix" && argc == 5) {
        const std::vector<uint64_t> x = load<uint64_t>(argv[2]);
        std::vector<uint64_t> mixed(x.size());
        std::vector<double> units(x.size());
        for (size_t i = 0; i < x.size(); ++i) mixed[i] = rzrng::mix64(x[i]), units[i] = rzrng::unit(x[i]);
        store(argv[3], mixed);
        store(argv[4], units);
        return 0;
    }
    if (what == "mulhi" && argc == 4) {
        const std::vector<uint64_t> ab = load<uint64_t>(argv[2]);
        std::vector<uint64_t> hi(ab.size() / 2);
        for (size_t i = 0; i < hi.size(); ++i) hi[i] = rzrng::mulhi64(ab[2 * i], ab[2 * i + 1]);
        store(argv[3], hi);
        return 0;
    }
    if (what == "index" && argc == 4) {
        const std::vector<uint64_t> rows = load<uint64_t>(argv[2]);
        std::vector<int64_t> index(rows.size() / 4);
        for (size_t i = 0; i < index.size(); ++i) index[i] = rzrr::replay_index(rows[4 * i], rows[4 * i + 1], rows[4 * i + 2], rows[4 * i + 3]);
        store(argv[3], index);
        return 0;
    }
    return 4;
}
'''


def mix64_int(x):
    """splitmix64's finaliser in Python integers: this test's own copy."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def words():
    rng = np.random.RandomState(20250)
    random = [(int(hi) << 32) | int(lo) for hi, lo in rng.randint(0, 1 << 32, size=(300, 2), dtype=np.int64)]
    return EDGES + random


drv = host_driver.fixture('rng', DRIVER)


def test_mix64_and_unit_are_the_integers_arithmetic(drv):
    xs = words()
    mixed, units = drv.run('mix', [], [np.array(xs, dtype=np.uint64)], [np.uint64, np.float64])
    assert [int(v) for v in mixed] == [mix64_int(x) for x in xs]
    # the unit step: the 53 high bits over 2^53, exact in a double -- 0 at one end, 1 - 2^-53 at the other
    assert units.tolist() == [(x >> 11) / float(1 << 53) for x in xs]
    assert units[xs.index(0)] == 0.0 and units[xs.index(M64)] == 1.0 - 2.0 ** -53 and float(units.max()) < 1.0
    more = [(1 << 11) - 1, 1 << 11]
    _, edge = drv.run('mix', [], [np.array(more, dtype=np.uint64)], [np.uint64, np.float64])
    assert edge.tolist() == [0.0, 2.0 ** -53]


def test_mulhi64_is_the_high_half_of_the_product(drv):
    xs = words()
    pairs = [(a, b) for a in EDGES for b in EDGES] + list(zip(xs[6:], reversed(xs[6:]))) + [(x, e) for x in xs[6:40] for e in EDGES]
    (hi, ) = drv.run('mulhi', [], [np.array(pairs, dtype=np.uint64)], [np.uint64])
    assert [int(v) for v in hi] == [(a * b) >> 64 for a, b in pairs]


def test_replay_index_is_the_packages_draw(drv):
    sizes = [1, 2, 3, 7, 8, 1000, 65536, 722 * 8, (1 << 24) * 8, (1 << 31) - 2, (1 << 31) - 1]
    seeds, steps, n = [0, 7, (1 << 63) + 12345, M64], [0, 1, 2, 1 << 40], 24
    rows = [(seed, step, i, size) for size in sizes for seed in seeds for step in steps for i in range(n)]
    (index, ) = drv.run('index', [], [np.array(rows, dtype=np.uint64)], [np.int64])
    assert index.tolist() == [replay_index(*row) for row in rows]
    at = 0
    for size in sizes:
        for seed in seeds:
            for step in steps:
                block = index[at:at + n]
                at += n
                assert np.array_equal(block, replay_indices(seed, step, n, size))
                assert block.min() >= 0 and block.max() < size
    assert at == len(index)
    # counters beyond a mini-batch's: the chain takes any 64-bit i
    far = [(3, 5, i, 1 << 20) for i in ((1 << 32) - 1, 1 << 32, 1 << 63, M64)]
    (index, ) = drv.run('index', [], [np.array(far, dtype=np.uint64)], [np.int64])
    assert index.tolist() == [replay_index(*row) for row in far]


def test_the_packages_two_forms_agree_with_each_other_and_with_the_independent_copy():
    xs = words()
    want = [mix64_int(x) for x in xs]
    assert [_rng.mix64(x) for x in xs] == want
    with np.errstate(over='ignore'):
        assert [int(v) for v in _rng.mix64_u64(np.array(xs, dtype=np.uint64))] == want
        assert [int(_rng.mix64_u64(np.uint64(x))) for x in EDGES] == want[:len(EDGES)]
    assert [int(v) for v in device_streams.mix64(np.array(xs, dtype=np.uint64))] == want
    assert [int(v) for v in device_streams.splitmix64(np.array(xs, dtype=np.uint64))] == want
