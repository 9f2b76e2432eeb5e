"""The harness of the host tests (tests/host_driver.py) on drivers of its own: what ``run`` hands back, and that it stops on what it is
there to catch -- two builds that disagree, a build that ends with a status."""
import subprocess

import numpy as np
import pytest

import host_driver
from rlzero_amd import _build

HEAD = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

template <typename T>
static std::vector<T> load(const char *path) {
    std::vector<T> v;
    T x;
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    while (fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
    fclose(f);
    return v;
}
template <typename T>
static void store(const char *path, const std::vector<T> &v) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
}
'''

# axpy k x.f32 [n] y.i64 [n] -> k x + y as f64 [n], (k + y) as i32 [n]
ROUND_TRIP = HEAD + r'''
int main(int argc, char **argv) {
    if (argc != 7 || std::string(argv[1]) != "axpy") return 4;
    const int k = atoi(argv[2]);
    const std::vector<float> x = load<float>(argv[3]);
    const std::vector<int64_t> y = load<int64_t>(argv[4]);
    std::vector<double> a;
    std::vector<int32_t> b;
    for (size_t i = 0; i < x.size(); ++i) a.push_back((double)k * x[i] + (double)y[i]), b.push_back((int32_t)(k + y[i]));
    store(argv[5], a);
    store(argv[6], b);
    return 0;
}
'''

# same x.u8 -> x; differ x.u8 -> x, with the first byte changed in the sanitized build; fail_plain / fail_san -> status 3 in that build
FAULTY = HEAD + r'''
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define SANITIZED 1
#endif
#endif
#ifndef SANITIZED
#define SANITIZED 0
#endif
int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if ((what == "fail_plain" && !SANITIZED) || (what == "fail_san" && SANITIZED)) return 3;
    if (argc != 4) return 4;
    std::vector<uint8_t> x = load<uint8_t>(argv[2]);
    if (what == "differ") x.at(0) ^= SANITIZED;
    store(argv[3], x);
    return 0;
}
'''

round_trip = host_driver.fixture('round_trip', ROUND_TRIP)
faulty = host_driver.fixture('faulty', FAULTY)


def test_run_returns_the_outputs_with_their_dtypes(round_trip):
    x, y = np.array([0.5, -1.25, 3.0], dtype=np.float32), np.array([7, -2, 1 << 20], dtype=np.int64)
    a, b = round_trip.run('axpy', [3], [x, y], [np.float64, np.int32])
    assert a.dtype == np.float64 and a.tolist() == [8.5, -5.75, 1048585.0]
    assert b.dtype == np.int32 and b.tolist() == [10, 1, 1048579]
    a2, _ = round_trip.run('axpy', [-1], [x[:1], y[:1]], [np.float64, np.int32])   # (a second call has files of its own)
    assert a2.tolist() == [6.5] and a.tolist() == [8.5, -5.75, 1048585.0]


def test_builds_that_disagree_are_caught(faulty):
    x = np.arange(5, dtype=np.uint8)
    assert faulty.run('same', [], [x], [np.uint8])[0].tolist() == x.tolist()
    with pytest.raises(AssertionError):
        faulty.run('differ', [], [x], [np.uint8])
    plain, san = faulty.both(['differ', *faulty.write([x])], faulty.fresh(1))   # (the primitive hands both builds' files back)
    assert np.fromfile(plain[0], dtype=np.uint8).tolist() == [0, 1, 2, 3, 4] and np.fromfile(san[0], dtype=np.uint8).tolist() == [1, 1, 2, 3, 4]


@pytest.mark.parametrize('what', ['fail_plain', 'fail_san'])
def test_a_failing_status_is_caught(faulty, what):
    """Whichever build it comes from (a report of the sanitizers ends the sanitized build with a status)."""
    x = np.arange(5, dtype=np.uint8)
    with pytest.raises(subprocess.CalledProcessError) as err:
        faulty.run(what, [], [x], [np.uint8])
    assert err.value.returncode == 3 and err.value.cmd[0] == faulty.exes[what == 'fail_san']


def test_the_float_flags_are_the_librarys():
    assert host_driver.FLOAT_FLAGS == ['-ffp-contract=off', '-fno-fast-math']
    assert all(flag in _build.FLAGS and flag in host_driver.FLAGS for flag in host_driver.FLOAT_FLAGS)
    assert all(flag in host_driver.compile_command() for flag in host_driver.FLAGS)
    assert '-Werror' in host_driver.FLAGS and not any(flag.startswith('-fsanitize') for flag in host_driver.FLAGS)
