"""The harness of the host tests (no test lives here, no GPU): a header under rlzero_amd/csrc/ that compiles without a HIP include is
called by a small stand-alone C++ program with its own main, the DRIVER of a test module.  The driver is built twice with ROCm's
clang++ -- plain, and with -fsanitize=address,undefined -- and every call runs both builds as child processes on the same binary
input files: a report of the sanitizers ends the sanitized build with a non-zero status, and the files the two wrote are held equal
byte for byte.  The float flags are the library's own (rlzero_amd/_build.py: FLAGS), so a bit-for-bit comparison with a numpy
restatement says something about the kernels that include the same header.

    drv = host_driver.fixture('name', DRIVER)                       # module scoped: the driver is built once per module
    def test_x(drv):
        out_a, out_b = drv.run('command', [3, 4], [array, array], [np.float32, np.int32])"""
import filecmp
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import REPO  # (puts the repository on sys.path)
from rlzero_amd import _build

CSRC = os.path.join(REPO, 'rlzero_amd', 'csrc')
INCLUDE = os.path.join(REPO, 'include')

FLOAT_FLAGS = ['-ffp-contract=off', '-fno-fast-math']   # what the bit-for-bit comparisons rest on: the library is built with the same
assert all(flag in _build.FLAGS for flag in FLOAT_FLAGS), 'the host drivers are not built with the float flags of the library'
FLAGS = ['-std=c++17', '-O1', *FLOAT_FLAGS, '-Wall', '-Werror']
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g']
RUN_ENV = dict(ASAN_OPTIONS='detect_leaks=0', UBSAN_OPTIONS='print_stacktrace=1')   # (stand-alone programs: the runtime is linked in)


def host_clangxx():
    """ROCm's clang++ (a host g++ may not know _Float16): beside HIPCC, or under ROCM_PATH / /opt/rocm."""
    roots = []
    if os.environ.get('HIPCC'):
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(os.environ['HIPCC']))))
    roots += [os.environ.get('ROCM_PATH') or '/opt/rocm', '/opt/rocm']
    for root in roots:
        for sub in ('llvm/bin', 'lib/llvm/bin', 'bin'):
            path = os.path.join(root, sub, 'clang++')
            if os.path.exists(path):
                return path
    return None


def compile_command(*args, include=(CSRC, INCLUDE)):
    """[clang++, the common flags, -I of each of `include`, *args]"""
    cxx = host_clangxx()
    assert cxx is not None, "ROCm's clang++ builds the host drivers (HIPCC, ROCM_PATH or /opt/rocm)"
    return [cxx, *FLAGS, *[opt for d in include for opt in ('-I', d)], *args]


def probe(tmp, source, include=(CSRC, INCLUDE)):
    """Compiles `source` (plain build only) in the directory `tmp`, runs it without arguments and returns what it printed, as bytes."""
    src, exe = os.path.join(str(tmp), 'probe.cpp'), os.path.join(str(tmp), 'probe')
    with open(src, 'w') as f:
        f.write(source)
    subprocess.run(compile_command(src, '-o', exe, include=include), check=True)
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout


class Driver(object):
    """The plain and the sanitized build of one driver, in the directory `tmp`."""

    def __init__(self, tmp, name, source, include=(CSRC, INCLUDE)):
        self.tmp, self.exes, self.calls = tmp, [], 0
        src = os.path.join(tmp, name + '.cpp')
        with open(src, 'w') as f:
            f.write(source)
        for exe, extra in ((name, []), (name + '_san', SANITIZE)):
            self.exes.append(os.path.join(tmp, exe))
            subprocess.run(compile_command(*extra, src, '-o', self.exes[-1], include=include), check=True)
        self.env = dict(os.environ, **RUN_ENV)

    def write(self, arrays):
        """One new file per array -> the paths"""
        self.calls += 1
        paths = [os.path.join(self.tmp, 'in%d_%d.bin' % (self.calls, i)) for i in range(len(arrays))]
        for path, arr in zip(paths, arrays):
            np.ascontiguousarray(arr).tofile(path)
        return paths

    def fresh(self, n):
        """(n unused paths for the plain build, n for the sanitized build)"""
        self.calls += 1
        return tuple([os.path.join(self.tmp, 'out%d_%d%s.bin' % (self.calls, i, tag)) for i in range(n)] for tag in ('', '_san'))

    def both(self, argv, outs):
        """The primitive: each build runs on `argv` followed by its own output paths, `outs` = ``fresh(n)``; a non-zero exit of either
        raises subprocess.CalledProcessError.  -> outs: (the plain build's output paths, the sanitized build's)"""
        for exe, paths in zip(self.exes, outs):
            subprocess.run([exe, *[str(a) for a in argv], *paths], check=True, env=self.env)
        return outs

    def same(self, argv, n_out):
        """``both``, and the two builds wrote the same bytes -> the plain build's paths.  The files are compared on disk and the
        sanitized build's are removed: an output may be large (tests/test_ring_host.py: 128 MB)."""
        plain, san = self.both(argv, self.fresh(n_out))
        for p, s in zip(plain, san):   # the sanitized build ran without a report (it would have exited non-zero)
            assert filecmp.cmp(p, s, shallow=False), 'the sanitized build wrote other bytes: %s' % ' '.join(str(a) for a in argv)
            os.remove(s)
        return plain

    def run(self, what, args, inputs, outputs):
        """`what args <a file of each array of inputs> <an output file per dtype of outputs>` -> the plain build's arrays"""
        paths = self.same([what, *args, *self.write(inputs)], len(outputs))
        return [np.fromfile(p, dtype=dt) for p, dt in zip(paths, outputs)]


def fixture(name, source, **kwargs):
    """A module-scoped fixture that builds the driver once; its temporary directory lives as long as the fixture."""
    @pytest.fixture(scope='module')
    def drv():
        with tempfile.TemporaryDirectory() as tmp:
            yield Driver(tmp, name, source, **kwargs)
    return drv
