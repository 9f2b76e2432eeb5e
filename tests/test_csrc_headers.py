"""Every kernel header of rz_net.hip compiles alone (rlzero_amd/csrc/rz_net_*.h, rz_delta.h), and so does the profile build.

rz_net.hip is one translation unit cut into one header per kernel family.  Each header includes what it uses and opens its own
anonymous namespace, so it can be read -- and parsed -- without the others before it: a syntax-only pass of hipcc over the header as
the main file, with the include paths of rlzero_amd/_build.py, must succeed.  A header that leans on what rz_net.hip happens to
include before it fails here in under a second.  -DRZ_NET_PROFILE changes kernel text in every family and is built by nothing else,
so one more case parses all of rz_net.hip with it.  Nothing is compiled to code."""
import glob
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'rlzero_amd', 'csrc')
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, 'rz_net_*.h'))) + ['rz_delta.h']


def find_hipcc():
    """The compiler of rlzero_amd/_build.py: HIPCC, hipcc on the PATH, or the one under ROCM_PATH / /opt/rocm."""
    for cand in (os.environ.get('HIPCC'), 'hipcc', os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'bin', 'hipcc')):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    return None


HIPCC = find_hipcc()
pytestmark = pytest.mark.skipif(HIPCC is None, reason='hipcc is not found (HIPCC, PATH, ROCM_PATH or /opt/rocm)')


def syntax_only(source, *defines):
    cmd = [HIPCC, '--offload-arch=gfx950', '-std=c++17', '-fsyntax-only', '-x', 'hip', '-I' + os.path.join(REPO, 'include'), '-I' + CSRC]
    return subprocess.run(cmd + list(defines) + [os.path.join(CSRC, source)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def test_the_family_headers_are_the_ones_the_index_names():
    assert HEADERS == ['rz_net_dev.h', 'rz_net_f32.h', 'rz_net_heads.h', 'rz_net_rows.h', 'rz_net_split.h', 'rz_delta.h']
    with open(os.path.join(CSRC, 'rz_net.hip')) as f:
        text = f.read()
    for name in HEADERS:
        assert '#include "%s"' % name in text, name


# (rz_host.h: the host-side runtime all five sources include -- no kernel family, but a header that must stand alone like the others)
@pytest.mark.parametrize('header', HEADERS + ['rz_host.h'])
def test_a_kernel_header_compiles_alone(header):
    done = syntax_only(header)
    assert done.returncode == 0, done.stdout.decode(errors='replace')[-4000:]


def test_the_profile_build_compiles():
    done = syntax_only('rz_net.hip', '-DRZ_NET_PROFILE')
    assert done.returncode == 0, done.stdout.decode(errors='replace')[-4000:]
