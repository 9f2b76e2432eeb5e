"""Every kernel header of the six sources compiles alone (rlzero_amd/csrc/rz_net_*.h, rz_delta.h, rz_engine_*.h, rz_muzero_*.h, and
the headers of rz_replay.hip, rz_mz_replay.hip and rz_mz_learn.hip named below), and so do the profile builds.

Each of the six is one translation unit cut into one header per kernel family.  Each header includes what it uses and opens its own
anonymous namespace, so it can be read -- and parsed -- without the others before it: a syntax-only pass of hipcc over the header as
the main file, with the include paths of rlzero_amd/_build.py, must succeed.  A header that leans on what its source happens to
include before it fails here in under a second.  -DRZ_NET_PROFILE changes kernel text in every family and is built by nothing else,
so one more case parses all of rz_net.hip with it; -DRZ_MZ_PROFILE changes k_mz_search's text and gets a case of its own.  Nothing is
compiled to code.

rz_play.h and rz_forced.h are left out: they use __forceinline__ without the runtime header, because the CPU tests also compile them
as plain C++, so they do not parse alone as HIP.  rz_mz_env.h and rz_mz_value.h are left out for the same reason: under hipcc their
functions are __host__ __device__ __forceinline__ (RZE_FN, RZV_FN), and they include no runtime header because the CPU tests compile
them as plain C++ (tests/test_mz_env_host.py, tests/test_mz_value_transform_host.py): "unknown type name '__forceinline__'".
rz_replay_rules.h, rz_mz_target.h and rz_rng.h are left out for that reason too.  rz_mz_pack.h and rz_ring.h -- plain C++ with no
attribute at all -- do parse alone as HIP and are held to it.

The last tests hold rlzero_amd/_build.py to what the compiler reads: an object is keyed on the headers headers_of() finds for its
source, and every project header the preprocessor opens for that source (hipcc -MM) must be among them."""
import glob
import os
import shutil
import subprocess

import pytest

from rlzero_amd import _build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'rlzero_amd', 'csrc')
NET_HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, 'rz_net_*.h'))) + ['rz_delta.h']
ENGINE_HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, 'rz_engine_*.h')))
MUZERO_HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, 'rz_muzero_*.h')))
# (named one by one: rz_replay_*.h would also find rz_replay_rules.h, which by design does not parse alone as HIP)
REPLAY_HEADERS = ['rz_replay_dev.h', 'rz_replay_add.h', 'rz_replay_batch.h', 'rz_replay_refresh.h']
MZ_REPLAY_HEADERS = ['rz_mz_replay_dev.h', 'rz_mz_replay_store.h', 'rz_mz_replay_batch.h', 'rz_mz_replay_refresh.h', 'rz_mz_replay_prio.h']
MZ_LEARN_HEADERS = ['rz_mz_learn_grad.h', 'rz_mz_learn_update.h']
HEADERS = NET_HEADERS + ENGINE_HEADERS + MUZERO_HEADERS + REPLAY_HEADERS + MZ_REPLAY_HEADERS + MZ_LEARN_HEADERS


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
    assert NET_HEADERS == ['rz_net_dev.h', 'rz_net_f32.h', 'rz_net_heads.h', 'rz_net_rows.h', 'rz_net_split.h', 'rz_delta.h']
    assert ENGINE_HEADERS == ['rz_engine_deferred.h', 'rz_engine_eval.h', 'rz_engine_ml.h', 'rz_engine_play.h', 'rz_engine_roots.h',
                              'rz_engine_step.h']
    assert MUZERO_HEADERS == ['rz_muzero_hot.h', 'rz_muzero_moves.h', 'rz_muzero_noise.h', 'rz_muzero_roots.h', 'rz_muzero_search.h',
                              'rz_muzero_step.h', 'rz_muzero_tree.h']
    for names in (REPLAY_HEADERS, MZ_REPLAY_HEADERS, MZ_LEARN_HEADERS):
        for name in names:
            assert os.path.isfile(os.path.join(CSRC, name)), name
    # every header with a kernel of the three belongs to a family: no other header beside the sources holds __global__
    kernel_headers = set()
    for path in glob.glob(os.path.join(CSRC, 'rz_replay*.h')) + glob.glob(os.path.join(CSRC, 'rz_mz_replay*.h')) + glob.glob(os.path.join(CSRC, 'rz_mz_learn*.h')):
        with open(path) as f:
            if '__global__' in f.read():
                kernel_headers.add(os.path.basename(path))
    assert kernel_headers <= set(REPLAY_HEADERS + MZ_REPLAY_HEADERS + MZ_LEARN_HEADERS)
    for source, names in (('rz_net.hip', NET_HEADERS), ('rz_engine.hip', ENGINE_HEADERS), ('rz_muzero.hip', MUZERO_HEADERS),
                          ('rz_replay.hip', REPLAY_HEADERS), ('rz_mz_replay.hip', MZ_REPLAY_HEADERS), ('rz_mz_learn.hip', MZ_LEARN_HEADERS)):
        with open(os.path.join(CSRC, source)) as f:
            text = f.read()
        for name in names:
            assert '#include "%s"' % name in text, name
        # the index of the file comment names every family header, and the includes stand in the order named here
        places = [text.index('#include "%s"' % name) for name in names]
        if source in ('rz_replay.hip', 'rz_mz_replay.hip', 'rz_mz_learn.hip'):
            assert places == sorted(places), source
            for name in names:
                assert '//   %s ' % name in text, name


def test_the_engine_source_is_host_code_only():
    with open(os.path.join(CSRC, 'rz_engine.hip')) as f:
        text = f.read()
    assert '__global__' not in text and '__device__' not in text


def test_the_muzero_source_is_host_code_only():
    with open(os.path.join(CSRC, 'rz_muzero.hip')) as f:
        text = f.read()
    assert '__global__' not in text and '__device__' not in text


@pytest.mark.parametrize('source', ['rz_replay.hip', 'rz_mz_replay.hip', 'rz_mz_learn.hip'])
def test_the_replay_and_learner_sources_are_host_code_only(source):
    with open(os.path.join(CSRC, source)) as f:
        text = f.read()
    assert '__global__' not in text and '__device__' not in text


# (rz_host.h: the host-side runtime all six sources include -- no kernel family, but a header that must stand alone like the others;
# rz_tree.h and rz_trace.h: the device code both translation units' kernels call; rz_mz_pack.h: the host arithmetic whose sizes
# rz_muzero.hip's headers take; rz_ring.h: the ring of both replay stores, plain C++ with no attribute like rz_mz_pack.h)
@pytest.mark.parametrize('header', HEADERS + ['rz_host.h', 'rz_tree.h', 'rz_trace.h', 'rz_mz_pack.h', 'rz_ring.h'])
def test_a_kernel_header_compiles_alone(header):
    done = syntax_only(header)
    assert done.returncode == 0, done.stdout.decode(errors='replace')[-4000:]


def test_the_profile_build_compiles():
    done = syntax_only('rz_net.hip', '-DRZ_NET_PROFILE')
    assert done.returncode == 0, done.stdout.decode(errors='replace')[-4000:]


def test_the_muzero_profile_build_compiles():
    done = syntax_only('rz_muzero.hip', '-DRZ_MZ_PROFILE')
    assert done.returncode == 0, done.stdout.decode(errors='replace')[-4000:]


# ---------------------------------------------------------------- _build.headers_of against the preprocessor

def project_headers_read(src):
    """The files under include/ and rlzero_amd/csrc/ that the preprocessor opens for `src` (hipcc -MM: nothing is compiled)."""
    cmd = [HIPCC] + _build.FLAGS + ['-I' + os.path.join(REPO, 'include'), '-MM', src]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert done.returncode == 0, done.stderr.decode(errors='replace')[-4000:]
    words = done.stdout.decode().replace('\\\n', ' ').split()
    paths = {os.path.realpath(w) for w in words if not w.endswith(':')}
    roots = (os.path.realpath(os.path.join(REPO, 'include')) + os.sep, os.path.realpath(CSRC) + os.sep)
    return {p for p in paths if p.startswith(roots)} - {os.path.realpath(src)}


@pytest.mark.parametrize('src', _build.SOURCES, ids=os.path.basename)
def test_an_object_depends_on_every_header_its_source_reads(src):
    read = project_headers_read(src)
    assert read, 'hipcc -MM lists no project header for %s' % src
    known = {os.path.realpath(p) for p in _build.headers_of(src)}
    assert read <= known, sorted(read - known)


def test_a_family_header_belongs_to_its_translation_unit_alone():
    sets = {os.path.basename(src): {os.path.basename(p) for p in _build.headers_of(src)} for src in _build.SOURCES}
    assert [name for name, hs in sets.items() if 'rz_engine_play.h' in hs] == ['rz_engine.hip']
    assert [name for name, hs in sets.items() if 'rz_muzero_search.h' in hs] == ['rz_muzero.hip']
    assert [name for name, hs in sets.items() if 'rz_replay_batch.h' in hs] == ['rz_replay.hip']
    assert [name for name, hs in sets.items() if 'rz_mz_replay_prio.h' in hs] == ['rz_mz_replay.hip']
    assert [name for name, hs in sets.items() if 'rz_mz_learn_grad.h' in hs] == ['rz_mz_learn.hip']
    assert 'rz_ring.h' in sets['rz_replay.hip'] and 'rz_ring.h' in sets['rz_mz_replay.hip'] and 'rz_ring.h' not in sets['rz_mz_learn.hip']
    assert 'rz_tree.h' in sets['rz_engine.hip'] and 'rz_tree.h' in sets['rz_net.hip']
    assert 'rz_mz_learn.h' not in sets['rz_net.hip']
