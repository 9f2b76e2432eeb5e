"""Whole MuZero moves for any environment the library knows (rz_mz_play_env, ABI 42), without a GPU: the entry point is exported and
bound, and the binding's play record is the header's -- its size and every field's offset, read from a program compiled against
include/rlzero_hip.h with ROCm's clang++ (tests/test_abi.py and tests/test_mz_env_host.py state their records' sizes by hand; here the
header answers for itself).  The environment trait in csrc/rz_mz_env.h gained no member for this feature -- the kernel's LDS record is
the trait's own load / store, its observation rows the trait's own observe, which tests/test_mz_env_host.py already holds equal to the
twins bit for bit -- so there is no new plain C++ to drive here."""
import ctypes
import inspect
import os
import re

from conftest import REPO
import host_driver

HEADER = os.path.join(REPO, 'include', 'rlzero_hip.h')


def header_text():
    return open(HEADER).read()


def test_play_env_is_exported_declared_and_bound():
    from rlzero_amd import _hip
    assert 'rz_mz_play_env' in _hip.exported_symbols()
    assert _hip.ABI_VERSION >= 42 and '#define RZ_ABI_VERSION %d' % _hip.ABI_VERSION in header_text()
    code = re.sub(r'/\*.*?\*/', '', header_text(), flags=re.S)
    proto = re.search(r'int rz_mz_play_env\(([^)]*)\);', code)
    assert proto and [a.split()[-1].lstrip('*') for a in proto.group(1).split(',')] == ['e', 'kind', 'd_hidden', 'n_sims', 'n_moves', 'play', 'stream']
    assert 'const rz_mz_whole_play *play' in proto.group(1)
    # rz_mz_play_cartpole keeps its signature
    assert ('int rz_mz_play_cartpole(rz_muzero *e, float *d_hidden, int32_t n_sims, int32_t n_moves, const rz_mz_cartpole_play *play, '
            'void *stream);') in code
    from rlzero_amd import _build
    lib = ctypes.CDLL(_build.build(verbose=False))
    assert hasattr(lib, 'rz_mz_play_env') and hasattr(lib, 'rz_mz_play_cartpole')
    restype, argtypes = _hip._SIGNATURES['rz_mz_play_env']
    assert restype is ctypes.c_int and len(argtypes) == 7 and argtypes[5]._type_ is _hip.RzMzWholePlay
    from rlzero_amd.muzero.tree import MuZeroTree
    params = list(inspect.signature(MuZeroTree.play_env).parameters)
    assert params[:5] == ['self', 'hidden', 'n_sims', 'n_moves', 'env'] and params[-2:] == ['kind', 'max_episode_steps']
    assert list(inspect.signature(MuZeroTree.play_cartpole).parameters) == params[:-2]


def test_play_record_is_the_headers(tmp_path):
    """sizeof and offsetof of every field of rz_mz_whole_play (and of rz_mz_cartpole_play, whose fields it begins with) from the
    compiled header against the ctypes structures."""
    from rlzero_amd import _hip
    records = {'rz_mz_whole_play': _hip.RzMzWholePlay, 'rz_mz_cartpole_play': _hip.RzMzCartPolePlay}
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "rlzero_hip.h"', 'int main() {']
    for name, cls in sorted(records.items()):
        lines.append('    std::printf("%s size %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in cls._fields_:
            lines.append('    std::printf("%s %s %%zu\\n", offsetof(%s, %s));' % (name, field, name, field))
    lines += ['    return 0;', '}']
    out = host_driver.probe(tmp_path, '\n'.join(lines) + '\n').decode().split('\n')
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out if ln}
    want = {}
    for name, cls in records.items():
        want[(name, 'size')] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            want[(name, field)] = getattr(cls, field).offset
    assert got == want
    # the new record is the old one followed by the time limit
    assert [f for f, _ in _hip.RzMzWholePlay._fields_] == [f for f, _ in _hip.RzMzCartPolePlay._fields_] + ['max_episode_steps']
    assert want[('rz_mz_whole_play', 'size')] == 144 and want[('rz_mz_whole_play', 'max_episode_steps')] == 136
    for field, _ in _hip.RzMzCartPolePlay._fields_:
        assert want[('rz_mz_whole_play', field)] == want[('rz_mz_cartpole_play', field)]


def test_the_route_is_opt_in():
    """The defaults of the self-play object and of the trainer do not change: whole moves for Acrobot are asked for."""
    import importlib.util
    from rlzero_amd.muzero.selfplay import MuZeroSelfPlay
    assert inspect.signature(MuZeroSelfPlay.__init__).parameters['fused_moves'].default is None
    spec = importlib.util.spec_from_file_location('train_muzero', os.path.join(REPO, 'tools', 'train_muzero.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert inspect.signature(mod.MuZeroPipeline.__init__).parameters['whole_moves'].default is None
    ap = mod.build_parser()
    assert ap.parse_args([]).whole_moves is False and ap.parse_args(['--env', 'acrobot', '--whole-moves']).whole_moves is True
