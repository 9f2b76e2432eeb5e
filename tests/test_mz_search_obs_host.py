"""What rz_mz_load_root_model uploads (rlzero_amd/csrc/rz_mz_pack.h: pack_root_model), on the CPU: a stand-alone driver -- built plain
and under the address and undefined-behaviour sanitizers by tests/host_driver.py -- packs the four representation tensors, and the
vector is restated in numpy from the header's comment and compared bit for bit, the zero rows of rep1 included."""
import numpy as np
import pytest

import host_driver

f32 = np.float32
H, ROOT_OBS = 64, 16

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include "rz_mz_pack.h"

static std::vector<float> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<float> v((size_t)n / sizeof(float));
    if (n && fread(v.data(), 1, (size_t)n, f) != (size_t)n) exit(2);
    fclose(f);
    return v;
}

int main(int argc, char **argv) {   // root obs_dim rep1.w rep1.b rep2.w rep2.b -> the packed floats, the four offsets (as floats)
    using namespace rzmp;
    static_assert(kMzRootObs == 16 && kMzH == 64, "the sizes the test is written for");
    if (argc != 9) return 4;
    const int D = atoi(argv[2]);
    const std::vector<float> t[4] = {slurp(argv[3]), slurp(argv[4]), slurp(argv[5]), slurp(argv[6])};
    if (t[0].size() != (size_t)64 * D || t[1].size() != 64 || t[2].size() != 64 * 64 || t[3].size() != 64) return 3;
    const float *p[4] = {t[0].data(), t[1].data(), t[2].data(), t[3].data()};
    const Representation r = pack_root_model(p, D);
    const float off[4] = {(float)r.off[0], (float)r.off[1], (float)r.off[2], (float)r.off[3]};
    FILE *a = fopen(argv[7], "wb"), *b = fopen(argv[8], "wb");
    if (!a || !b || fwrite(r.host.data(), 4, r.host.size(), a) != r.host.size() || fwrite(off, 4, 4, b) != 4) return 2;
    fclose(a);
    fclose(b);
    return 0;
}
'''

drv = host_driver.fixture('mz_root_pack', DRIVER)


@pytest.mark.parametrize('D', [1, 9, 16])
def test_the_root_model_is_packed_as_the_header_says(drv, D):
    rs = np.random.RandomState(40 + D)
    w1, b1, w2, b2 = [rs.standard_normal(s).astype(f32) for s in ((H, D), (H, ), (H, H), (H, ))]
    host, off = drv.run('root', [D], [w1, b1, w2, b2], [f32, f32])
    assert off.tolist() == [0, ROOT_OBS * H, ROOT_OBS * H + H, ROOT_OBS * H + H + H * H] and host.size == ROOT_OBS * H + H + H * H + H
    rep1 = np.zeros((ROOT_OBS, H), dtype=f32)
    rep1[:D] = w1.T   # k-major, rows obs_dim .. 15 zero
    want = np.concatenate((rep1.reshape(-1), b1, w2.T.reshape(-1), b2))
    assert host.view(np.uint32).tolist() == want.view(np.uint32).tolist()
