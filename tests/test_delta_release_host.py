"""The three-wave split of a leaf's gather (rlzero_amd/csrc/rz_gather.h: Split<3> and the functions' <3> forms), on the CPU.

In the handed pass of the resident search (k_delta_res) wave 0 finishes the selection and runs conv1; waves 1 .. 3 -- gathering waves
0 .. 2 -- copy the base's records: 12 conv2 / 24 conv1 records a round, 14 / 6 rounds, a table of 104 entries a wave.  A driver with its
own main plays the FOUR waves lane by lane the way delta_passes<true> uses the header: wave 0 goes through the same instructions with
no place of its own (gathering wave -1) and no record anywhere.  It reports per (set, round, wave, lane) the offset requested from
the base and the byte of the layer's LDS records it is stored to (-1: nothing stored).  The same is restated in numpy and compared
element by element; the driver is also built with -fsanitize=address,undefined and run (the tables are heap arrays of exactly
Split<3>::kTabEntries entries, read with bounds checks)."""
import tempfile

import numpy as np
import pytest

import host_driver

C1_MAX, C2_MAX = 128, 164          # records a pass may hold (rz_delta.h: kC1Slots, kC2Slots)
P1, P2 = 160, 288                  # bytes from one LDS record to the next (rz_delta.h: P1, P2)
BASE_C2 = 256 * 128                # the conv2 records' place in a base: behind 256 conv1 records of 128 bytes
OUTSIDE = 1 << 30
NW = 3                             # gathering waves
C1 = dict(rounds=6, lanes=8, per_wave=8, per_round=24, bytes=128, pitch=P1, base=0, hmax=C1_MAX)
C2 = dict(rounds=14, lanes=16, per_wave=4, per_round=12, bytes=256, pitch=P2, base=BASE_C2, hmax=C2_MAX)
TAB = 14 * 4 + 6 * 8               # entries of a gathering wave's table
C1_COUNTS = (0, 23, 24, 25, 127, 128)
C2_COUNTS = (0, 1, 11, 12, 13, 163, 164)

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rz_gather.h"

typedef rzg::Split<3> GS;
static_assert(GS::kC1Rounds == 6 && GS::kC2Rounds == 14 && GS::kTabEntries == 104, "the three-wave split");

int main(int argc, char **argv) {   // gather3 pitch1 pitch2 base_c2 sets.bin out.bin
    if (argc != 6) return 4;
    const int pitch1 = atoi(argv[1]), pitch2 = atoi(argv[2]), base_c2 = atoi(argv[3]);
    FILE *f = fopen(argv[4], "rb");
    if (!f) { perror(argv[4]); return 2; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint64_t> sets((size_t)bytes / 8);
    if (bytes && fread(sets.data(), 1, (size_t)bytes, f) != (size_t)bytes) return 2;
    fclose(f);
    const size_t n_cases = sets.size() / 16;
    constexpr int per_case = 2 + (GS::kC1Rounds + GS::kC2Rounds) * 4 * 64 * 2;
    std::vector<int32_t> out(n_cases * per_case);
    for (size_t c = 0; c < n_cases; ++c) {
        uint64_t W[4][rzg::kWords];   // the windows of radius 1 .. 4
        for (int r = 0; r < 4; ++r)
            for (int w = 0; w < rzg::kWords; ++w) W[r][w] = sets[c * 16 + r * 4 + w];
        int32_t *o = out.data() + c * per_case;
        int32_t *o1 = o + 2, *o2 = o1 + GS::kC1Rounds * 4 * 64 * 2;
        for (int wave = 0; wave < 4; ++wave) {
            // (delta_passes<true>: gathering wave gw = wave - 1; wave 0 has no place of its own, reads the entries of gathering wave 0's
            // rounds from a table nobody wrote and has no record)
            const int gw = wave - 1, gwi = gw < 0 ? 0 : gw;
            const bool gathers = gw >= 0;
            std::vector<uint16_t> tab(GS::kTabEntries, (uint16_t)0xffff);   // (what an earlier leaf left there)
            // held records / slots in the words before word w, and in all, the way delta_passes<true> forms them: from the per-word
            // popcounts the hand-over stores behind the sets (cnt[radius - 1][word]); a held set's count is a DIFFERENCE of two of
            // them, which is right because W1 <= W3 and W2 <= W4 word by word
            int cnt[4][rzg::kWords], pn1[rzg::kWords + 1] = {0}, ps1[rzg::kWords + 1] = {0}, pn2[rzg::kWords + 1] = {0}, ps2[rzg::kWords + 1] = {0};
            for (int r = 0; r < 4; ++r)
                for (int w = 0; w < rzg::kWords; ++w) cnt[r][w] = rzg::popcount(W[r][w]);
            for (int w = 0; w < rzg::kWords; ++w) {
                pn1[w + 1] = pn1[w] + cnt[2][w] - cnt[0][w], ps1[w + 1] = ps1[w] + cnt[2][w];
                pn2[w + 1] = pn2[w] + cnt[3][w] - cnt[1][w], ps2[w + 1] = ps2[w] + cnt[3][w];
                // ... and they are the held words' own popcounts
                if (cnt[2][w] - cnt[0][w] != rzg::popcount(rzg::held(W[2][w], W[0][w]))) return 10;
                if (cnt[3][w] - cnt[1][w] != rzg::popcount(rzg::held(W[3][w], W[1][w]))) return 10;
            }
            for (int w = 0; w < rzg::kWords; ++w) {
                const int n1 = pn1[w], s1 = ps1[w], n2 = pn2[w], s2 = ps2[w];
                const uint64_t h1 = rzg::held(W[2][w], W[0][w]), h2 = rzg::held(W[3][w], W[1][w]);
                for (int lane = 0; lane < 64; ++lane) {
                    const int cell = 64 * w + lane;
                    if ((h1 >> lane) & 1ull) {
                        const int p = rzg::c1_place<3>(n1 + rzg::below(h1, lane), gw);
                        if (gathers && p >= 0) tab.at(p) = rzg::entry(cell, s1 + rzg::below(W[2][w], lane));
                        if (!gathers && p >= 0) return 9;   // a record fell to wave 0
                    }
                    if ((h2 >> lane) & 1ull) {
                        const int p = rzg::c2_place<3>(n2 + rzg::below(h2, lane), gw);
                        if (gathers && p >= 0) tab.at(p) = rzg::entry(cell, s2 + rzg::below(W[3][w], lane));
                        if (!gathers && p >= 0) return 9;
                    }
                }
            }
            const int n1 = pn1[rzg::kWords], n2 = pn2[rzg::kWords];
            o[0] = n1, o[1] = n2;
            for (int round = 0; round < GS::kC1Rounds; ++round)
                for (int lane = 0; lane < 64; ++lane) {
                    const int j = rzg::c1_record<3>(round, gwi, lane), chunk = rzg::c1_chunk(lane);
                    const bool has = gathers && rzg::c1_has(j, n1);
                    const uint16_t e = tab.at(rzg::c1_index<3>(j));
                    int32_t *q = o1 + ((round * 4 + wave) * 64 + lane) * 2;
                    q[0] = rzg::c1_src(has, rzg::entry_cell(e), chunk);
                    q[1] = has ? rzg::dst(rzg::entry_slot(e), chunk, pitch1) : -1;
                }
            for (int round = 0; round < GS::kC2Rounds; ++round)
                for (int lane = 0; lane < 64; ++lane) {
                    const int j = rzg::c2_record<3>(round, gwi, lane), chunk = rzg::c2_chunk(lane);
                    const bool has = gathers && rzg::c2_has(j, n2);
                    const uint16_t e = tab.at(rzg::c2_index<3>(j));
                    int32_t *q = o2 + ((round * 4 + wave) * 64 + lane) * 2;
                    q[0] = rzg::c2_src(has, rzg::entry_cell(e), chunk, base_c2);
                    q[1] = has ? rzg::dst(rzg::entry_slot(e), chunk, pitch2) : -1;
                }
        }
        if (rzg::c1_rounds<3>(o[0]) > GS::kC1Rounds && o[0] <= rzg::kC1Max) return 8;
        if (rzg::c2_rounds<3>(o[1]) > GS::kC2Rounds && o[1] <= rzg::kC2Max) return 8;
    }
    f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { perror(argv[5]); return 2; }
    fclose(f);
    return 0;
}
'''


# ---- the sets

def window_sets(n, changed):
    """W1 .. W4 of a leaf of an n x n board as bool [4][256]: the cells within Chebyshev distance r of a changed cell."""
    cells = np.arange(n * n)
    y, x = cells // n, cells % n
    d = np.full(n * n, 1000)
    for c in changed:
        d = np.minimum(d, np.maximum(np.abs(y - c // n), np.abs(x - c % n)))
    sets = np.zeros((4, 256), dtype=bool)
    for r in range(1, 5):
        sets[r - 1, :n * n] = d <= r
    return sets


def counted_sets(n1, n2, seed):
    """Sets that hold exactly n1 conv1 and n2 conv2 records: W1 = W2 = a few cells, W3 = W1 + n1 further cells, W4 = W2 + n2 further
    cells, scattered over the four words (the gather asks W1 <= W3 and W2 <= W4 only: the held sets are W3 & ~W1 and W4 & ~W2).  The
    slots W3 / W4 use stay within the budget: |W3| <= 128, |W4| <= 164."""
    rng = np.random.default_rng(seed)
    sets = np.zeros((4, 256), dtype=bool)
    inner = 0 if max(n1 - C1_MAX, n2 - C2_MAX) >= 0 else int(rng.integers(0, min(C1_MAX - n1, C2_MAX - n2) + 1))
    perm = rng.permutation(256)
    core, rest = perm[:inner], perm[inner:]
    sets[:, core] = True
    sets[2, rng.permutation(rest)[:n1]] = True
    sets[3, rng.permutation(rest)[:n2]] = True
    assert int((sets[2] & ~sets[0]).sum()) == n1 and int((sets[3] & ~sets[1]).sum()) == n2
    return sets


def words(sets):
    """bool [4][256] -> uint64 [16]: word w of a set = cells 64 w .. 64 w + 63, bit = cell & 63."""
    return np.packbits(sets.reshape(16, 64), axis=1, bitorder='little').view('<u8').reshape(16)


def in_budget(sets):
    n = sets.sum(axis=1)
    return n[0] <= 128 and n[1] <= 128 and n[2] <= C1_MAX and n[3] <= C2_MAX


def cases():
    """Every pair of the counts at the rounds' edges (twice, differently scattered); real leaves: single cells, word boundaries,
    corners, the fullest 16 x 16 budget, seeded samples; leaves past the budget."""
    out = []
    for k, (n1, n2) in enumerate((a, b) for a in C1_COUNTS for b in C2_COUNTS):
        out += [counted_sets(n1, n2, 10 * k), counted_sets(n1, n2, 10 * k + 1)]
    for n in (11, 15, 16):
        S = n * n
        out += [window_sets(n, (c, )) for c in range(0, S, 7)] + [window_sets(n, (S - 1, ))]
        out += [window_sets(n, (b - 1, b)) for b in (64, 128, 192) if b < S]
        out.append(window_sets(n, (0, n - 1, S - n, S - 1)))
        rng = np.random.default_rng(2000 + n)
        for k in (2, 3, 4):
            out += [window_sets(n, tuple(int(c) for c in rng.choice(S, size=k, replace=False))) for _ in range(30)]
    out.append(window_sets(16, (4 * 16 + 4, 11 * 16 + 11)))
    out.append(window_sets(16, (3 * 16 + 3, 3 * 16 + 12, 12 * 16 + 3)))   # three windows of radius 4 far apart: 192 > 164 conv2 slots
    return out


# ---- the restatement

def expected(sets, geo, outer, inner):
    """(src, dst) [rounds][4 waves][64 lanes] of one layer: record j = the j-th cell of H = W_outer & ~W_inner in ascending order, slot =
    the cell's rank in W_outer; round i gives record per_round i + per_wave gw + lane // lanes to the lane group of GATHERING wave gw =
    wave - 1, chunk = lane % lanes; wave 0 gets nothing."""
    src = np.full((geo['rounds'], 4, 64), OUTSIDE, dtype=np.int64)
    dst = np.full((geo['rounds'], 4, 64), -1, dtype=np.int64)
    W = sets[outer]
    H = W & ~sets[inner]
    slot_of = np.cumsum(W) - 1
    chunk = np.arange(geo['lanes'])
    for j, cell in enumerate(np.flatnonzero(H)):
        rnd, gw, group = j // geo['per_round'], (j // geo['per_wave']) % NW, j % geo['per_wave']
        if rnd >= geo['rounds'] or j >= geo['hmax']:   # (past the budget: such a leaf copies nothing)
            break
        lanes = group * geo['lanes'] + chunk
        src[rnd, 1 + gw, lanes] = geo['base'] + cell * geo['bytes'] + 16 * chunk
        dst[rnd, 1 + gw, lanes] = slot_of[cell] * geo['pitch'] + 16 * chunk
    return src, dst, H, slot_of


@pytest.fixture(scope='module')
def gathered():
    """(sets of each case, the plain driver's output, the sanitized driver's output)"""
    sets = cases()
    per_case = 2 + (C1['rounds'] + C2['rounds']) * 4 * 64 * 2
    with tempfile.TemporaryDirectory() as tmp:
        drv = host_driver.Driver(tmp, 'gather3', DRIVER)
        outs = drv.both([P1, P2, BASE_C2, *drv.write([np.stack([words(s) for s in sets]).astype('<u8')])], drv.fresh(1))
        plain, san = (np.fromfile(out, dtype='<i4').reshape(len(sets), per_case) for (out, ) in outs)
    return sets, plain, san


def split(row):
    n1, n2 = int(row[0]), int(row[1])
    a = row[2:2 + C1['rounds'] * 4 * 64 * 2].reshape(C1['rounds'], 4, 64, 2)
    b = row[2 + C1['rounds'] * 4 * 64 * 2:].reshape(C2['rounds'], 4, 64, 2)
    return n1, n2, a, b


def test_the_split_is_the_one_the_kernel_counts_on():
    """164 conv2 records at 12 a round: 14 rounds; 128 conv1 records at 24 a round: 6 rounds; 104 entries fit a wave's 128-entry row."""
    assert -(-C2_MAX // C2['per_round']) == C2['rounds'] == 14 and -(-C1_MAX // C1['per_round']) == C1['rounds'] == 6
    assert TAB == 104 <= 128
    assert C2['per_round'] == NW * C2['per_wave'] and C1['per_round'] == NW * C1['per_wave']


def test_cases_cover_the_counts():
    """Every count the rounds' edges ask for occurs, alone and with every count of the other layer, inside the budget."""
    seen = set()
    for s in cases():
        if in_budget(s):
            seen.add((int((s[2] & ~s[0]).sum()), int((s[3] & ~s[1]).sum())))
    assert {(a, b) for a in C1_COUNTS for b in C2_COUNTS} <= seen
    assert not all(in_budget(s) for s in cases())


def test_every_chunk_once_to_its_slot_and_none_to_wave_0(gathered):
    """Inside the budget: every (held cell, 16-byte chunk) is requested by exactly one lane of one round of waves 1 .. 3 and stored at
    its slot's address; every other lane -- all of wave 0 -- requests the offset past the buffer's end and stores nothing."""
    sets, got, _ = gathered
    checked = 0
    for k, (s, row) in enumerate(zip(sets, got)):
        n1, n2, g1, g2 = split(row)
        for geo, g, cnt, outer, inner in ((C1, g1, n1, 2, 0), (C2, g2, n2, 3, 1)):
            src, dst, H, slot_of = expected(s, geo, outer, inner)
            assert cnt == int(H.sum()), k
            if not in_budget(s):
                continue
            assert cnt <= geo['hmax'] and -(-cnt // geo['per_round']) <= geo['rounds']
            assert np.array_equal(g[..., 0], src) and np.array_equal(g[..., 1], dst), k
            # the properties themselves, from the driver's output alone
            assert (g[:, 0, :, 0] == OUTSIDE).all() and (g[:, 0, :, 1] == -1).all(), k   # no record goes to wave 0
            moved = g[..., 0] != OUTSIDE
            assert np.array_equal(moved, g[..., 1] >= 0)
            want = sorted((geo['base'] + c * geo['bytes'] + 16 * i, slot_of[c] * geo['pitch'] + 16 * i) for c in np.flatnonzero(H) for i in range(geo['lanes']))
            have = sorted(zip(g[..., 0][moved].tolist(), g[..., 1][moved].tolist()))
            assert have == want, k
            assert len(set(d for _, d in have)) == len(have)   # no LDS byte is written twice
            assert g[..., 1].max(initial=-1) < geo['hmax'] * geo['pitch']
            checked += 1
    assert checked > 600


def test_past_the_budget_nothing_leaves_the_tables(gathered):
    """A leaf past the budget (it takes the passes without a base; nothing of the gather is stored): the requests stay inside the
    base's records or past the buffer's end, the stores inside the layer's records, and wave 0 still moves nothing."""
    sets, got, _ = gathered
    seen = 0
    for s, row in zip(sets, got):
        if in_budget(s):
            continue
        seen += 1
        _, _, g1, g2 = split(row)
        for geo, g in ((C1, g1), (C2, g2)):
            src, dst = g[..., 0], g[..., 1]
            inside = src != OUTSIDE
            assert (src[inside] >= geo['base']).all() and (src[inside] < geo['base'] + 256 * geo['bytes']).all()
            assert (dst >= -1).all() and (dst < 256 * geo['pitch']).all()
            assert not inside[:, 0].any() and (dst[:, 0] == -1).all()
    assert seen > 0


def test_sanitized_driver_agrees(gathered):
    """The driver built with -fsanitize=address,undefined ran over all inputs without a report (it would have exited non-zero) and
    wrote the same bytes."""
    _, got, san = gathered
    assert np.array_equal(got, san)
