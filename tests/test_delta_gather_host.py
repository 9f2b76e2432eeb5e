"""Which lane moves which 16 bytes of a leaf's base records (rlzero_amd/csrc/rz_gather.h), on the CPU.

A driver with its own main is compiled against the header with ROCm's clang++ (by tests/host_driver.py).  It plays the four
waves of a workgroup lane by lane with the header's functions, the way delta_passes<SETS> uses them: every wave writes the table
entries of the held cells whose records fall to it, reads the entries of its rounds back, and reports per (set, round, wave, lane)
the offset requested from the base and the byte of the layer's LDS records it is stored to (-1: nothing stored).  The same is
restated in numpy from the header's opening comment and compared element by element.

The window sets of a leaf are restated here as well: cells within Chebyshev distance r = 1 .. 4 of a changed cell, on the board.
The same driver is also built with -fsanitize=address,undefined and run over all inputs (the tables are heap arrays of exactly
rzg::kTabEntries entries)."""
import tempfile

import numpy as np
import pytest

import host_driver

BOARDS = [11, 13, 15, 16]
C1_MAX, C2_MAX = 128, 164          # records a pass may hold (rz_delta.h: kC1Slots, kC2Slots)
T1_CELLS, T2_CELLS, T3_CELLS = 128, 128, 128   # cells conv1 / conv2 / conv3 may compute: 4 tiles of 32, 8 of 16, 8 of 16
P1, P2 = 160, 288                  # bytes from one LDS record to the next (rz_delta.h: P1, P2)
BASE_C2 = 256 * 128                # the conv2 records' place in a base: behind 256 conv1 records of 128 bytes
OUTSIDE = 1 << 30
C1 = dict(rounds=4, lanes=8, per_wave=8, per_round=32, bytes=128, pitch=P1, base=0, hmax=C1_MAX)
C2 = dict(rounds=11, lanes=16, per_wave=4, per_round=16, bytes=256, pitch=P2, base=BASE_C2, hmax=C2_MAX)

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rz_gather.h"

int main(int argc, char **argv) {   // gather pitch1 pitch2 base_c2 sets.bin out.bin
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
    constexpr int per_case = 2 + (rzg::kC1Rounds + rzg::kC2Rounds) * 4 * 64 * 2;
    std::vector<int32_t> out(n_cases * per_case);
    for (size_t c = 0; c < n_cases; ++c) {
        uint64_t W[4][rzg::kWords];   // the windows of radius 1 .. 4
        for (int r = 0; r < 4; ++r)
            for (int w = 0; w < rzg::kWords; ++w) W[r][w] = sets[c * 16 + r * 4 + w];
        int32_t *o = out.data() + c * per_case;
        int32_t *o1 = o + 2, *o2 = o1 + rzg::kC1Rounds * 4 * 64 * 2;
        for (int wave = 0; wave < 4; ++wave) {
            std::vector<uint16_t> tab(rzg::kTabEntries, (uint16_t)0xffff);   // (what an earlier leaf left there)
            int n1 = 0, s1 = 0, n2 = 0, s2 = 0;   // held records / slots in the words before this one
            for (int w = 0; w < rzg::kWords; ++w) {
                const uint64_t h1 = rzg::held(W[2][w], W[0][w]), h2 = rzg::held(W[3][w], W[1][w]);
                for (int lane = 0; lane < 64; ++lane) {
                    const int cell = 64 * w + lane;
                    if ((h1 >> lane) & 1ull) {
                        const int p = rzg::c1_place(n1 + rzg::below(h1, lane), wave);
                        if (p >= 0) tab.at(p) = rzg::entry(cell, s1 + rzg::below(W[2][w], lane));
                    }
                    if ((h2 >> lane) & 1ull) {
                        const int p = rzg::c2_place(n2 + rzg::below(h2, lane), wave);
                        if (p >= 0) tab.at(p) = rzg::entry(cell, s2 + rzg::below(W[3][w], lane));
                    }
                }
                n1 += rzg::popcount(h1), s1 += rzg::popcount(W[2][w]);
                n2 += rzg::popcount(h2), s2 += rzg::popcount(W[3][w]);
            }
            o[0] = n1, o[1] = n2;
            for (int round = 0; round < rzg::kC1Rounds; ++round)
                for (int lane = 0; lane < 64; ++lane) {
                    const int j = rzg::c1_record(round, wave, lane), chunk = rzg::c1_chunk(lane);
                    const bool has = rzg::c1_has(j, n1);
                    const uint16_t e = tab.at(rzg::c1_index(j));
                    int32_t *q = o1 + ((round * 4 + wave) * 64 + lane) * 2;
                    q[0] = rzg::c1_src(has, rzg::entry_cell(e), chunk);
                    q[1] = has ? rzg::dst(rzg::entry_slot(e), chunk, pitch1) : -1;
                }
            for (int round = 0; round < rzg::kC2Rounds; ++round)
                for (int lane = 0; lane < 64; ++lane) {
                    const int j = rzg::c2_record(round, wave, lane), chunk = rzg::c2_chunk(lane);
                    const bool has = rzg::c2_has(j, n2);
                    const uint16_t e = tab.at(rzg::c2_index(j));
                    int32_t *q = o2 + ((round * 4 + wave) * 64 + lane) * 2;
                    q[0] = rzg::c2_src(has, rzg::entry_cell(e), chunk, base_c2);
                    q[1] = has ? rzg::dst(rzg::entry_slot(e), chunk, pitch2) : -1;
                }
        }
        // the other lookups of the header, against each other: record j -> cell -> record j, the counts
        uint64_t H2[rzg::kWords], H1[rzg::kWords];
        for (int w = 0; w < rzg::kWords; ++w) H1[w] = rzg::held(W[2][w], W[0][w]), H2[w] = rzg::held(W[3][w], W[1][w]);
        if (rzg::count(H1) != o[0] || rzg::count(H2) != o[1]) return 5;
        for (int j = 0; j < o[1]; ++j)
            if (rzg::rank(H2, rzg::cell_of(H2, j)) != j) return 6;
        for (int j = 0; j < o[0]; ++j)
            if (rzg::rank(H1, rzg::cell_of(H1, j)) != j) return 6;
        if (rzg::cell_of(H1, o[0]) != -1 || rzg::cell_of(H2, o[1]) != -1) return 7;
        if (rzg::c1_rounds(o[0]) > rzg::kC1Rounds && o[0] <= rzg::kC1Max) return 8;
        if (rzg::c2_rounds(o[1]) > rzg::kC2Rounds && o[1] <= rzg::kC2Max) return 8;
    }
    f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { perror(argv[5]); return 2; }
    fclose(f);
    return 0;
}
'''


# ---- the leaves

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


def words(sets):
    """bool [4][256] -> uint64 [16]: word w of a set = cells 64 w .. 64 w + 63, bit = cell & 63."""
    return np.packbits(sets.reshape(16, 64), axis=1, bitorder='little').view('<u8').reshape(16)


def in_budget(sets):
    n = sets.sum(axis=1)
    return n[0] <= T1_CELLS and n[1] <= T2_CELLS and n[2] <= min(T3_CELLS, C1_MAX) and n[3] <= C2_MAX


def leaves():
    """(board, changed cells) of every case: each single cell; the pairs on both sides of a word boundary; the four corners; the
    fullest budget a board admits; seeded samples of 2, 3 and 4 cells."""
    out = []
    for n in BOARDS:
        S = n * n
        out += [(n, (c, )) for c in range(S)]
        out += [(n, (b - 1, b)) for b in (64, 128, 192) if b < S]
        out += [(n, (b - 1, b, c)) for b in (64, 128, 192) if b < S for c in (0, S - 1)]
        corners = (0, n - 1, S - n, S - 1)
        out.append((n, corners))
        out += [(n, (a, b)) for a in corners for b in corners if a < b]
        rng = np.random.default_rng(1000 + n)
        for k in (2, 3, 4):
            out += [(n, tuple(int(c) for c in rng.choice(S, size=k, replace=False))) for _ in range(60)]
    out.append((16, (4 * 16 + 4, 11 * 16 + 11)))
    return out


# ---- the restatement

def expected(sets, geo, outer, inner):
    """(src, dst) [rounds][4 waves][64 lanes] of one layer: record j = the j-th cell of H = W_outer & ~W_inner in ascending order, slot
    = the cell's rank in W_outer; round i gives record per_round i + per_wave wave + lane // lanes to the lane group, chunk = lane % lanes."""
    src = np.full((geo['rounds'], 4, 64), OUTSIDE, dtype=np.int64)
    dst = np.full((geo['rounds'], 4, 64), -1, dtype=np.int64)
    W = sets[outer]
    H = W & ~sets[inner]
    slot_of = np.cumsum(W) - 1
    chunk = np.arange(geo['lanes'])
    for j, cell in enumerate(np.flatnonzero(H)):
        rnd, wave, group = j // geo['per_round'], (j // geo['per_wave']) % 4, j % geo['per_wave']
        if rnd >= geo['rounds']:   # (past the budget: such a leaf copies nothing)
            break
        lanes = group * geo['lanes'] + chunk
        src[rnd, wave, lanes] = geo['base'] + cell * geo['bytes'] + 16 * chunk
        dst[rnd, wave, lanes] = slot_of[cell] * geo['pitch'] + 16 * chunk
    return src, dst, H, slot_of


@pytest.fixture(scope='module')
def gathered():
    """(cases, sets of each, the plain driver's output, the sanitized driver's output)"""
    cases = leaves()
    sets = [window_sets(n, ch) for n, ch in cases]
    per_case = 2 + (C1['rounds'] + C2['rounds']) * 4 * 64 * 2
    with tempfile.TemporaryDirectory() as tmp:
        drv = host_driver.Driver(tmp, 'gather', DRIVER)
        outs = drv.both([P1, P2, BASE_C2, *drv.write([np.stack([words(s) for s in sets]).astype('<u8')])], drv.fresh(1))
        plain, san = (np.fromfile(out, dtype='<i4').reshape(len(cases), per_case) for (out, ) in outs)
    return cases, sets, plain, san


def split(row):
    n1, n2 = int(row[0]), int(row[1])
    a = row[2:2 + C1['rounds'] * 4 * 64 * 2].reshape(C1['rounds'], 4, 64, 2)
    b = row[2 + C1['rounds'] * 4 * 64 * 2:].reshape(C2['rounds'], 4, 64, 2)
    return n1, n2, a, b


def test_cases_cover_the_edges():
    """The cases hold what they are meant to: cell 255, three- and four-word boards, the fullest leaf, leaves past the budget."""
    cases = leaves()
    assert (16, (255, )) in cases and (13, (168, )) in cases and (11, (63, 64)) in cases and (15, (191, 192)) in cases
    full = window_sets(16, (4 * 16 + 4, 11 * 16 + 11))
    # two 9 x 9 windows off every edge that share the four cells (7 .. 8, 7 .. 8): 158 of the 164 conv2 slots, 98 of the 128 conv1 slots;
    # 108 conv2 and 80 conv1 records are copied
    assert full.sum(axis=1).tolist() == [18, 50, 98, 158] and in_budget(full)
    assert int((full[3] & ~full[1]).sum()) == 108 and int((full[2] & ~full[0]).sum()) == 80
    budget = [in_budget(window_sets(n, ch)) for n, ch in cases]
    assert not all(budget) and sum(budget) > 1000


def test_every_chunk_once_to_its_slot(gathered):
    """Inside the budget: every (held cell, 16-byte chunk) is requested by exactly one lane of one round and stored at its slot's
    address; every other lane requests the offset past the buffer's end and stores nothing; 11 / 4 rounds suffice.  The lane is the
    one the work split names."""
    cases, sets, got, _ = gathered
    checked = 0
    for (n, ch), s, row in zip(cases, sets, got):
        n1, n2, g1, g2 = split(row)
        for geo, g, cnt, outer, inner in ((C1, g1, n1, 2, 0), (C2, g2, n2, 3, 1)):
            src, dst, H, slot_of = expected(s, geo, outer, inner)
            assert cnt == int(H.sum()), (n, ch)
            if not in_budget(s):
                continue
            assert cnt <= geo['hmax'] and -(-cnt // geo['per_round']) <= geo['rounds']
            assert np.array_equal(g[..., 0], src) and np.array_equal(g[..., 1], dst), (n, ch)
            # the property itself, from the driver's output alone
            moved = g[..., 0] != OUTSIDE
            assert np.array_equal(moved, g[..., 1] >= 0)
            want = sorted((geo['base'] + c * geo['bytes'] + 16 * k, slot_of[c] * geo['pitch'] + 16 * k) for c in np.flatnonzero(H) for k in range(geo['lanes']))
            have = sorted(zip(g[..., 0][moved].tolist(), g[..., 1][moved].tolist()))
            assert have == want, (n, ch)
            assert len(set(d for _, d in have)) == len(have)   # no LDS byte is written twice
            assert g[..., 1].max(initial=-1) < geo['hmax'] * geo['pitch']
            checked += 1
    assert checked > 2000


def test_past_the_budget_nothing_leaves_the_tables(gathered):
    """A leaf past the budget (it takes the passes without a base; nothing of the gather is stored): the requests stay inside the
    base's records or past the buffer's end, the stores inside the layer's records."""
    cases, sets, got, _ = gathered
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
    assert seen > 0


def test_sanitized_driver_agrees(gathered):
    """The driver built with -fsanitize=address,undefined ran over all inputs without a report (it would have exited non-zero) and
    wrote the same bytes."""
    _, _, got, san = gathered
    assert np.array_equal(got, san)
