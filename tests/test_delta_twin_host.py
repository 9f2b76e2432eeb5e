"""rz_memo.h's twin rule on the CPU (tests/host_driver.py: plain and sanitized builds of a stand-alone driver): `twin_cell` -- the
lowest cell that is empty at the root, has no (t, OWN) entry and lies 7 or more from a and from b -- and `twin_source` -- where every
cell of a twin pass's leaf takes its value features from, and which entry its computed values are stored to -- are held element by
element against a numpy restatement on 15 x 15, 11 rows x 16 columns and 11 x 11.  Asserted besides: a twin's window, a's and b's are
pairwise disjoint; the cells within 3 of the twin take the BASE's values (the leaf has no stone there) and store to the twin's entry;
cases without a candidate answer -1 (a centre pair on 11 x 11; every far cell occupied or already filled); twins on the board's edge and
in a corner occur; and no 128-byte line is shared between entries -- a's, the twin's (both kind OWN) or b's (OPP_LAST)."""
import numpy as np
import pytest

import host_driver

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "rz_memo.h"

template <typename T> static std::vector<T> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v(n / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}
template <typename T> static void dump(const char *path, const std::vector<T> &v) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
}

// twin BH BW <pairs: int32 [n][2] = a, b> <empty: uint64 [n][4]> <bits: uint64 [n][8]>
//   -> <t int32 [n]> <sources int32 [n][BH * BW][3] = source, fills, slot (all -9 without a twin)> <entry byte ranges int32 [n][3][2]>
//      <int32 [7] = the constants>
int main(int argc, char **argv) {
    if (argc != 11 || std::string(argv[1]) != "twin") return 2;
    const int BH = atoi(argv[2]), BW = atoi(argv[3]), S = BH * BW;
    const std::vector<int32_t> pairs = slurp<int32_t>(argv[4]);
    const std::vector<uint64_t> empty = slurp<uint64_t>(argv[5]), bits = slurp<uint64_t>(argv[6]);
    const size_t n = pairs.size() / 2;
    std::vector<int32_t> ts(n), src(n * S * 3, -9), range(n * 6, -1);
    for (size_t i = 0; i < n; ++i) {
        const int a = pairs[2 * i], b = pairs[2 * i + 1];
        const int t = rzm::twin_cell(a, b, BW, S, empty.data() + 4 * i, bits.data() + i * rzm::kBitmapWords);
        ts[i] = t;
        if (t < 0) continue;
        for (int c = 0; c < S; ++c) {
            int fills = -2, slot = -2;
            src[(i * S + c) * 3] = rzm::twin_source_yx(c / BW, c % BW, a / BW, a % BW, b / BW, b % BW, t / BW, t % BW, &fills, &slot);
            src[(i * S + c) * 3 + 1] = fills;
            src[(i * S + c) * 3 + 2] = slot;
        }
        const int e[3] = {rzm::entry_index(rzm::kOwn, a, S), rzm::entry_index(rzm::kOppLast, b, S), rzm::entry_index(rzm::kOwn, t, S)};
        for (int k = 0; k < 3; ++k) {
            range[i * 6 + 2 * k] = e[k] * rzm::kEntryBytes + rzm::slot_offset(0, 0);
            range[i * 6 + 2 * k + 1] = e[k] * rzm::kEntryBytes + rzm::slot_offset(rzm::kSlots - 1, rzm::kFeatures - 1) + 3;
        }
    }
    dump(argv[7], ts);
    dump(argv[8], src);
    dump(argv[9], range);
    dump(argv[10], std::vector<int32_t>{rzm::kSrcBase, rzm::kSrcMemo, rzm::kSrcRun, rzm::kFromBase, rzm::kFromA, rzm::kFromTwin, rzm::kLineBytes});
    return 0;
}
'''

drv = host_driver.fixture('memo_twin_driver', DRIVER)

BOARDS = [(15, 15), (11, 16), (11, 11)]   # rows, columns


def _words(cells, n_words):
    w = np.zeros(n_words, dtype=np.uint64)
    for c in cells:
        w[c >> 6] |= np.uint64(1) << np.uint64(c & 63)
    return w


def _cases(BH, BW):
    S = BH * BW
    rng = np.random.RandomState(7 * BH + BW)
    pairs, empty, bits, own_sets, empty_sets = [], [], [], [], []

    def add(a, b, emp, own):
        pairs.append((a, b))
        empty.append(_words(emp, 4))
        bits.append(np.concatenate([_words(own, 4), _words([b], 4)]))
        own_sets.append(set(own))
        empty_sets.append(set(emp))

    centre = (BH // 2) * BW + BW // 2
    every = list(range(S))
    far = [(a, b) for a in (0, BW - 1, S - BW, S - 1, centre, BW // 2, centre - BW // 2) for b in every
           if max(abs(a // BW - b // BW), abs(a % BW - b % BW)) >= 7]
    for a, b in far[::5]:
        rest = [c for c in every if c not in (a, b)]
        add(a, b, every, [])                                             # the empty board: the lowest far cell, often the corner 0
        add(a, b, every, [c for c in every if c < S // 2])               # the upper half filled: a twin in the lower rows
        add(a, b, list(rng.choice(rest, 12, replace=False)) + [a, b], list(rng.choice(rest, 6, replace=False)))
        add(a, b, [a, b], [])                                            # nothing else is empty: no twin
        add(a, b, every, every)                                          # every entry there: no twin
    return np.array(pairs, dtype=np.int32), np.array(empty), np.array(bits), own_sets, empty_sets


@pytest.mark.parametrize('BH,BW', BOARDS)
def test_the_twin_and_its_cell_sources_element_by_element(drv, BH, BW):
    S = BH * BW
    pairs, empty, bits, own_sets, empty_sets = _cases(BH, BW)
    ts, src, rng_, consts = drv.run('twin', [BH, BW], [pairs, empty, bits], [np.int32, np.int32, np.int32, np.int32])
    BASE, MEMO, RUN, F_NONE, F_A, F_T, LINE = (int(v) for v in consts)
    src, rng_ = src.reshape(len(pairs), S, 3), rng_.reshape(len(pairs), 3, 2)
    c = np.arange(S)
    cy, cx = c // BW, c % BW

    def cheb(p):
        return np.maximum(np.abs(cy - p // BW), np.abs(cx - p % BW))
    seen = dict(none=0, edge=0, corner=0)
    for i, (a, b) in enumerate(pairs):
        ok = (cheb(a) >= 7) & (cheb(b) >= 7) & np.isin(c, sorted(empty_sets[i])) & ~np.isin(c, sorted(own_sets[i]))
        want_t = int(c[ok][0]) if ok.any() else -1
        assert ts[i] == want_t, (a, b, ts[i], want_t)
        if want_t < 0:
            seen['none'] += 1
            assert (src[i] == -9).all()
            continue
        t = want_t
        ty, tx = divmod(t, BW)
        seen['edge'] += ty in (0, BH - 1) or tx in (0, BW - 1)
        seen['corner'] += t in (0, BW - 1, S - BW, S - 1)
        in_a, in_b, in_t = cheb(a) <= 3, cheb(b) <= 3, cheb(t) <= 3
        assert not (in_a & in_b).any() and not (in_a & in_t).any() and not (in_b & in_t).any()      # three disjoint windows
        assert np.array_equal(src[i, :, 0], np.where(in_a, RUN, np.where(in_b, MEMO, BASE)))
        assert (src[i, in_t, 0] == BASE).all()                                                      # the leaf has no stone at t
        assert np.array_equal(src[i, :, 1], np.where(in_a, F_A, np.where(in_t, F_T, F_NONE)))
        for p, inside in ((a, in_a), (b, in_b), (t, in_t)):
            assert np.array_equal(src[i, inside, 2], ((cy - p // BW + 3) * 7 + cx - p % BW + 3)[inside])
        assert (src[i, ~(in_a | in_b | in_t), 2] == -1).all()
        # what the pass holds from the base around one stone (within 4, a function of the inputs within 2 more) never sees another
        lines = [set(range(lo // LINE, hi // LINE + 1)) for lo, hi in rng_[i]]
        assert not (lines[0] & lines[1]) and not (lines[0] & lines[2]) and not (lines[1] & lines[2])
        assert all(hi - lo + 1 == 49 * 2 * 4 for lo, hi in rng_[i])
    assert seen['none'] > 0 and seen['edge'] > 0 and seen['corner'] > 0, seen
