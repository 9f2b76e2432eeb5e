"""rz_memo.h's one-window rule on the CPU (tests/host_driver.py: plain and sanitized builds of a stand-alone driver): `served` -- which
windows of a far pair come from the memo: none, a's, b's or both -- and `cell_source` -- base, memo or run, for every cell of the leaf --
are held element by element against a numpy restatement.  Boards of 15 x 15, 11 x 11, 16 x 16 and 11 rows x 16 columns; pairs at
Chebyshev distance exactly 6, 7 and 8 along rows, columns and diagonals and corner to corner, each under all four states of its two
valid bits, and once each at depth 1, depth 3 and against a base that is not the root.  Asserted: `served` is "both" exactly where
`hit` says yes, "none" for every pair that is not far whatever its bits say, and every cell of the leaf has exactly one source."""
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

// half BH BW <pairs: int32 [n][4] = a, b, depth, base_is_root> <bits: uint64 [n][8]> -> <verdicts int32 [n][3] = far, hit, served>
//                                                                       <sources int32 [n][BH * BW][3] = source, window, slot>
//                                                                       <int32 [7] = the constants>
int main(int argc, char **argv) {
    if (argc != 9 || std::string(argv[1]) != "half") return 2;
    const int BH = atoi(argv[2]), BW = atoi(argv[3]);
    const std::vector<int32_t> pairs = slurp<int32_t>(argv[4]);
    const std::vector<uint64_t> bits = slurp<uint64_t>(argv[5]);
    const size_t n = pairs.size() / 4;
    std::vector<int32_t> verdict(n * 3), src(n * BH * BW * 3);
    for (size_t i = 0; i < n; ++i) {
        const int a = pairs[4 * i], b = pairs[4 * i + 1], depth = pairs[4 * i + 2];
        const bool root = pairs[4 * i + 3] != 0;
        const uint64_t *w = bits.data() + i * rzm::kBitmapWords;
        const int srv = rzm::served(depth, root, a, b, BW, w);
        verdict[3 * i] = rzm::far_pair(depth, root, a, b, BW);
        verdict[3 * i + 1] = rzm::hit(depth, root, a, b, BW, w);
        verdict[3 * i + 2] = srv;
        for (int c = 0; c < BH * BW; ++c) {
            int win = -2, slot = -2;
            src[(i * BH * BW + c) * 3] = rzm::cell_source(c / BW, c % BW, a, b, BW, srv, &win, &slot);
            src[(i * BH * BW + c) * 3 + 1] = win;
            src[(i * BH * BW + c) * 3 + 2] = slot;
        }
    }
    dump(argv[6], verdict);
    dump(argv[7], src);
    dump(argv[8], std::vector<int32_t>{rzm::kServeNone, rzm::kServeA, rzm::kServeB, rzm::kServeBoth, rzm::kSrcBase, rzm::kSrcMemo, rzm::kSrcRun});
    return 0;
}
'''

drv = host_driver.fixture('memo_half_driver', DRIVER)

BOARDS = [(15, 15), (11, 11), (16, 16), (11, 16)]   # rows, columns


def _cases(BH, BW):
    S = BH * BW
    centres = {0, BW - 1, S - BW, S - 1, BW // 2, (BH // 2) * BW, (BH // 2) * BW + BW - 1, S - BW // 2 - 1, (BH // 2) * BW + BW // 2, BW + 1}
    centres |= {c for w in (64, 128, 192) for c in (w - 1, w) if c < S}
    rows, bits = [], []

    def add(a, b, depth, root, va, vb):
        rows.append((a, b, depth, root))
        w = np.zeros(8, dtype=np.uint64)
        if va:
            w[0 * 4 + (a >> 6)] |= np.uint64(1) << np.uint64(a & 63)
        if vb:
            w[1 * 4 + (b >> 6)] |= np.uint64(1) << np.uint64(b & 63)
        bits.append(w)

    def every(a, b):
        for va in (0, 1):
            for vb in (0, 1):
                add(a, b, 2, 1, va, vb)
        add(a, b, 1, 1, 1, 1)
        add(a, b, 3, 1, 1, 1)
        add(a, b, 2, 0, 1, 1)
        add(a, b, 2, 0, 1, 0)

    for a in sorted(centres):
        ay, ax = divmod(a, BW)
        for d in (6, 7, 8):
            for sy, sx in ((0, 1), (1, 0), (1, 1), (0, -1), (-1, 0), (-1, -1), (1, -1), (-1, 1), (1, 0.5)):
                by, bx = ay + int(sy * d), ax + int(sx * d)
                if 0 <= by < BH and 0 <= bx < BW:
                    every(a, by * BW + bx)
    for a, b in ((0, S - 1), (S - 1, 0), (BW - 1, S - BW), (S - BW, BW - 1)):   # corner to corner
        every(a, b)
    return np.array(rows, dtype=np.int32), np.array(bits, dtype=np.uint64)


@pytest.mark.parametrize('BH,BW', BOARDS)
def test_served_windows_and_cell_sources_element_by_element(drv, BH, BW):
    pairs, bits = _cases(BH, BW)
    verdict, src, consts = drv.run('half', [BH, BW], [pairs, bits], [np.int32, np.int32, np.int32])
    NONE, A, B_, BOTH, BASE, MEMO, RUN = (int(v) for v in consts)
    assert (NONE, A | B_, A & B_) == (0, BOTH, 0) and len({BASE, MEMO, RUN}) == 3
    verdict, src = verdict.reshape(-1, 3), src.reshape(len(pairs), BH * BW, 3)
    a, b, depth, root = pairs.T
    dist = np.maximum(np.abs(a // BW - b // BW), np.abs(a % BW - b % BW))
    far = (depth == 2) & (root != 0) & (dist >= 7)
    va = ((bits[np.arange(len(a)), a >> 6] >> (a & 63).astype(np.uint64)) & np.uint64(1)) != 0
    vb = ((bits[np.arange(len(b)), 4 + (b >> 6)] >> (b & 63).astype(np.uint64)) & np.uint64(1)) != 0
    want = np.where(far, np.where(va, A, 0) | np.where(vb, B_, 0), NONE)
    assert np.array_equal(verdict[:, 0], far.astype(np.int32))
    assert np.array_equal(verdict[:, 2], want)
    assert np.array_equal(verdict[:, 2] == BOTH, verdict[:, 1] != 0)             # "both" is `hit`, and nothing else is
    assert (verdict[~far, 2] == NONE).all() and (va & vb & ~far).any()            # no far pair: none, whatever the bits say
    at2 = (depth == 2) & (root != 0)
    for d in (6, 7, 8):
        assert (at2 & (dist == d)).any()
    assert (at2 & (dist == max(BH, BW) - 1)).any()                                # corner to corner
    for s in (NONE, A, B_, BOTH):                                                 # all four states among the far pairs, at 7 exactly too
        assert (verdict[far & (dist == 7), 2] == s).any()
    c = np.arange(BH * BW)
    cy, cx = c // BW, c % BW
    for i in range(len(pairs)):
        day, dax, dby, dbx = cy - a[i] // BW, cx - a[i] % BW, cy - b[i] // BW, cx - b[i] % BW
        in_a = (np.abs(day) <= 3) & (np.abs(dax) <= 3)
        in_b = (np.abs(dby) <= 3) & (np.abs(dbx) <= 3) & ~in_a
        srv = int(want[i])
        want_src = np.where(in_a, MEMO if srv & A else RUN, np.where(in_b, MEMO if srv & B_ else RUN, BASE))
        want_win = np.where(in_a, 1, np.where(in_b, 2, 0))
        want_slot = np.where(in_a, (day + 3) * 7 + dax + 3, np.where(in_b, (dby + 3) * 7 + dbx + 3, -1))
        assert np.array_equal(src[i, :, 0], want_src), pairs[i]
        assert np.array_equal(src[i, :, 1], want_win), pairs[i]
        assert np.array_equal(src[i, :, 2], want_slot), pairs[i]
        if far[i]:
            # exactly one source per cell: the two windows are disjoint, each is whole (clipped by the board alone), the rest is the base's
            wa = (np.abs(day) <= 3) & (np.abs(dax) <= 3)
            wb = (np.abs(dby) <= 3) & (np.abs(dbx) <= 3)
            assert not (wa & wb).any()
            for w, bit in ((wa, A), (wb, B_)):
                assert (src[i, w, 0] == (MEMO if srv & bit else RUN)).all()
            assert (src[i, ~(wa | wb), 0] == BASE).all()
            assert (src[i, :, 0] == MEMO).sum() == (wa.sum() if srv & A else 0) + (wb.sum() if srv & B_ else 0)
            # what a one-window pass around the missing stone takes from the base (conv2 records within 4 of it, each a function of
            # the inputs within 2 of its cell) never sees the served stone: distance >= 7 - 4 = 3 > 2
            assert dist[i] - 4 >= 3
        else:
            assert (src[i, :, 0] != MEMO).all()
