"""rz_memo.h, the rule and the layout of k_delta_res<false>'s feature memo, on the CPU: a stand-alone driver (tests/host_driver.py: plain
and sanitized builds) evaluates every function of the header for lists of (a, b) pairs on boards of 11 x 11, 15 x 15, 16 x 16 and
11 rows x 16 columns, and a numpy restatement of the rule is held against it element by element: the far-pair test at distances 6 (no)
and 7 (yes), the hit rule over the valid bits, every cell's source (the window of a, of b, or the base) and its window slot, the
entries' places in memory (no 128-byte line shared by two entries, every slot inside its entry)."""
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

// pairs BH BW <pairs: int32 [n][4] = a, b, depth, base_is_root> <bits: uint64 [n][8]> -> <verdicts int32 [n][2] = far, hit>
//                                                                                       <sources int32 [n][BH * BW][2] = source, slot>
// layout S -> <int32 [2 S][3] = entry index, first byte, last byte of its slots> <int32 [4] = constants>
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "pairs" && argc == 8) {
        const int BH = atoi(argv[2]), BW = atoi(argv[3]);
        const std::vector<int32_t> pairs = slurp<int32_t>(argv[4]);
        const std::vector<uint64_t> bits = slurp<uint64_t>(argv[5]);
        const size_t n = pairs.size() / 4;
        std::vector<int32_t> verdict(n * 2), src(n * BH * BW * 2);
        for (size_t i = 0; i < n; ++i) {
            const int a = pairs[4 * i], b = pairs[4 * i + 1], depth = pairs[4 * i + 2];
            const bool root = pairs[4 * i + 3] != 0;
            verdict[2 * i] = rzm::far_pair(depth, root, a, b, BW);
            verdict[2 * i + 1] = rzm::hit(depth, root, a, b, BW, bits.data() + i * rzm::kBitmapWords);
            for (int c = 0; c < BH * BW; ++c) {
                int slot = -2;
                src[(i * BH * BW + c) * 2] = rzm::source_of(c / BW, c % BW, a, b, BW, &slot);
                src[(i * BH * BW + c) * 2 + 1] = slot;
            }
        }
        dump(argv[6], verdict);
        dump(argv[7], src);
        return 0;
    }
    if (what == "layout" && argc == 5) {
        const int S = atoi(argv[2]);
        std::vector<int32_t> out;
        for (int kind = 0; kind < 2; ++kind)
            for (int cell = 0; cell < S; ++cell) {
                const int e = rzm::entry_index(kind, cell, S);
                out.push_back(e);
                out.push_back(e * rzm::kEntryBytes + rzm::slot_offset(0, 0));
                out.push_back(e * rzm::kEntryBytes + rzm::slot_offset(rzm::kSlots - 1, rzm::kFeatures - 1) + 3);
            }
        dump(argv[3], out);
        dump(argv[4], std::vector<int32_t>{rzm::kEntryBytes, rzm::kLineBytes, (int32_t)rzm::game_bytes(S), rzm::entries_per_game(S)});
        return 0;
    }
    return 2;
}
'''

drv = host_driver.fixture('memo_driver', DRIVER)

BOARDS = [(11, 11), (15, 15), (16, 16), (11, 16)]   # rows, columns


def _cases(BH, BW):
    """(a, b, depth, base_is_root) and the valid bits of each: a in the corners, on the edges and on both sides of the 64-cell word
    boundaries; b at Chebyshev distance exactly 6 and exactly 7 along rows, columns and diagonals wherever the board has room, and a
    few far corners; each pair at depth 2 against the root's base with all four settings of its two valid bits, and once each at depth
    1, at depth 3 and against a base that is not the root (valid bits set: only the rule says no)."""
    S = BH * BW
    centres = {0, BW - 1, S - BW, S - 1, BW // 2, (BH // 2) * BW, (BH // 2) * BW + BW - 1, S - BW // 2 - 1, (BH // 2) * BW + BW // 2}
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

    for a in sorted(centres):
        ay, ax = divmod(a, BW)
        for d in (6, 7):
            for sy, sx in ((0, 1), (1, 0), (1, 1), (0, -1), (-1, 0), (-1, -1), (1, -1), (-1, 1), (1, 0.5)):
                by, bx = ay + int(sy * d), ax + int(sx * d)
                if 0 <= by < BH and 0 <= bx < BW:
                    b = by * BW + bx
                    for va in (0, 1):
                        for vb in (0, 1):
                            add(a, b, 2, 1, va, vb)
                    add(a, b, 1, 1, 1, 1)
                    add(a, b, 3, 1, 1, 1)
                    add(a, b, 2, 0, 1, 1)
        for b in (0, S - 1):
            add(a, b, 2, 1, 1, 1)
    return np.array(rows, dtype=np.int32), np.array(bits, dtype=np.uint64)


@pytest.mark.parametrize('BH,BW', BOARDS)
def test_rule_and_sources_element_by_element(drv, BH, BW):
    pairs, bits = _cases(BH, BW)
    verdict, src = drv.run('pairs', [BH, BW], [pairs, bits], [np.int32, np.int32])
    verdict, src = verdict.reshape(-1, 2), src.reshape(len(pairs), BH * BW, 2)
    a, b, depth, root = pairs.T
    dist = np.maximum(np.abs(a // BW - b // BW), np.abs(a % BW - b % BW))
    far = (depth == 2) & (root != 0) & (dist >= 7)
    va = (bits[np.arange(len(a)), a >> 6] >> (a & 63).astype(np.uint64)) & np.uint64(1)
    vb = (bits[np.arange(len(b)), 4 + (b >> 6)] >> (b & 63).astype(np.uint64)) & np.uint64(1)
    assert np.array_equal(verdict[:, 0], far.astype(np.int32))
    assert np.array_equal(verdict[:, 1], (far & (va != 0) & (vb != 0)).astype(np.int32))
    at2 = (depth == 2) & (root != 0)
    assert (at2 & (dist == 6)).any() and (at2 & (dist == 7)).any() and not verdict[at2 & (dist == 6), 0].any() and verdict[at2 & (dist == 7), 0].all()
    assert verdict[far, 1].any() and not verdict[far, 1].all()
    # every cell's source: numpy's restatement of the windows
    c = np.arange(BH * BW)
    cy, cx = c // BW, c % BW
    for i in range(len(pairs)):
        day, dax, dby, dbx = cy - a[i] // BW, cx - a[i] % BW, cy - b[i] // BW, cx - b[i] % BW
        in_a = (np.abs(day) <= 3) & (np.abs(dax) <= 3)
        in_b = (np.abs(dby) <= 3) & (np.abs(dbx) <= 3)
        want_src = np.where(in_a, 1, np.where(in_b, 2, 0))
        want_slot = np.where(in_a, (day + 3) * 7 + dax + 3, np.where(in_b, (dby + 3) * 7 + dbx + 3, -1))
        assert np.array_equal(src[i, :, 0], want_src), pairs[i]
        assert np.array_equal(src[i, :, 1], want_slot), pairs[i]
        if far[i]:   # no cell lies in both windows, and a's own slot is the centre
            assert not (in_a & in_b).any()
            assert src[i, a[i], 1] == 24 and src[i, b[i], 1] == 24 and src[i, a[i], 0] == 1 and src[i, b[i], 0] == 2


@pytest.mark.parametrize('BH,BW', BOARDS)
def test_no_line_is_shared_between_entries(drv, BH, BW):
    S = BH * BW
    table, consts = drv.run('layout', [S], [], [np.int32, np.int32])
    table = table.reshape(2 * S, 3)
    pitch, line, game_bytes, n_entries = (int(v) for v in consts)
    assert n_entries == 2 * S and game_bytes == n_entries * pitch and pitch % line == 0
    assert sorted(table[:, 0]) == list(range(2 * S))                      # kind, cell -> a place of its own
    first_line, last_line = table[:, 1] // line, table[:, 2] // line
    owner = {}
    for e, lo, hi in zip(table[:, 0], first_line, last_line):
        for ln in range(lo, hi + 1):
            assert owner.setdefault(ln, e) == e, 'line %d holds parts of two entries' % ln
    assert (table[:, 2] < game_bytes).all() and (table[:, 2] - table[:, 1] + 1 == 49 * 2 * 4).all()
