"""rz_memo.h's kind D1 on the CPU (tests/host_driver.py: plain and sanitized builds of a stand-alone driver): `d1_twin_cell` -- the
lowest cell ABOVE a that is empty at the root, has no (t, D1) entry and lies 7 or more from a -- and `d1_source_yx` -- where every cell
of a depth-1 leaf takes its value features from, served or run, and which cells store to the twin's entry -- are held element by
element against a numpy restatement on 15 x 15 and 11 rows x 16 columns.  Cases: a in the four corners, on the edges, in the centre and
on either side of every 64-cell word boundary; twins at distance exactly 7 and exactly 8; no candidate (nothing above a, nothing far
enough, every far cell filled or occupied); bits in all four words.  Asserted besides: a's window and the twin's are disjoint; the cells
within 3 of the twin take the BASE's values and store to the twin's entry; a served leaf takes a's 7 x 7 from the entry and fills nothing;
`d1_hit` is depth == 1 and the root's base and the bit; the D1 entries are line-aligned, inside S * 512 bytes, and share no 128-byte line;
and the far pairs' store keeps its size: entries_per_game(S) == 2 S."""
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

// d1 BH BW <a: int32 [n]> <empty: uint64 [n][4]> <d1bits: uint64 [n][4]>
//   -> <t int32 [n]> <a run pass's sources int32 [n][BH * BW][3] = source, fills, slot> <a served leaf's, alike>
//      <hits int32 [n][4] = d1_hit at (depth 1, root's base), (depth 1, another base), (depth 2, root's base), (depth 0, root's base)>
//      <entry byte ranges int32 [n][2][2] = a's, t's (-1 without a twin)> <int32 [10] = the constants>
int main(int argc, char **argv) {
    if (argc != 13 || std::string(argv[1]) != "d1") return 2;
    const int BH = atoi(argv[2]), BW = atoi(argv[3]), S = BH * BW;
    const std::vector<int32_t> as = slurp<int32_t>(argv[4]);
    const std::vector<uint64_t> empty = slurp<uint64_t>(argv[5]), bits = slurp<uint64_t>(argv[6]);
    const size_t n = as.size();
    std::vector<int32_t> ts(n), run(n * S * 3), srv(n * S * 3), hits(n * 4), range(n * 4, -1);
    for (size_t i = 0; i < n; ++i) {
        const int a = as[i];
        const uint64_t *b = bits.data() + i * rzm::kD1BitmapWords;
        const int t = rzm::d1_twin_cell(a, BW, S, empty.data() + 4 * i, b);
        ts[i] = t;
        for (int c = 0; c < S; ++c) {
            int fills = -2, slot = -2;
            run[(i * S + c) * 3] = rzm::d1_source_yx(c / BW, c % BW, a / BW, a % BW, false, t < 0 ? -1 : t / BW, t < 0 ? -1 : t % BW, &fills, &slot);
            run[(i * S + c) * 3 + 1] = fills;
            run[(i * S + c) * 3 + 2] = slot;
            srv[(i * S + c) * 3] = rzm::d1_source_yx(c / BW, c % BW, a / BW, a % BW, true, t < 0 ? -1 : t / BW, t < 0 ? -1 : t % BW, &fills, &slot);
            srv[(i * S + c) * 3 + 1] = fills;
            srv[(i * S + c) * 3 + 2] = slot;
        }
        hits[4 * i] = rzm::d1_hit(1, true, a, b);
        hits[4 * i + 1] = rzm::d1_hit(1, false, a, b);
        hits[4 * i + 2] = rzm::d1_hit(2, true, a, b);
        hits[4 * i + 3] = rzm::d1_hit(0, true, a, b);
        const int e[2] = {rzm::d1_entry_index(a), t < 0 ? -1 : rzm::d1_entry_index(t)};
        for (int k = 0; k < 2; ++k) {
            if (e[k] < 0) continue;
            range[i * 4 + 2 * k] = e[k] * rzm::kEntryBytes + rzm::slot_offset(0, 0);
            range[i * 4 + 2 * k + 1] = e[k] * rzm::kEntryBytes + rzm::slot_offset(rzm::kSlots - 1, rzm::kFeatures - 1) + 3;
        }
    }
    dump(argv[7], ts);
    dump(argv[8], run);
    dump(argv[9], srv);
    dump(argv[10], hits);
    dump(argv[11], range);
    dump(argv[12], std::vector<int32_t>{rzm::kSrcBase, rzm::kSrcMemo, rzm::kSrcRun, rzm::kFromBase, rzm::kFromTwin, rzm::kLineBytes, rzm::kD1BitmapWords,
                                        rzm::d1_entries_per_game(S), (int32_t)rzm::d1_game_bytes(S), rzm::entries_per_game(S)});
    return 0;
}
'''

drv = host_driver.fixture('memo_d1_driver', DRIVER)

BOARDS = [(15, 15), (11, 16)]   # rows, columns


def _words(cells):
    w = np.zeros(4, dtype=np.uint64)
    for c in cells:
        w[c >> 6] |= np.uint64(1) << np.uint64(c & 63)
    return w


def _cheb(a, b, BW):
    return max(abs(a // BW - b // BW), abs(a % BW - b % BW))


def _cases(BH, BW):
    S = BH * BW
    rng = np.random.RandomState(11 * BH + BW)
    every = list(range(S))
    centre = (BH // 2) * BW + BW // 2
    firsts = [0, BW - 1, S - BW, S - 1, BW // 2, centre - BW // 2, centre + BW // 2 - (BW + 1) % 2, S - BW // 2, centre, 63, 64, 127, 128]
    firsts += [c for c in (191, 192) if c < S]
    as_, empty, bits, sets = [], [], [], []

    def add(a, emp, d1):
        as_.append(a)
        empty.append(_words(emp))
        bits.append(_words(d1))
        sets.append((set(emp), set(d1)))

    for a in firsts:
        far = [c for c in every if c > a and _cheb(c, a, BW) >= 7]
        near = [c for c in every if _cheb(c, a, BW) < 7]
        add(a, every, [])                                                   # the empty board: the lowest far cell above a
        add(a, every, [c for c in every if c < S // 2])                     # the upper half filled (words 0 and 1, part of 2)
        add(a, every, [c for c in every if c >= S // 2] + [a])              # the lower half filled (the last words), and a's own bit
        add(a, every, far)                                                  # every far cell above a is filled: no twin
        add(a, near, [])                                                    # nothing far is empty: no twin
        add(a, [c for c in every if c <= a], [])                            # nothing above a is empty: no twin
        for d in (7, 8):                                                    # the only candidates lie at distance exactly d
            ring = [c for c in every if c > a and _cheb(c, a, BW) == d]
            if ring:
                add(a, near + ring, [])
        for corner in (BW - 1, S - BW, S - 1):                              # the only candidate is a corner
            if corner > a and _cheb(corner, a, BW) >= 7:
                add(a, near + [corner], [])
        rest = [c for c in every if c != a]
        add(a, list(rng.choice(rest, 14, replace=False)) + [a], list(rng.choice(rest, 7, replace=False)))
    return np.array(as_, dtype=np.int32), np.array(empty), np.array(bits), sets


@pytest.mark.parametrize('BH,BW', BOARDS)
def test_the_d1_twin_and_the_cell_sources_element_by_element(drv, BH, BW):
    S = BH * BW
    as_, empty, bits, sets = _cases(BH, BW)
    ts, run, srv, hits, rng_, consts = drv.run('d1', [BH, BW], [as_, empty, bits], [np.int32] * 6)
    BASE, MEMO, RUN, F_NONE, F_T, LINE, WORDS, PER_GAME, GAME_BYTES, FAR_PER_GAME = (int(v) for v in consts)
    assert (WORDS, PER_GAME, GAME_BYTES, FAR_PER_GAME) == (4, S, S * 512, 2 * S)
    run, srv = run.reshape(len(as_), S, 3), srv.reshape(len(as_), S, 3)
    hits, rng_ = hits.reshape(len(as_), 4), rng_.reshape(len(as_), 2, 2)
    c = np.arange(S)
    cy, cx = c // BW, c % BW

    def cheb(p):
        return np.maximum(np.abs(cy - p // BW), np.abs(cx - p % BW))
    seen = dict(none=0, corner=0, edge=0, d7=0, d8=0, words=set(), hit=0)
    for i, a in enumerate(as_):
        a = int(a)
        emp, d1 = sets[i]
        ok = (c > a) & (cheb(a) >= 7) & np.isin(c, sorted(emp)) & ~np.isin(c, sorted(d1))
        want_t = int(c[ok][0]) if ok.any() else -1
        assert ts[i] == want_t, (a, ts[i], want_t)
        assert list(hits[i]) == [int(a in d1), 0, 0, 0], (a, hits[i])
        seen['hit'] += a in d1
        in_a = cheb(a) <= 3
        slot_a = (cy - a // BW + 3) * 7 + cx - a % BW + 3
        # a served leaf: a's 7 x 7 from the entry, the base elsewhere, nothing stored -- whatever twin the rule would name
        assert np.array_equal(srv[i, :, 0], np.where(in_a, MEMO, BASE)) and (srv[i, :, 1] == F_NONE).all()
        assert np.array_equal(srv[i, :, 2], np.where(in_a, slot_a, -1))
        assert rng_[i, 0, 0] % LINE == 0 and 0 <= rng_[i, 0, 0] and rng_[i, 0, 1] < GAME_BYTES and rng_[i, 0, 1] - rng_[i, 0, 0] + 1 == 49 * 2 * 4
        if want_t < 0:
            seen['none'] += 1
            assert np.array_equal(run[i, :, 0], np.where(in_a, RUN, BASE)) and (run[i, :, 1] == F_NONE).all()
            assert np.array_equal(run[i, :, 2], np.where(in_a, slot_a, -1))
            assert (rng_[i, 1] == -1).all()
            continue
        t = want_t
        ty, tx = divmod(t, BW)
        seen['corner'] += t in (BW - 1, S - BW, S - 1)
        seen['edge'] += ty in (0, BH - 1) or tx in (0, BW - 1)
        seen['d7'] += _cheb(t, a, BW) == 7
        seen['d8'] += _cheb(t, a, BW) == 8
        seen['words'].add(t >> 6)
        in_t = cheb(t) <= 3
        assert not (in_a & in_t).any()                                                               # two disjoint windows
        assert np.array_equal(run[i, :, 0], np.where(in_a, RUN, BASE))                               # the leaf has no stone at t: the base's
        assert np.array_equal(run[i, :, 1], np.where(in_t, F_T, F_NONE))                             # a's own window is never stored
        slot_t = (cy - ty + 3) * 7 + cx - tx + 3
        assert np.array_equal(run[i, :, 2], np.where(in_t, slot_t, np.where(in_a, slot_a, -1)))
        assert rng_[i, 1, 0] % LINE == 0 and 0 <= rng_[i, 1, 0] and rng_[i, 1, 1] < GAME_BYTES and rng_[i, 1, 1] - rng_[i, 1, 0] + 1 == 49 * 2 * 4
        lines = [set(range(lo // LINE, hi // LINE + 1)) for lo, hi in rng_[i]]
        assert not (lines[0] & lines[1])
    assert seen['none'] > 0 and seen['corner'] > 0 and seen['edge'] > 0 and seen['d7'] > 0 and seen['d8'] > 0 and seen['hit'] > 0, seen
    assert seen['words'] == set(range((S + 63) // 64)), seen                                          # twins in every word of the bits
    # bits in all four words were read: the filled halves above cover words 0 .. 3
    assert all((bits[:, w] != 0).any() for w in range((S + 63) // 64))
