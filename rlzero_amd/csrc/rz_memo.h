// rz_memo.h -- the per-move feature memo of k_delta_res<false> (rz_delta.h): plain C++, no HIP include, so that the CPU can test the
// rule and the layout (tests/test_delta_memo_host.py); the kernel and rz_net.hip call these functions.
//
// What is remembered.  Under the reference's selection rule most leaves of a move are root + a + b: a the root mover's stone, b the
// other side's stone and the last move.  A value feature at cell c depends on the input cells within Chebyshev distance 3 of c (three
// 3 x 3 convolutions, 1 x 1 heads).  With distance(a, b) >= 7 no cell has both stones in its field, so every cell of the leaf has
//   - within 3 of a: the feature it has in "root + a as the mover's stone, not the last move"         (kind OWN),
//   - within 3 of b: the feature it has in "root + b as the other side's stone and the last move"    (kind OPP_LAST),
//   - elsewhere:     the parity-0 base's value,
// and the first two do not depend on the other stone: an entry (cell, kind) holds the 7 x 7 window of the two value features around the
// cell, filled by the first far-apart leaf that computes it and laid over the base's planes by every later one (a HIT: no trunk).
// rz_delta.h's invariant -- a cell's accumulator sees its products in a fixed order, whatever tile it sits in -- makes the window's
// values the bits the leaf's own passes would compute.
//
// Layout.  Per game 2 x S entries (S = cells of the net's board), entry kind * S + cell, kEntryBytes = 512 apart: 49 slots
// (dy + 3) * 7 + (dx + 3) of two f32 (392 bytes used; off-board slots are never written or read).  The pitch is a multiple of the
// 128-byte line, so no line holds parts of two entries: an entry's lines are written once per base (its valid bit is clear until then)
// and read only behind that, by the one workgroup that owns the game -- a line can never sit in the CU's L1 from before its entry was
// written, which a denser pitch (392 or 448 bytes) would allow through the neighbouring entry's reads.  Plain loads therefore; the
// price is 23 % of unused memory.  Per game a valid bitmap of 2 kinds x 256 bits (kBitmapWords 64-bit words, kind-major), cleared
// wherever the game's bases are built or invalidated: a memo never outlives the base it patches.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RZM_FN __host__ __device__ inline
#else
#define RZM_FN inline
#endif

namespace rzm {

constexpr int kOwn = 0, kOppLast = 1;             // the kinds
constexpr int kRadius = 3, kSide = 2 * kRadius + 1, kSlots = kSide * kSide;   // the window of a head feature: 7 x 7
constexpr int kFeatures = 2;                      // the value planes (head outputs 4 and 5)
constexpr int kEntryBytes = 512, kLineBytes = 128;
constexpr int kMinDist = 2 * kRadius + 1;         // 7: no cell within kRadius of both
constexpr int kBitmapWords = 2 * 4;               // uint64 words of a game's valid bits: [kind][256 cells]
static_assert(kSlots * kFeatures * 4 <= kEntryBytes && kEntryBytes % kLineBytes == 0, "an entry owns its lines");

// sources of a cell's value features on a hit
constexpr int kFromBase = 0, kFromA = 1, kFromB = 2;

RZM_FN int entries_per_game(int S) { return 2 * S; }
RZM_FN long long game_bytes(int S) { return (long long)entries_per_game(S) * kEntryBytes; }
RZM_FN int entry_index(int kind, int cell, int S) { return kind * S + cell; }
// byte offset of feature f of window slot `slot` inside an entry
RZM_FN int slot_offset(int slot, int f) { return (slot * kFeatures + f) * 4; }
RZM_FN int bit_word(int kind, int cell) { return kind * 4 + (cell >> 6); }

RZM_FN int abs_i(int v) { return v < 0 ? -v : v; }
RZM_FN int cheb(int y0, int x0, int y1, int x1) {
    const int dy = abs_i(y0 - y1), dx = abs_i(x0 - x1);
    return dy > dx ? dy : dx;
}
// the window slot of cell (cy, cx) around the centre (y, x), -1 outside the window
RZM_FN int slot_of(int cy, int cx, int y, int x) {
    const int dy = cy - y, dx = cx - x;
    return abs_i(dy) <= kRadius && abs_i(dx) <= kRadius ? (dy + kRadius) * kSide + dx + kRadius : -1;
}

// A leaf whose path from the root is `depth` cells, a then b (board cells y * BW + x), evaluated against a base that is the parity-0
// base of the root (base_is_root: the header equals the root): can the memo serve or learn it at all?
// (the _yx forms take board coordinates: the kernel divides by the width with its own reciprocal)
RZM_FN bool far_pair_yx(int depth, bool base_is_root, int ay, int ax, int by, int bx) {
    return depth == 2 && base_is_root && cheb(ay, ax, by, bx) >= kMinDist;
}
RZM_FN bool far_pair(int depth, bool base_is_root, int a, int b, int BW) {
    return far_pair_yx(depth, base_is_root, a / BW, a % BW, b / BW, b % BW);
}
RZM_FN bool valid_bit(const uint64_t *bits, int kind, int cell) { return (bits[bit_word(kind, cell)] >> (cell & 63)) & 1ull; }
// the hit rule: a far pair with both entries valid
RZM_FN bool hit(int depth, bool base_is_root, int a, int b, int BW, const uint64_t *bits) {
    return far_pair(depth, base_is_root, a, b, BW) && valid_bit(bits, kOwn, a) && valid_bit(bits, kOppLast, b);
}

// ONE WINDOW.  A far pair with exactly one entry valid runs the missing stone's window alone and takes the other stone's from the memo.
// `served`: the windows of a far pair that come from the memo, a set of kServeA (a's, entry (a, OWN)) and kServeB (b's, entry
// (b, OPP_LAST)): none -- both windows are run (and every leaf that is no far pair) --, one of them, or both, which is `hit`.
// Exactness of the pass around the missing stone, say a (b alike): with cheb(a, b) >= 7 every record the pass takes from the base
// instead of computing it -- conv1's records within 3 of a for conv2, conv2's within 4 of a for conv3 -- lies at distance >= 3 from
// b, and a conv1 / conv2 record depends on the input cells within 1 / 2 of its cell: none of them is b, so the base's record is the
// leaf's record there.  What the pass computes itself (conv1 within 1, conv2 within 2, conv3 and the heads within 3 of a) reads
// inputs within 3 of a, b is not among them either.  The radius-4 sets of the two stones may touch at distance 7 or 8: harmless for
// the same reason, the shared cells' conv2 records are the base's in the leaf too.  b's 7 x 7 of value features is the entry's, by
// the argument at the top; every other cell takes the base's value.  So each cell of the leaf has exactly one source (cell_source).
constexpr int kServeNone = 0, kServeA = 1, kServeB = 2, kServeBoth = kServeA | kServeB;
RZM_FN int served(int depth, bool base_is_root, int a, int b, int BW, const uint64_t *bits) {
    if (!far_pair(depth, base_is_root, a, b, BW)) return kServeNone;
    return (valid_bit(bits, kOwn, a) ? kServeA : 0) | (valid_bit(bits, kOppLast, b) ? kServeB : 0);
}
// the sources of a cell's value features in a leaf that serves the windows `srv`: the base's planes, a memo entry, the leaf's own pass
constexpr int kSrcBase = 0, kSrcMemo = 1, kSrcRun = 2;

// where cell (cy, cx) of a hit's leaf takes its value features from, and the window slot there (far pair: at most one window holds it)
RZM_FN int source_of_yx(int cy, int cx, int ay, int ax, int by, int bx, int *slot) {
    const int sa = slot_of(cy, cx, ay, ax), sb = slot_of(cy, cx, by, bx);
    *slot = sa >= 0 ? sa : sb;
    return sa >= 0 ? kFromA : sb >= 0 ? kFromB : kFromBase;
}
RZM_FN int source_of(int cy, int cx, int a, int b, int BW, int *slot) {
    return source_of_yx(cy, cx, a / BW, a % BW, b / BW, b % BW, slot);
}
// cell (cy, cx) of a far pair's leaf that serves the windows `srv` (served): base, memo (window `*win` = kFromA / kFromB, slot `*slot`) or run
RZM_FN int cell_source_yx(int cy, int cx, int ay, int ax, int by, int bx, int srv, int *win, int *slot) {
    *win = source_of_yx(cy, cx, ay, ax, by, bx, slot);
    if (*win == kFromBase) return kSrcBase;
    return (srv & (*win == kFromA ? kServeA : kServeB)) ? kSrcMemo : kSrcRun;
}
RZM_FN int cell_source(int cy, int cx, int a, int b, int BW, int srv, int *win, int *slot) {
    return cell_source_yx(cy, cx, a / BW, a % BW, b / BW, b % BW, srv, win, slot);
}

// THE TWIN.  A far pair root + a + b that runs a's window alone (b's served, entry (a, OWN) missing) has a second window's budget to
// spare: it also runs the window of t, the LOWEST cell of the board that is empty at the root, has no (t, OWN) entry and lies
// kMinDist or more from a AND from b, on the pseudo-position root + a + b + t (t the root mover's stone, as a is, and not the last
// move), and fills (t, OWN) beside (a, OWN): the leaf root + t + b' that comes later finds its window there.  No such cell: no twin.
// Exactness.  (1) a's window, with t on the board: what the pass computes around a reads inputs within 3 of a, and every record it
// takes from the base -- conv1's within 3, conv2's within 4 of a -- depends on inputs within 6 of a: t, 7 or more away, is none of
// them, as b is not (served, above).  Where the radius-4 sets of a and t touch (distance 7 or 8) a record that is only HELD lies
// more than 2 from both stones: the base's there, in the leaf too.  So a's 7 x 7 is the leaf's, bit for bit.  (2) t's window: the same
// argument with a and t exchanged gives the 7 x 7 of "root + t as the mover's stone, not the last move" -- neither a nor b is within
// 6 of a cell the pass computes or holds for it --, which is the meaning of (t, OWN).  (3) The value row: the LEAF has no stone at t,
// and with a and b 7 or more away its cells within 3 of t have the BASE's features.  The pass has written the pseudo-position's
// there, so the threads within 3 of t store their two values to the entry and then put the base's values back into the value row;
// keeping what the pass wrote would evaluate a position the search never reached.
// The choice of t changes which later leaves are served, never a value: any cell that passes `twin_ok` would do.
// What the kernel calls: twin_ok_yx (ResHook::twin_of: lane L tests cells L, 64 + L, ..., a ballot per word, the lowest set bit), slot_of,
// source_of_yx and entry_index (the fill behind delta_passes).  twin_cell and twin_source_yx below are the HOST's statement of the same
// rule, cell by cell, as cell_source_yx is of the one-window patch: tests/test_delta_twin_host.py holds them to numpy, and
// tests/test_delta_twin.py holds the kernel's counters and trees to that rule on the GPU.
RZM_FN bool twin_ok_yx(int ty, int tx, bool empty, bool has_own, int ay, int ax, int by, int bx) {
    return empty && !has_own && cheb(ty, tx, ay, ax) >= kMinDist && cheb(ty, tx, by, bx) >= kMinDist;
}
// root_empty: 4 words, bit = cell empty at the root (bits past the board's S cells are not looked at) -> t, or -1
RZM_FN int twin_cell(int a, int b, int BW, int S, const uint64_t *root_empty, const uint64_t *bits) {
    for (int t = 0; t < S; ++t)
        if (twin_ok_yx(t / BW, t % BW, (root_empty[t >> 6] >> (t & 63)) & 1ull, valid_bit(bits, kOwn, t), a / BW, a % BW, b / BW, b % BW)) return t;
    return -1;
}
// a twin pass's sources: cell (cy, cx) of the leaf root + a + b, b served, a run, twin t.  -> cell_source's answer, and *fills = the
// entry the cell's two computed values are stored to: kFromA (a's), kFromTwin (t's; the cell then takes the BASE's values) or kFromBase (none)
constexpr int kFromTwin = 3;
RZM_FN int twin_source_yx(int cy, int cx, int ay, int ax, int by, int bx, int ty, int tx, int *fills, int *slot) {
    int win;
    const int src = cell_source_yx(cy, cx, ay, ax, by, bx, kServeB, &win, slot);
    const int st = slot_of(cy, cx, ty, tx);
    *fills = st >= 0 ? kFromTwin : src == kSrcRun ? kFromA : kFromBase;
    *slot = st >= 0 ? st : *slot;
    return st >= 0 ? kSrcBase : src;
}

// KIND D1: THE DEPTH-1 LEAF.  About a quarter of a search's leaves are root + a: a the root mover's stone AND the last move, one changed
// cell against the parity-1 base.  An entry (t, D1) holds the 7 x 7 window of the two value features around t in "root + t as the stone
// of the side that has just moved, and the last move"; a depth-1 leaf root + t whose entry is there takes its window from it and the
// parity-1 base's planes elsewhere (d1_hit): no trunk.  A depth-1 leaf is evaluated once a search, so its OWN window is never stored:
// the entries are filled by TWINS alone.  A depth-1 leaf root + a that runs its pass also runs the window of t = d1_twin_cell: the
// lowest cell ABOVE a that is empty at the root, has no (t, D1) entry and lies kMinDist or more from a -- on the pseudo-position
// root + a + t, t a second stone of the side that has just moved and a second last move -- and fills (t, D1).  Above a: the reference
// visits a node's unvisited children in index order, so the cells below a have been depth-1 leaves already, in this search or, on a kept
// tree, in an earlier one, and will not come again (profiles/microbench/d1_probe.py: without the restriction 94 % of the twins are wasted
// on a kept tree, with it none).
// Layout.  A store of its own beside the far pairs': d1_entries_per_game(S) = S entries a game, entry = cell, the same pitch and slot
// layout, and kD1BitmapWords valid words a game of their own (bit = cell), cleared wherever the far pairs' bits are.  Nothing above
// changes its value or meaning.
// Exactness.  (1) a's window with t on the board: what the pass computes around a reads inputs within 3 of a, and every record it
// takes from the base -- conv1's within 3 of a, conv2's within 4 -- depends on inputs within 6 of a; t, 7 or more away, is none of
// them, so a's 7 x 7 is the leaf's, bit for bit.  (2) t's window on root + a + t is that of root + t: the same argument with a and t
// exchanged -- both are stones of the same side and both are marked as the last move, so the pseudo-position is symmetric in them.
// (3) The leaf has no stone at t: the threads within 3 of t store their two values to the entry and put the parity-1 base's values
// back into the value row.  (4) The colour plane (plane 3) is the same at every cell and follows the LEAF's stone count: the twin's
// stone is not counted, so the plane is that of root + one stone, which is what both root + a and root + t have.
// What the kernel calls: d1_twin_ok_yx (ResHook::d1_twin_of: lane L tests cells L, 64 + L, ..., a ballot per word, the lowest set bit),
// d1_entry_index, d1_game_bytes, slot_of (the fill behind delta_passes) and, for a served leaf, source_of_yx with b = a (the far pair's
// hit branch).  d1_hit, d1_twin_cell and d1_source_yx below are the HOST's statement of the same rule, cell by cell:
// tests/test_delta_d1_host.py holds them to numpy -- that is the specification, not the device's path --, and tests/test_delta_d1.py holds
// the kernel's counters and trees to the rule on the GPU.
constexpr int kD1BitmapWords = 4;                 // uint64 words of a game's D1 valid bits: [256 cells]
RZM_FN int d1_entries_per_game(int S) { return S; }
RZM_FN long long d1_game_bytes(int S) { return (long long)d1_entries_per_game(S) * kEntryBytes; }
RZM_FN int d1_entry_index(int cell) { return cell; }
RZM_FN bool d1_valid_bit(const uint64_t *d1bits, int cell) { return (d1bits[cell >> 6] >> (cell & 63)) & 1ull; }
// the hit rule of a depth-1 leaf root + a: the base is the root's and the entry is there
RZM_FN bool d1_hit(int depth, bool base_is_root, int a, const uint64_t *d1bits) { return depth == 1 && base_is_root && d1_valid_bit(d1bits, a); }
RZM_FN bool d1_twin_ok_yx(int ty, int tx, bool empty, bool has_d1, int ay, int ax) {
    return empty && !has_d1 && (ty > ay || (ty == ay && tx > ax)) && cheb(ty, tx, ay, ax) >= kMinDist;
}
// root_empty as twin_cell takes it -> t, or -1
RZM_FN int d1_twin_cell(int a, int BW, int S, const uint64_t *root_empty, const uint64_t *d1bits) {
    for (int t = 0; t < S; ++t)
        if (d1_twin_ok_yx(t / BW, t % BW, (root_empty[t >> 6] >> (t & 63)) & 1ull, d1_valid_bit(d1bits, t), a / BW, a % BW)) return t;
    return -1;
}
// the sources of a depth-1 leaf root + a, cell (cy, cx).  served: a D1 hit (no pass).  (ty, tx): the twin of a pass that runs, ty < 0:
// none.  -> kSrcMemo (entry (a, D1), slot *slot), kSrcRun (the pass computes it) or kSrcBase (the parity-1 base's planes), and *fills =
// kFromTwin where the cell's two computed values are stored to entry (t, D1), slot *slot, before the base's are put back; else kFromBase
RZM_FN int d1_source_yx(int cy, int cx, int ay, int ax, bool served, int ty, int tx, int *fills, int *slot) {
    const int sa = slot_of(cy, cx, ay, ax), st = ty >= 0 && !served ? slot_of(cy, cx, ty, tx) : -1;
    *fills = st >= 0 ? kFromTwin : kFromBase;
    *slot = st >= 0 ? st : sa;
    return sa >= 0 ? (served ? kSrcMemo : kSrcRun) : kSrcBase;
}

}  // namespace rzm
