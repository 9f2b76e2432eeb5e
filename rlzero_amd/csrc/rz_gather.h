// rz_gather.h -- which lane moves which 16 bytes when a leaf's pass -1 copies the base's records into LDS (rz_delta.h, delta_passes<SETS>):
// plain C++, no HIP include, so that the CPU can test the mapping (tests/test_delta_gather_host.py); the kernel calls these functions.
//
// The sets are 256-bit masks of cells as four 64-bit words (rz_window.h), word w = cells 64 w .. 64 w + 63.  With W1 .. W4 the windows
// of radius 1 .. 4 around the changed cells, a pass holds in LDS the conv1 records of W3 and the conv2 records of W4; those inside W1 /
// W2 it computes, the others -- H1 = W3 & ~W1, H2 = W4 & ~W2 -- it copies from the base.  Record j of a held set is its j-th cell in
// ascending cell order; the record's LDS slot is the cell's rank in W3 / W4 (what maps, lists and the convolutions know it by).
//
// Work split.  A conv2 record is 256 bytes = 16 lanes x 16 bytes: one wave-instruction carries four records, a round of the four waves
// sixteen -- round i gives record 16 i + 4 wave + (lane >> 4) to the lane group, lane & 15 is the 16-byte chunk.  A conv1 record is 128
// bytes = 8 lanes: round i gives record 32 i + 8 wave + (lane >> 3), chunk lane & 7.  The budget of a pass (164 conv2 / 128 conv1
// records) bounds the rounds at 11 / 4.  A lane group whose record is past the set's count requests the offset kOutside -- past the end
// of the base's buffer resource: zeros, no memory access -- and stores nothing.
//
// j -> (cell, slot) without a barrier: every wave keeps a table of the records of ITS rounds.  Lane L owns cells L, 64 + L, 128 + L,
// 192 + L; for each one that is held it knows j (the bits below it in H, plus the words before) and the slot (the same from W), and if
// the record falls to its wave it writes the 16-bit entry cell | slot << 8 at the record's place in the wave's table.  The wave then
// reads the entries of its rounds back (one wave's LDS operations complete in order).  76 entries a wave: 11 x 4 conv2, 4 x 8 conv1.
//
// Three waves (Split<3>, the functions' <3> forms; k_delta_res' handed pass): the same split over gathering waves 0 .. 2 -- a round is
// 12 conv2 / 24 conv1 records, 14 / 6 rounds cover the budget, a wave's table has 14 x 4 + 6 x 8 = 104 entries.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RZG_FN __host__ __device__ inline
#else
#define RZG_FN inline
#endif

namespace rzg {

constexpr int kWords = 4;                          // 256 cells
constexpr int kC1Max = 128, kC2Max = 164;          // records of conv1's / conv2's output a pass may hold (rz_delta.h: kC1Slots, kC2Slots)
constexpr int kC1Bytes = 128, kC2Bytes = 256;      // a record in the base
constexpr int kC1Lanes = kC1Bytes / 16, kC2Lanes = kC2Bytes / 16;              // lanes that move one record
constexpr int kC1PerWave = 64 / kC1Lanes, kC2PerWave = 64 / kC2Lanes;          // records of one wave-instruction: 8 / 4
// the split over NW gathering waves (NW = 4: every wave of the workgroup, the names without a parameter below; NW = 3: waves 1 .. 3 of
// the resident search's handed pass, numbered 0 .. 2 here, while wave 0 finishes the selection and runs conv1)
template <int NW>
struct Split {
    static constexpr int kC1PerRound = NW * kC1PerWave, kC2PerRound = NW * kC2PerWave;          // records of a round of the NW waves
    static constexpr int kC1Rounds = (kC1Max + kC1PerRound - 1) / kC1PerRound;                  // 4 waves: 4, 3 waves: 6
    static constexpr int kC2Rounds = (kC2Max + kC2PerRound - 1) / kC2PerRound;                  // 4 waves: 11, 3 waves: 14
    static constexpr int kTabC2 = 0, kTabC1 = kC2Rounds * kC2PerWave;                           // a wave's table: its conv2 entries, then its conv1 entries
    static constexpr int kTabEntries = kTabC1 + kC1Rounds * kC1PerWave;                         // 4 waves: 76, 3 waves: 104
};
constexpr int kC1PerRound = Split<4>::kC1PerRound, kC2PerRound = Split<4>::kC2PerRound;      // ... of a round of the four waves: 32 / 16
constexpr int kC1Rounds = Split<4>::kC1Rounds;                                  // 4
constexpr int kC2Rounds = Split<4>::kC2Rounds;                                  // 11
constexpr int kTabC2 = Split<4>::kTabC2, kTabC1 = Split<4>::kTabC1;            // a wave's table: its conv2 entries, then its conv1 entries
constexpr int kTabEntries = Split<4>::kTabEntries;                              // 76 (152 bytes)
static_assert(kC1Rounds == 4 && kC2Rounds == 11 && kTabEntries == 76, "the four-wave split");
static_assert(Split<3>::kC1Rounds == 6 && Split<3>::kC2Rounds == 14 && Split<3>::kTabEntries == 104, "the three-wave split: 164 / 12 and 128 / 24 rounds");
constexpr int kOutside = 1 << 30;                  // an offset past every buffer's end

RZG_FN int popcount(uint64_t w) { return __builtin_popcountll(w); }

// ---- masks -> held set, count, record j -> cell, cell -> slot
RZG_FN uint64_t held(uint64_t outer, uint64_t inner) { return outer & ~inner; }   // one word of H = W_outer & ~W_inner
RZG_FN int count(const uint64_t (&m)[kWords]) { return popcount(m[0]) + popcount(m[1]) + popcount(m[2]) + popcount(m[3]); }
// set bits of `word` below bit `bit` (0 .. 63)
RZG_FN int below(uint64_t word, int bit) { return popcount(word & ((1ull << bit) - 1ull)); }
// the rank of `cell` in set m: its record number in a held set, its slot in a window (cell need not be a member)
RZG_FN int rank(const uint64_t (&m)[kWords], int cell) {
    int r = 0;
    for (int w = 0; w < kWords; ++w) r += w < (cell >> 6) ? popcount(m[w]) : 0;
    return r + below(m[cell >> 6], cell & 63);
}
// the cell of record j of set m (-1: m has no such record)
RZG_FN int cell_of(const uint64_t (&m)[kWords], int j) {
    for (int w = 0; w < kWords; ++w) {
        uint64_t v = m[w];
        const int c = popcount(v);
        if (j >= c) {
            j -= c;
            continue;
        }
        for (; j > 0; --j) v &= v - 1ull;
        return 64 * w + __builtin_ctzll(v);
    }
    return -1;
}

// ---- (round, wave, lane) -> (record, chunk)
template <int NW = 4> RZG_FN int c2_record(int round, int wave, int lane) { return Split<NW>::kC2PerRound * round + kC2PerWave * wave + (int)((unsigned)lane / kC2Lanes); }
RZG_FN int c2_chunk(int lane) { return (int)((unsigned)lane % kC2Lanes); }
template <int NW = 4> RZG_FN int c1_record(int round, int wave, int lane) { return Split<NW>::kC1PerRound * round + kC1PerWave * wave + (int)((unsigned)lane / kC1Lanes); }
RZG_FN int c1_chunk(int lane) { return (int)((unsigned)lane % kC1Lanes); }
// rounds that hold a record, of a set of n
template <int NW = 4> RZG_FN int c2_rounds(int n) { return (n + Split<NW>::kC2PerRound - 1) / Split<NW>::kC2PerRound; }
template <int NW = 4> RZG_FN int c1_rounds(int n) { return (n + Split<NW>::kC1PerRound - 1) / Split<NW>::kC1PerRound; }

// ---- the waves' tables: the wave a record falls to, its place there (c?_index(c?_record(i, wave, lane)) = first + per-wave i + lane group)
template <int NW = 4> RZG_FN int c2_wave(int j) { return (int)(((unsigned)j / kC2PerWave) % (unsigned)NW); }
template <int NW = 4> RZG_FN int c2_index(int j) { return Split<NW>::kTabC2 + (int)(((unsigned)j / Split<NW>::kC2PerRound) * kC2PerWave + (unsigned)j % kC2PerWave); }
template <int NW = 4> RZG_FN int c1_wave(int j) { return (int)(((unsigned)j / kC1PerWave) % (unsigned)NW); }
template <int NW = 4> RZG_FN int c1_index(int j) { return Split<NW>::kTabC1 + (int)(((unsigned)j / Split<NW>::kC1PerRound) * kC1PerWave + (unsigned)j % kC1PerWave); }
RZG_FN uint16_t entry(int cell, int slot) { return (uint16_t)(cell | slot << 8); }
RZG_FN int entry_cell(uint16_t e) { return e & 255; }
RZG_FN int entry_slot(uint16_t e) { return e >> 8; }
// the table place the owner of a held cell writes (-1: none -- the record falls to another wave or lies past the budget, whose
// leaves take the passes without a base).  j: the cell's record number.
template <int NW = 4> RZG_FN int c2_place(int j, int wave) { return j < kC2Max && c2_wave<NW>(j) == wave ? c2_index<NW>(j) : -1; }
template <int NW = 4> RZG_FN int c1_place(int j, int wave) { return j < kC1Max && c1_wave<NW>(j) == wave ? c1_index<NW>(j) : -1; }

// ---- the 16 bytes a lane moves: from this offset of the base (conv1 records at 0, conv2 records at `base_c2`) ...
RZG_FN int c2_src(bool has, int cell, int chunk, int base_c2) { return has ? base_c2 + cell * kC2Bytes + 16 * chunk : kOutside; }
RZG_FN int c1_src(bool has, int cell, int chunk) { return has ? cell * kC1Bytes + 16 * chunk : kOutside; }
// ... to this byte of the layer's LDS records (`pitch`: bytes from one slot to the next)
RZG_FN int dst(int slot, int chunk, int pitch) { return slot * pitch + 16 * chunk; }
// whether record j exists and is copied: inside the set's count and the budget
RZG_FN bool c2_has(int j, int n) { return j < n && j < kC2Max; }
RZG_FN bool c1_has(int j, int n) { return j < n && j < kC1Max; }

}  // namespace rzg
