// rz_window.h -- the window table of receptive-field leaf evaluation (rz_delta.h): plain C++, built on the host once per net
// (rz_net_delta_reserve) and read by k_delta_res.
//
// For every cell c = y * cols + x of a rows x cols board (cols <= 16, rows * cols <= 256) and every radius r = 1 .. 4, the 256-bit
// mask of the ON-BOARD cells within Chebyshev distance r of c, as four 64-bit words: t[16 c + 4 (r - 1) + w] holds cells 64 w ..
// 64 w + 63.  Entries of cells c >= rows * cols are zero.  A leaf's cell sets of pass -1 (delta_passes) are unions of these rows: the
// cells within distance th of at least one changed cell -- exactly what cell_dist's minimum over the changed cells gives.
#pragma once
#include <stdint.h>

namespace rzw {

constexpr int kRadii = 4;                                 // radius 1 .. 4: conv1 computes (1), conv2 computes (2), conv3 / conv1 held (3), conv2 held (4)
constexpr int kWords = 4;                                 // 256 cells
constexpr int kEntries = 256 * kRadii * kWords;           // uint64 words of the table (32 KB)

inline void window_table(uint64_t *t, int rows, int cols) {
    for (int i = 0; i < kEntries; ++i) t[i] = 0ull;
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x)
            for (int r = 1; r <= kRadii; ++r) {
                uint64_t *m = t + (size_t)(y * cols + x) * kRadii * kWords + (r - 1) * kWords;
                for (int yy = y - r; yy <= y + r; ++yy)
                    for (int xx = x - r; xx <= x + r; ++xx)
                        if (yy >= 0 && yy < rows && xx >= 0 && xx < cols) {
                            const int c = yy * cols + xx;
                            m[c >> 6] |= 1ull << (c & 63);
                        }
            }
}

}  // namespace rzw
