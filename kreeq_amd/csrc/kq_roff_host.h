// kq_roff_host.h -- geometry of the region-major offset matrix of a table pass (k_p3_region_offsets in kq_kernels.h):
// roff[row][pitch] of uint32_t, one row per allocated region plus the closing one.  Host arithmetic only, no device code,
// so that it can be exercised by a stand-alone program (tests/native/roff_geometry_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace kq {

constexpr uint32_t ROFF_MAX_SETS = 64;           // = P3_MAX_SETS (checked where both are visible)
constexpr uint32_t ROFF_PITCH_STEP = 16;         // columns of one 64-byte line

// columns per row for a pass over n_sets sets: n_sets rounded up to whole 64-byte lines; 0 = no matrix (no sets, or more
// than a pass can hold)
inline uint32_t roff_pitch(uint32_t n_sets) {
    if (n_sets == 0 || n_sets > ROFF_MAX_SETS) return 0;
    return (n_sets + ROFF_PITCH_STEP - 1) / ROFF_PITCH_STEP * ROFF_PITCH_STEP;
}
// rows of the matrix of a table (or table window) of `regions` allocated regions: offsets r and r + 1 bound region r
inline uint64_t roff_rows(uint64_t regions) { return regions + 1; }
// bytes of the buffer that serves every pass over such a table, whatever its number of sets; 0 = not representable
// (regions < 2^32 for every table the library builds: 2^32 x 256 B fits a size_t of 64 bits)
inline size_t roff_bytes(uint64_t regions) {
    if (regions >= (1ull << 32)) return 0;
    return (size_t)(roff_rows(regions) * ROFF_MAX_SETS * sizeof(uint32_t));
}
// element index of roff[row][col] at a given pitch
inline uint64_t roff_index(uint64_t row, uint32_t pitch, uint32_t col) { return row * pitch + col; }

}  // namespace kq
