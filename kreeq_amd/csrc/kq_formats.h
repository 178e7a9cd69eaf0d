// kq_formats.h -- record formats and fan-out limits of the partitioned path: plain constants that the device headers
// (kq_partition.h) and the host-only kernel selector (kq_select_host.h) both read.  No device code, no HIP.
#pragma once
#include <cstdint>
namespace kq {
constexpr int NB_MAX = 2048;                     // bins of one split incl. the discard bin: fan-out <= NB_MAX - 1
constexpr int PART_MAX_K = 28;                   // packed 8-byte records up to here, WIDE above
// Record formats of the partitioned path:
//   FMT_PACK8  (k <= 28)  one u64: top 56 bits of the table hash | two 3-bit edge indices at bits 56..61
//   FMT_WIDE   (any k)    u64 table hash (or raw key, see LevelCfg::in_raw) + lockstep u8 (AUX_IDX6 / AUX_EDGE_BYTE)
//   FMT_NARROW (k <= 21, two-level split with 256 top-bit buckets) u32 + lockstep u8: after P1 the top 8
//              hash bits are the bucket a record lies in, the remaining <= 34 bits are the u32 (upper 32) and the
//              low 2 bits of the u8, whose upper 6 bits are the edge indices.  5 bytes instead of 8 through
//              three of the four record passes, and the level histogram reads only the u32 array.
constexpr int FMT_PACK8 = 0, FMT_WIDE = 1, FMT_NARROW = 2;
constexpr int FMT_PACK8_TO_NARROW = 3;      // k_lv_scatter only: packed records in, narrow records out (bins = hash prefix)
constexpr uint32_t NARROW_CBITS = 8, NARROW_MAX_K = 21;
// FMT_TOP8 (k = 29..32 on a table with hash-prefix buckets): one u64 = the 56 hash bits below the bucket prefix,
// left-aligned, | the two edge indices in the low 6 bits.  Replaces the 9-byte WIDE records on the count and
// lookup paths; split levels and region kernels address it like a narrow record whose u32 is the top half.
constexpr int FMT_TOP8 = 4;
// FMT_TIGHT (k <= 21, tables of >= 2^16 regions; the LAST level's output and the pending sets of the count path only): one
// u32, no lockstep byte.  A record that has reached its region r needs only the hash bits r does not imply:
//   (top 32 hash bits - rstart[r]) << 16 | the 10 hash bits below << 6 | the two edge indices
// (ceil(2^32 / R) <= 2^16 values of the first field).  `>> 6` is the 32-bit key of k_count_regions_q4.  4 bytes instead of
// 5 in the arena, one store per record instead of two in the last level, one load in the table pass.
constexpr int FMT_TIGHT = 5;
constexpr int FMT_NARROW_TO_TIGHT = 6;      // k_lv_scatter only: narrow records in, tight records out (last level)
}  // namespace kq
