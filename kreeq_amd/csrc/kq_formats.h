// kq_formats.h -- table and tile constants, record formats, fan-out limits and the argument structs of the partitioned path:
// plain data that the device headers (kq_device.h, kq_partition.h, kq_kernels.h) and the host-only headers (the kernel
// selector kq_select_host.h, the sizing arithmetic kq_plan_host.h) both read.  No device code, no HIP.
#pragma once
#include <cstdint>
namespace kq {
#ifndef KQ_REGION_SHIFT
#define KQ_REGION_SHIFT 11
#endif
constexpr int REGION_SHIFT = KQ_REGION_SHIFT;
constexpr uint32_t REGION_SLOTS = 1u << REGION_SHIFT;   // 2048 slots x 16 B = 32 KiB in HBM
constexpr int HI_K = 29;                       // k >= HI_K: the hash has more than 56 bits, the region implies its top 8
constexpr int TILE_STARTS = 4032;          // k-mer starts of one tile of the sequence scanner (kq_device.h): 252 lanes x 16 starts; window = 4032 + 16 + 48 bytes
constexpr uint64_t n_tiles_of(uint64_t lead, uint64_t len) { return (lead + len + TILE_STARTS - 1) / TILE_STARTS; }
// k-mer starts a launch may process, in caller positions: lets the host cut a huge batch into
// slices that share the input array (a slice's scan window includes the neighbouring bases)
struct EmitRange { uint64_t lo, hi; };

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

constexpr int MS_THREADS = 256;
constexpr int MS_ITEMS = 16;
constexpr int MS_TILE = MS_THREADS * MS_ITEMS;   // 4096 records per multisplit round
constexpr int SEG_MAX = 65536;                   // segments of one split level (256 hash-prefix buckets x up to 256 sub-buckets)
constexpr uint32_t SUB_BITS_MAX = 8;
constexpr int AUX_IDX6 = 0, AUX_EDGE_BYTE = 1, AUX_TIGHT = 2;    // AUX_TIGHT: FMT_TIGHT sets (no lockstep array at all)
constexpr uint64_t TIGHT_MIN_REGIONS = 1ull << 16;
constexpr int P1_F = 1;                 // hist workgroups per scatter workgroup (the scatter grid is already 6 x the resident workgroups)
constexpr uint32_t P2_UNIT = 4 * MS_TILE;   // records per work unit of a split level (never crosses a segment); 4 rounds: k_lv_scatter 357 us vs 384 us at 8, 401 us at 16, 430 us at 1
constexpr uint32_t SCAN_CHUNK = 16384;      // elements per workgroup of the multi-block exclusive scan

struct PartCfg {
    uint64_t n_regions;   // R
    uint32_t g_shift;     // coarse bucket = region >> g_shift
    uint32_t n_coarse;    // bins of P1: ceil(R / 2^g_shift) < NB_MAX (mode 0) or n_parts (mode 1)
    uint32_t mode;        // 0: bin = coarse bucket of the key's table region; 1: bin = owner part (multi-GPU staging)
    uint32_t map_count;   // mode 1: gfalibs mapCount
    uint32_t map_mask;    // map_count - 1 when it is a power of two, else 0
    uint32_t filt_lo, filt_hi;   // count only k-mers whose map index key % map_count lies in [filt_lo, filt_hi)
    uint32_t raw_out;     // 1: WIDE records carry the raw key (kq_emit_partitioned_dev), else its table hash
    uint32_t narrow;      // 1: bin = top NARROW_CBITS hash bits (n_regions is a multiple of 2^NARROW_CBITS), FMT_NARROW records
    uint32_t owner_sub;   // mode 1: each owner part is cut into 2^owner_sub sub-bins by lane id (a multisplit with a handful of
                          // bins serialises its LDS rank atomics on a few addresses); the parts stay contiguous.  The histogram
                          // and the scatter pass give a k-mer the same lane, hence the same sub-bin
    uint32_t sub_bits;    // narrow: > 0 = a middle level cuts each bucket into 2^sub_bits sub-buckets first (very large tables)
    uint32_t win_lo, win_hi;   // bin mode 6 (FMT_NARROW and FMT_TOP8 alike): the table is a window of the hash-prefix buckets [win_lo, win_hi): k-mers of other buckets are dropped in P1
    uint32_t n_rng;       // k_p1_hist bin mode 5 (KQ_OPT_COUNT_MAP_PASSES): count for all n_rng equal map ranges at once, bin = range * 256 + bucket
};

// One record set of k_count_regions: records sorted by table region (format FMT_*; `aux` = lockstep u8 array or null)
// and base[0..n_regions] = first record of every region.
constexpr int P3_MAX_SETS = 64;
struct P3Set { const uint64_t* recs; const uint8_t* aux; const unsigned long long* base; uint64_t n_max; };

// One level of the record split.  Input records are grouped in n_seg segments (seg_off[0..n_seg]);
// a record of segment b with table region r goes to bin (r >> out_shift) - (b << (seg_shift - out_shift)).
//   flat -> coarse buckets : n_seg = 1, seg_shift = 32 (b == 0), out_shift = g_shift, nb = n_coarse
//   coarse -> regions      : n_seg = n_coarse, seg_shift = g_shift, out_shift = 0, nb = 2^g_shift
// Output group index = b * nb + bin (== the region id at the last level).
struct LevelCfg {
    uint64_t n_regions;
    uint32_t n_seg, nb, seg_shift, out_shift;
    uint32_t in_raw;        // 1: the input records hold raw keys (kq_insert_records): this level mixes them
    uint32_t k;             // k-mer length (width of the table's mix), needed when in_raw
    uint32_t narrow;        // 1: FMT_NARROW records, segment b = hash-prefix bucket b owning regions [b * nb, (b + 1) * nb)
    uint32_t top8;          // 1: one segment of packed records, bin = top NARROW_CBITS hash bits; the scatter writes narrow records
    // narrow levels: segment b = (bucket b >> nr_shift, sub-bucket b & (2^nr_shift - 1)) starts at region
    // bucket * nr_rps + sub * nr_sub; bin = (region - that) / nr_div (nr_inv = ceil(2^32 / nr_div))
    uint32_t nr_shift, nr_rps, nr_sub, nr_div, nr_inv;
    uint32_t nr_mid, nr_fshift, nr_fmask, nr_f24;   // narrow_bin: middle level, 24 - sub_bits, the bits of the position inside a sub-bucket, product fits 32 bits
    // multi-GPU exchange of narrow records (receive side): spb > 1 = the input has spb segments per logical segment (one
    // run per peer rank): input segment s belongs to logical segment s / spb, whose units and output groups they share
    uint32_t spb;
    uint32_t rep_shift;     // rank replication of the multisplit (block_multisplit's rs), set by the host from nb
    const uint32_t* rstart = nullptr; // non-null: this (last, narrow) level writes FMT_TIGHT records relative to rstart[region]
};
}  // namespace kq
