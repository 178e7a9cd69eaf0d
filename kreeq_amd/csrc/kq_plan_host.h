// kq_plan_host.h -- sizing arithmetic of the count path: how many regions a table gets, which split levels a partition plan has
// and how wide they are, where every array of the partition scratch lies, how large a pending set and the arena are, how a
// batch is sliced and whether a slice is partitioned at all.  Host arithmetic only, from plain values to plain structs: no HIP,
// no handle, no allocation -- kreeq_amd.hip makes the calls these numbers are for, and a stand-alone program
// (tests/native/plan_main.cpp) checks them on the CPU, at sizes no GPU test reaches.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "kq_formats.h"

namespace kq {

// ---- table geometry ---------------------------------------------------------------------------------------------------
// region counts the record formats can address.  NOT idempotent: a result that the sub-bucket rounding lifts past the next
// 256 << sbits boundary would get a wider unit if rounded again (8 403 324 -> 8 421 376 = 257 regions per sub-bucket at
// s = 7; plan_cfg copes: its middle level divides what it can)
inline uint64_t round_regions(uint64_t regions, int k) {
    if (regions < 16) regions = 16;
    // FMT_NARROW / FMT_TOP8 records: 256 hash-prefix buckets of whole regions; k >= HI_K needs it for every table
    // (a slot drops the top 8 hash bits, which its region then implies)
    if (regions >= (uint64_t)NB_MAX || k >= HI_K) regions = (regions + 255) / 256 * 256;
    if (regions >= (1ull << 19)) {                                                  // ... of 2^s sub-buckets of whole regions each, <= 256 regions per sub-bucket
        uint32_t sbits = 3;
        while (sbits < SUB_BITS_MAX && (((regions + 255) / 256) >> sbits) > 256) ++sbits;
        const uint64_t unit = 256ull << sbits;
        regions = (regions + unit - 1) / unit * unit;
    }
    return regions;
}
// kq_create: load <= 0.7 at the hinted number of distinct k-mers
inline uint64_t initial_regions(uint64_t capacity_hint, int k) {
    const uint64_t slots = (uint64_t)((double)(capacity_hint ? capacity_hint : (1u << 20)) / 0.7);
    return round_regions((slots + REGION_SLOTS - 1) >> REGION_SHIFT, k);
}
// growth by rehash: allocated slots and regions double until `need_slots` fit, which keeps every multiple the geometry (and a
// window) has -- a table created below 2048 regions stays off the multiples of 256 (257 -> 2056) and keeps packed records.
// !ok: the region index would overflow
struct GrowTarget { uint64_t slots, regions; bool ok; };
inline GrowTarget grow_target(uint64_t n_slots, uint64_t n_regions, uint64_t need_slots) {
    GrowTarget g{n_slots, n_regions, true};
    while (g.slots < need_slots) { g.slots *= 2; g.regions *= 2; }
    g.ok = g.regions < (1ull << 32);
    return g;
}
// the window [lo, hi) of the 256 hash-prefix buckets on a table of `alloc_now` allocated regions: the geometry is 256 / (hi - lo)
// times larger (`virt` regions), the memory stays what it was (`alloc_new` regions).  !ok: virt does not fit the region index
struct WindowGeom { uint64_t virt, alloc_new; bool ok; };
inline WindowGeom window_geometry(uint64_t alloc_now, uint32_t lo, uint32_t hi, int k) {
    const uint64_t nb = hi - lo;
    WindowGeom g;
    g.virt = round_regions(std::max<uint64_t>((alloc_now + nb - 1) / nb * 256, (uint64_t)NB_MAX), k);
    g.ok = g.virt < (1ull << 32);
    g.alloc_new = lo == 0 && hi == 256 ? g.virt : nb * (g.virt >> 8);
    return g;
}
// slots the main table needs so that `used + extra` k-mers sit at load <= 0.85
inline uint64_t main_need(uint64_t used, uint64_t extra) { return (uint64_t)((double)(used + extra) / 0.85) + REGION_SLOTS; }
// side table: #k-mers with cov >= 255 <= instances / 255, kept at load <= 0.5 up to 2^23 entries (1.2 GB); jobs beyond that
// (hc_follows_fill) get HC_CAP_BIG and, where the fill has been read (`hc_used`), room for its eightfold growth
constexpr uint64_t HC_CAP_BIG = 1ull << 25;      // side-table floor of jobs beyond 2^31 instances (2.7 GB)
constexpr uint64_t HC_UNOBSERVED = ~0ull;
inline bool hc_follows_fill(uint64_t kmers_bound) { return kmers_bound / 255 + 1 > (1ull << 23); }
inline uint64_t hc_need(uint64_t kmers_bound, uint64_t hc_used = HC_UNOBSERVED) {
    const uint64_t bound = kmers_bound / 255 + 1;
    uint64_t need = hc_follows_fill(kmers_bound) ? HC_CAP_BIG : 2 * bound;
    if (hc_used != HC_UNOBSERVED) need = std::max<uint64_t>(need, 8 * hc_used);
    return need;
}

// ---- partition plan ---------------------------------------------------------------------------------------------------
struct TableShape { int k; uint64_t n_regions; int map_count; uint32_t mid_rps; };

inline PartCfg plan_cfg(const TableShape& t, bool allow_narrow = false) {
    PartCfg cfg;
    cfg.n_regions = t.n_regions;
    // fan-outs: the first split (fused with the sequence scan) is insensitive to its fan-out up to
    // ~512 bins, the second is bound by the length of the runs it writes (4096 / fan-out records), so
    // the first level takes as many bins as it can: 256..512 coarse buckets, the rest in level two
    // (measured on configs[1]: 262 x 64 beats the balanced 66 x 256 by 0.2 ms per 130 M records)
    uint32_t g = 1;
    while (((cfg.n_regions + (1ull << g) - 1) >> g) > 512 && g < 10) ++g;
    while (((cfg.n_regions + (1ull << g) - 1) >> g) >= (uint64_t)NB_MAX) ++g;
    cfg.g_shift = cfg.n_regions < (uint64_t)NB_MAX ? 0 : g;
    cfg.n_coarse = (uint32_t)((cfg.n_regions + (1ull << cfg.g_shift) - 1) >> cfg.g_shift);
    cfg.mode = 0; cfg.map_count = (uint32_t)t.map_count;
    cfg.map_mask = (t.map_count & (t.map_count - 1)) == 0 ? (uint32_t)t.map_count - 1 : 0;
    cfg.filt_lo = 0; cfg.filt_hi = (uint32_t)t.map_count;
    cfg.raw_out = 0;
    // 5-byte records (FMT_NARROW): first split on the top 8 hash bits, which needs every bucket to own a
    // whole number of regions (kq_create rounds tables of >= 2048 regions to a multiple of 256; doubling keeps it)
    cfg.narrow = 0; cfg.sub_bits = 0; cfg.owner_sub = 0; cfg.n_rng = 0; cfg.win_lo = 0; cfg.win_hi = 1u << NARROW_CBITS;
    if (allow_narrow && (t.k <= (int)NARROW_MAX_K || t.k > PART_MAX_K) && cfg.n_regions >= (uint64_t)NB_MAX && cfg.n_regions % (1u << NARROW_CBITS) == 0) {
        const uint64_t rps = cfg.n_regions >> NARROW_CBITS;
        // one level bucket -> regions while a bucket has < mid_rps regions (the multisplit writes runs of 4096 / fan-out
        // records, so the last fan-out should stay near 256), else a middle level of 2^sb sub-buckets (sb <= 8): covers
        // every table that fits the HBM.  kq_create rounds the region count so that sb reaches its target
        uint32_t sb = 0;
        if (rps >= t.mid_rps) {
            const uint64_t target_nb = std::max<uint64_t>(1, std::min<uint64_t>(256, t.mid_rps / 8));
            while ((rps >> sb) > target_nb && sb < SUB_BITS_MAX && rps % (2ull << sb) == 0) ++sb;
        }
        if ((rps >> sb) < (uint64_t)NB_MAX && (sb > 0 || rps < (uint64_t)NB_MAX)) { cfg.narrow = 1; cfg.sub_bits = sb; }
    }
    if (cfg.narrow) { cfg.n_coarse = 1u << NARROW_CBITS; if (cfg.g_shift == 0) cfg.g_shift = 1; }
    return cfg;
}
// can the record split reach every region of this table?  (5-byte records: up to 256 x 8 x 2047 regions, i.e.
// any table that fits the HBM; 8-byte / wide records: two fan-outs below NB_MAX)
inline bool part_table_ok(const TableShape& t, bool narrow_possible) {
    if (t.n_regions <= (1ull << 20)) return true;
    if (!narrow_possible) return false;
    return plan_cfg(t, true).narrow != 0;
}
// record format between the stages of a plan; a scanned sequence (count, region-wise lookup): 5-byte records up to k = 21 and
// 8-byte hash-remainder records above k = 28 (tables with hash-prefix buckets), 8-byte packed records up to k = 28, hash + edge
// byte otherwise
inline int plan_fmt(const PartCfg& cfg, int k) { return !cfg.narrow ? FMT_PACK8 : k > PART_MAX_K ? FMT_TOP8 : FMT_NARROW; }
inline int sequence_fmt(int fmt, int k) { return k > PART_MAX_K && fmt != FMT_TOP8 ? FMT_WIDE : fmt; }
// FMT_TIGHT output of the last split level (count path only: the lookup kernels read 5-byte records)
inline bool tight_ok(int fmt, uint64_t n_regions, bool has_region_starts) { return fmt == FMT_NARROW && n_regions >= TIGHT_MIN_REGIONS && has_region_starts; }

// the numbers of a plan for at most n_max records (rounded up to a multiple of 8: slack for vector loads); n_tiles = 0 when the
// input is records; min_segs: segments / output groups an exchange level needs beyond the table's own
struct PlanSizes {
    PartCfg cfg;              // P1 (bases -> coarse buckets)
    bool two_level;
    int fmt;                  // record format between the stages (FMT_*); the caller switches to FMT_WIDE where it applies
    uint64_t n_max, R;
    uint32_t g1;              // P1 scatter workgroups
    uint64_t m1_n, m2_n, sums_n, groups_n;
    uint64_t seg_max;         // segments of the widest level
    uint64_t rec_words, aux_words;   // 8-byte words of one record array and of its lockstep bytes
    bool split2;              // the second record array lives in a buffer of its own
};
inline PlanSizes plan_sizes(const TableShape& t, int n_cu, uint64_t n_max, uint64_t n_tiles, uint32_t p1_bins, bool allow_narrow, uint64_t min_segs) {
    PlanSizes p;
    p.cfg = plan_cfg(t, allow_narrow);
    n_max = (n_max + 7) & ~7ull;
    p.two_level = p.cfg.g_shift != 0;
    p.fmt = plan_fmt(p.cfg, t.k);
    p.n_max = n_max; p.R = p.cfg.n_regions;
    // scatter workgroups: six times what is resident (3 or 2 per CU), each with its own cursor column: the hardware
    // dispatcher balances them (a grid of exactly the resident count ran 8 % longer: k_p1_scatter 577 -> 531 us)
    p.g1 = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_tiles, (uint64_t)n_cu * (p1_bins < 512 ? 18 : 12)));
    p.m1_n = (uint64_t)p1_bins * p.g1 * P1_F;
    const uint64_t nb_max = std::max<uint64_t>(std::max<uint64_t>(1ull << p.cfg.g_shift, p.cfg.n_coarse), p.cfg.narrow ? (p.cfg.n_regions >> NARROW_CBITS) >> p.cfg.sub_bits : 0);
    p.seg_max = std::max<uint64_t>(min_segs, p.cfg.narrow ? ((uint64_t)1 << NARROW_CBITS) << p.cfg.sub_bits : (uint64_t)NB_MAX);
    p.m2_n = (n_max / P2_UNIT + p.seg_max + 2) * nb_max;         // u32 entries, enough for either level
    p.groups_n = std::max<uint64_t>(std::max<uint64_t>(p.R, (uint64_t)p.cfg.n_coarse << p.cfg.g_shift), min_segs) + 2;
    p.sums_n = std::max(p.m1_n, p.groups_n) / SCAN_CHUNK + 2;
    p.aux_words = (n_max + 7) / 8 + 1;
    p.rec_words = p.fmt == FMT_NARROW ? n_max / 2 + 2 : n_max;          // narrow records: u32 + lockstep byte
    // the second record array of a large plan lives in a physically scrambled buffer of its own
    p.split2 = (p.rec_words + p.aux_words) * 8 >= ((size_t)512 << 20);
    return p;
}
// Where every array of a plan lies: offsets in 8-byte words from the start of the scratch -- of recs2 / aux2 from the start of
// the second buffer when split2 (`part2_bytes` of it, else 0) -- and `words`, the size of the scratch.  One cursor walks the
// list, so the size is where it ends.  Every array starts on an 8-byte word; the lockstep arrays are (n_max + 7) / 8 + 1 words,
// so what follows them -- recs2 in the scratch -- starts on a 16-byte boundary only for odd n_max / 8
struct PlanLayout { uint64_t recs1, aux1, recs2, aux2, m1, seg_off, unit_base, group_base, sums, total, hot, m2, words; size_t part2_bytes; };
inline PlanLayout plan_layout(const PlanSizes& p) {
    uint64_t here = 0, there = 0;
    auto take = [](uint64_t& cursor, uint64_t n_words) { const uint64_t at = cursor; cursor += n_words; return at; };
    PlanLayout l;
    l.recs1 = take(here, p.rec_words);
    l.aux1 = take(here, p.aux_words);
    uint64_t& second = p.split2 ? there : here;
    l.recs2 = take(second, p.rec_words);
    l.aux2 = take(second, p.aux_words);
    l.m1 = take(here, p.m1_n);
    l.seg_off = take(here, p.seg_max + 2);
    l.unit_base = take(here, p.seg_max + 2);
    l.group_base = take(here, p.groups_n);
    l.sums = take(here, p.sums_n);
    l.total = take(here, 4);
    l.hot = take(here, p.R + 2);
    l.m2 = take(here, (p.m2_n + 1) / 2);          // u32 entries
    l.words = here;
    l.part2_bytes = (size_t)there * 8;
    return l;
}

// ---- split levels -----------------------------------------------------------------------------------------------------
// rank replication of a level's bin counters: as many counters per bin as fit 512 (at most 64, one per lane)
inline LevelCfg with_rep_shift(const LevelCfg& lv) {
    LevelCfg lvr = lv;
    lvr.rep_shift = 0;
    while (lvr.rep_shift < 6 && (((uint64_t)lv.nb + 1) << (lvr.rep_shift + 1)) <= 512) ++lvr.rep_shift;
    return lvr;
}
inline LevelCfg level_coarse_to_regions(const PartCfg& cfg) {
    LevelCfg lv; lv.n_regions = cfg.n_regions; lv.n_seg = cfg.n_coarse; lv.nb = 1u << cfg.g_shift; lv.seg_shift = cfg.g_shift; lv.out_shift = 0; lv.in_raw = 0; lv.k = 0; lv.narrow = 0; lv.top8 = 0;
    lv.nr_shift = lv.nr_rps = lv.nr_sub = lv.nr_inv = 0; lv.nr_div = 1;
    lv.nr_mid = 0; lv.nr_fshift = 24; lv.nr_fmask = 0xFFFFFFu; lv.nr_f24 = 0;
    lv.spb = 1;
    return lv;
}
// FMT_NARROW: 256 top-bit buckets -> their regions (bucket b owns regions [b * nb, (b + 1) * nb))
// `sub_bits` > 0: a middle level first cuts every bucket into 2^sub_bits sub-buckets (tables of more than
// 2048 regions per bucket: the last level then has 256 << sub_bits segments of rps >> sub_bits regions)
inline LevelCfg level_narrow(const PartCfg& cfg, uint32_t sub_bits = 0, bool middle = false, bool top8_records = false) {
    LevelCfg lv; lv.n_regions = cfg.n_regions;
    const uint32_t rps = (uint32_t)(cfg.n_regions >> NARROW_CBITS), subsz = rps >> sub_bits;
    lv.seg_shift = 0; lv.out_shift = 0; lv.in_raw = 0; lv.k = 0; lv.narrow = top8_records ? 2 : 1; lv.top8 = 0;
    lv.nr_rps = rps; lv.nr_sub = subsz;
    if (middle) { lv.n_seg = 1u << NARROW_CBITS; lv.nb = 1u << sub_bits; lv.nr_shift = 0; lv.nr_div = subsz; }
    else        { lv.n_seg = (1u << NARROW_CBITS) << sub_bits; lv.nb = subsz; lv.nr_shift = sub_bits; lv.nr_div = 1; }
    lv.nr_inv = lv.nr_div > 1 ? (uint32_t)(((1ull << 32) + lv.nr_div - 1) / lv.nr_div) : 0;
    lv.nr_mid = middle ? 1u : 0u; lv.nr_fshift = 24 - sub_bits; lv.nr_fmask = (1u << (24 - sub_bits)) - 1u;
    lv.nr_f24 = ((uint64_t)subsz << (24 - sub_bits)) <= (1ull << 32) && subsz < (1u << 24) ? 1u : 0u;
    lv.spb = 1;
    return lv;
}
inline LevelCfg level_flat_to_coarse(const PartCfg& cfg) {
    LevelCfg lv; lv.n_regions = cfg.n_regions; lv.n_seg = 1; lv.nb = cfg.n_coarse; lv.seg_shift = 32; lv.out_shift = cfg.g_shift; lv.in_raw = 0; lv.k = 0; lv.narrow = 0; lv.top8 = 0;
    lv.nr_shift = lv.nr_rps = lv.nr_sub = lv.nr_inv = 0; lv.nr_div = 1;
    lv.nr_mid = 0; lv.nr_fshift = 24; lv.nr_fmask = 0xFFFFFFu; lv.nr_f24 = 0;
    lv.spb = 1;
    return lv;
}

// ---- pending sets and their arena -------------------------------------------------------------------------------------
// layout of one pending set of at most n_max records: the records, their lockstep bytes (formats that have them), R + 2 region offsets
struct SetLayout { bool has_aux; size_t aux_off /*= the record bytes*/, base_off, total; };
inline SetLayout set_bytes(uint64_t n_max, int fmt, uint64_t R) {
    const size_t rec = (fmt == FMT_NARROW || fmt == FMT_TIGHT) ? 4 : 8;
    SetLayout l;
    l.has_aux = fmt == FMT_NARROW || fmt == FMT_WIDE;
    l.aux_off = ((size_t)n_max * rec + 63) & ~(size_t)63;
    l.base_off = l.aux_off + (l.has_aux ? ((size_t)n_max + 63) & ~(size_t)63 : 0);
    l.total = (l.base_off + (size_t)(R + 2) * 8 + 255) & ~(size_t)255;
    return l;
}
// The arena starts at a few sets and doubles every time it fills up, up to a few times the table and what is free less
// a reserve (a fixed KQ_OPT_PENDING_BYTES is taken as it is): a short job never pays for allocating tens of GB (hipMalloc
// costs milliseconds per GB), a long one gets there within its first batches.
// arena_want: the size the arena should have for one more set of `need` bytes (pend_budget: KQ_OPT_PENDING_BYTES, never 0
// here; was_full: a pass was just run because the set did not fit); only a value above arena_bytes makes the caller ask the
// device for its free memory and call arena_budget: bytes to allocate, 0 = keep the arena, ARENA_STAY = no room, the set
// stays in the plan's scratch
inline size_t arena_want(size_t need, size_t arena_bytes, bool was_full, int64_t pend_budget) {
    if (need > arena_bytes) return pend_budget > 0 ? (size_t)pend_budget : std::max<size_t>(4 * need, (size_t)64 << 20);
    return was_full && pend_budget < 0 ? 2 * arena_bytes : arena_bytes;
}
constexpr size_t ARENA_STAY = ~(size_t)0;
inline size_t arena_budget(size_t want, size_t need, size_t arena_bytes, int64_t pend_budget, size_t free_b, size_t total_b, size_t table_bytes) {
    size_t budget = want;
    // ceiling: what is free now (the partition scratch of this slice size is allocated already) less a reserve of 1/8 of
    // the device for whatever comes later (side-table growth, lookup / export buffers); half of it when that is tight
    const size_t avail = free_b + arena_bytes, reserve = std::max<size_t>(total_b / 8, (size_t)8 << 30);
    const size_t ceiling = avail > 2 * reserve ? avail - reserve : avail / 2;
    if (pend_budget < 0) budget = std::min<size_t>(want, std::min<size_t>(ceiling, std::max<size_t>(4 * need, 4 * table_bytes)));
    if (budget <= arena_bytes && need <= arena_bytes) return 0;         // at its ceiling already
    return budget < need ? ARENA_STAY : budget;
}

// ---- slices of a resident sequence ------------------------------------------------------------------------------------
// aligned view of a device byte string: 16-byte aligned base + lead
inline void aligned_view(const char* d, const uint8_t** ab, uint64_t* lead) {
    uintptr_t p = (uintptr_t)d;
    *lead = p & 15;
    *ab = (const uint8_t*)(p - *lead);
}
// the k-mer starts [a, b) of a resident sequence as a scan of their own: one extra base on the left and k on the right, so
// k-mers and edges across a cut are seen exactly once.  ASCII bytes (d_inv == nullptr) or the packed form, whose words hold
// 16 bases
struct SliceView { const uint8_t* ab; const uint16_t* pinv; uint64_t lead, len; EmitRange er; };
inline SliceView slice_view(const char* d_bases, const uint16_t* d_inv, uint64_t len, int k, uint64_t a, uint64_t b) {
    const uint64_t sub_off = a ? a - 1 : 0;
    SliceView v;
    v.len = std::min(len, b + k) - sub_off;
    v.er = EmitRange{a - sub_off, b - sub_off};
    v.pinv = nullptr;
    if (d_inv) { v.ab = (const uint8_t*)(reinterpret_cast<const uint32_t*>(d_bases) + sub_off / 16); v.pinv = d_inv + sub_off / 16; v.lead = sub_off % 16; }
    else aligned_view(d_bases + sub_off, &v.ab, &v.lead);
    return v;
}
// A resident batch of any size is processed in slices of <= slice_kmers (2^28) k-mer starts: the partition scratch is 16 B
// per start.  Unless the caller fixed the size (slice_user):
//  with pending sets -- large tables split records over up to 65536 segments before the last level: slices of up to 2^31
//    starts keep a few work units per segment and the number of pending sets per table pass low (one slice instead of two per
//    1.3e9-k-mer batch: table pass -3 %, step -1.8 % at 1000 Mbp); 10 B of scratch per start for the default k, so only as
//    far as a quarter of the free HBM pays for it;
//  without (pend_budget == 0) the partitioned path streams the whole table once per slice, so a slice should bring a few
//    records per slot: with a large table (and memory to spare for 16 B of scratch per start) slices grow up to 2^31 starts.
// slice_at_cap: equal slices of at most `cap` starts; slice_reads_free: choose_slice will look at free_b (the caller asks the
// device only then; have_mem_info = the answer came); work_bytes: the scratch held already
inline uint64_t slice_at_cap(uint64_t kmers, uint64_t slice_kmers, uint64_t n_slots, uint64_t cap) {
    const uint64_t slice = std::min<uint64_t>(cap, std::max<uint64_t>(slice_kmers, n_slots / 4));
    const uint64_t n_slices = (kmers + slice - 1) / slice;
    return (kmers + n_slices - 1) / n_slices;
}
inline bool slice_reads_free(uint64_t kmers, uint64_t slice_kmers, bool slice_user, int64_t pend_budget, uint64_t n_slots) {
    if (slice_user || kmers <= slice_kmers) return false;
    return pend_budget != 0 ? slice_at_cap(kmers, slice_kmers, n_slots, 1ull << 31) > (1ull << 30) : 2 * n_slots > slice_kmers;
}
inline uint64_t choose_slice(uint64_t kmers, uint64_t slice_kmers, bool slice_user, int64_t pend_budget, uint64_t n_slots, size_t free_b, size_t work_bytes, bool have_mem_info) {
    if (slice_user || kmers <= slice_kmers) return slice_kmers;
    if (pend_budget != 0) {
        const uint64_t large = slice_at_cap(kmers, slice_kmers, n_slots, 1ull << 31);
        if (large <= (1ull << 30) || (have_mem_info && free_b + work_bytes >= (size_t)11 * large + ((size_t)2 << 30))) return large;   // the plan takes ~10.2 B per start
        return slice_at_cap(kmers, slice_kmers, n_slots, 1ull << 30);
    }
    if (2 * n_slots <= slice_kmers || !have_mem_info) return slice_kmers;
    const uint64_t by_mem = (uint64_t)((free_b + work_bytes) / 24);          // 16 B scratch + margin per start
    return std::max(slice_kmers, std::min<uint64_t>(std::min<uint64_t>(2 * n_slots, 1ull << 31), by_mem));
}
// consecutive slices of one call on two streams with a scratch set each (count_seq_dev).  Not in a map-range or window pass
// (`whole_table` false) unless KQ_OPT_OVERLAP = 2: its slices read their record count back, and measured at full size the
// kernels of two such slices only time-slice the GPU
inline bool slices_fork(int overlap, bool profile, int count_path, uint64_t kmers, uint64_t slice, bool whole_table) {
    return overlap && !profile && count_path != 1 && (kmers + slice - 1) / slice >= 2 && slice >= (1u << 20) && (overlap == 2 || whole_table);
}
// a table pass streams the whole table (2 x 16 B per slot) on top of ~37 B per record; the atomic path costs
// ~95 ps per record whatever the table size (~480 B at the part's streaming rate): partition a slice of n starts unless the
// table is more than ~200 B per record the pass will apply -- this slice, plus what is pending already, times the
// slices of this size the arena can still take (at most 8: the caller may read the table any time)
inline bool slice_partitions(uint64_t n, bool table_ok, uint64_t table_bytes, uint64_t n_regions, int64_t pend_budget, uint64_t pend_records, bool have_arena, size_t arena_bytes) {
    double pass_records = (double)n;
    if (pend_budget != 0) {
        const double per_set = (double)set_bytes(n, FMT_PACK8, n_regions).total;
        const double room = have_arena ? (double)arena_bytes : 4.0 * (double)table_bytes;
        pass_records = (double)pend_records + (double)n * std::max(1.0, std::min(8.0, room / per_set));
    }
    return n >= (1u << 20) && table_ok && (double)table_bytes <= 200.0 * pass_records;
}
// region-wise lookup (lookup_path: KQ_OPT_LOOKUP_PATH): counters only, a sequence worth partitioning, and a table small enough
// next to it (the partitioned path streams the whole table once per slice)
inline bool lookup_partitions(bool per_base, int lookup_path, bool table_ok, uint64_t kmers, uint64_t slice_kmers, uint64_t table_bytes) {
    return !per_base && lookup_path != 1 && table_ok &&
           (lookup_path == 2 || (kmers >= (1u << 20) && (double)table_bytes <= 64.0 * (double)std::min<uint64_t>(kmers, slice_kmers)));
}

// ---- owner parts (multi-GPU staging) ----------------------------------------------------------------------------------
// first bucket of part p of n_parts: the parts are contiguous ranges of the 256 hash-prefix buckets (kreeq_amd/dist.py: bucket_range)
inline uint32_t part_first_bucket(int p, int n_parts) { return (uint32_t)(((uint64_t)p * 256 + n_parts - 1) / n_parts); }
// owner split: up to 256 bins in all, owner part x 2^owner_sub_bits sub-bins by lane (the order inside a part is unspecified anyway)
inline uint32_t owner_sub_bits(int n_parts) {
    uint32_t sb = 0;
    while (((uint32_t)n_parts << (sb + 1)) <= 256u && sb < 5) ++sb;
    return sb;
}

}  // namespace kq
