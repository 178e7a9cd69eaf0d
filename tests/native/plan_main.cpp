// Stand-alone check of the count path's sizing arithmetic (kreeq_amd/csrc/kq_plan_host.h), meant to be built with
// -fsanitize=address,undefined.  (a) a table written out by hand from the arithmetic as it stood inside kreeq_amd.hip: the
// geometries of tools/bench_extra/selection_trace.py, the headline table, the two oddities of round_regions and of growth,
// windows, pending sets, one scratch layout in full, slices, and a row on each side of every threshold of the slice, arena and
// path rules.  (b) what the kernels rely on, over a sweep of region requests around every power of two up to 2^24 regions
// (a 512 GiB table: above the HBM; bucketed plans stop existing only at 2^27 regions, where rps >> 8 reaches NB_MAX).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kq_plan_host.h"

using namespace kq;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad < 50) fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++bad; } } while (0)

constexpr uint64_t KiB = 1ull << 10, MiB = 1ull << 20, GiB = 1ull << 30;
static TableShape shape(int k, uint64_t regions, uint32_t mid_rps = 2048) { return TableShape{k, regions, 128, mid_rps}; }

// ---- (a) the hand-written table ---------------------------------------------------------------------------------------
static void geometry_table() {
    // capacity hint -> regions: load 0.7, whole regions, a multiple of 256 from 2048 regions and for k >= 29
    struct { uint64_t hint, regions_lo_k, regions_hi_k; } tables[] = {{400000, 280, 512}, {1430000, 998, 1024}, {2935000, 2048, 2048}, {93585409, 65536, 65536}, {0, 732, 768}};
    for (auto& t : tables) {
        for (int k : {15, 21, 25}) CHECK(initial_regions(t.hint, k) == t.regions_lo_k);
        for (int k : {30, 31}) CHECK(initial_regions(t.hint, k) == t.regions_hi_k);
    }
    // the plans of those tables: {regions, k class, KQ_OPT_NARROW_MID} -> {narrow, sub_bits, g_shift, n_coarse}.  k = 25 never
    // takes 5-byte records; below 2048 regions nothing does: the bins are the regions themselves (g_shift 0)
    struct { uint64_t R; bool bucket_k; uint32_t mid; uint32_t narrow, sub_bits, g_shift, n_coarse; } plans[] = {
        {280, true, 2048, 0, 0, 0, 280},   {280, false, 2048, 0, 0, 0, 280},   {280, true, 2, 0, 0, 0, 280},
        {512, true, 2048, 0, 0, 0, 512},   {512, true, 16, 0, 0, 0, 512},
        {998, true, 2048, 0, 0, 0, 998},   {998, false, 2, 0, 0, 0, 998},      {1024, true, 2048, 0, 0, 0, 1024},
        {2048, true, 2048, 1, 0, 2, 256},  {2048, true, 2, 1, 3, 2, 256},      {2048, true, 16, 1, 0, 2, 256},
        {2048, false, 2048, 0, 0, 2, 512}, {2048, false, 2, 0, 0, 2, 512},
        {65536, true, 2048, 1, 0, 7, 256}, {65536, true, 2, 1, 8, 7, 256},     {65536, true, 16, 1, 7, 7, 256},
        {65536, false, 2048, 0, 0, 7, 512}, {65536, false, 16, 0, 0, 7, 512}};
    for (auto& p : plans)
        for (int k : {15, 21, 25, 30, 31}) {
            if ((k != 25) != p.bucket_k) continue;
            if (k >= HI_K && (p.R == 280 || p.R == 998)) continue;        // (k >= 29 tables have 512 / 1024 regions at these hints)
            const PartCfg c = plan_cfg(shape(k, p.R, p.mid), true);
            CHECK(c.n_regions == p.R && c.narrow == p.narrow && c.sub_bits == p.sub_bits && c.g_shift == p.g_shift && c.n_coarse == p.n_coarse);
            CHECK(c.mode == 0 && c.map_count == 128 && c.map_mask == 127 && c.filt_lo == 0 && c.filt_hi == 128 && c.raw_out == 0 && c.owner_sub == 0 && c.n_rng == 0 && c.win_lo == 0 && c.win_hi == 256);
            CHECK(plan_fmt(c, k) == (!p.narrow ? FMT_PACK8 : k >= HI_K ? FMT_TOP8 : FMT_NARROW));
            CHECK(part_table_ok(shape(k, p.R, p.mid), true) && part_table_ok(shape(k, p.R, p.mid), false));
            // without allow_narrow (the record entry points, the direct kernel's filter): the coarse plan at any k
            const PartCfg w = plan_cfg(shape(k, p.R, p.mid));
            CHECK(w.narrow == 0 && w.sub_bits == 0 && w.g_shift == (p.R < 2048 ? 0u : p.g_shift) && w.n_coarse == (p.R < 2048 ? p.R : 512));
        }
    CHECK(plan_cfg(TableShape{21, 2048, 100, 2048}, true).map_mask == 0 && plan_cfg(TableShape{21, 2048, 100, 2048}, true).filt_hi == 100);
    CHECK(sequence_fmt(FMT_PACK8, 25) == FMT_PACK8 && sequence_fmt(FMT_PACK8, 28) == FMT_PACK8 && sequence_fmt(FMT_PACK8, 29) == FMT_WIDE && sequence_fmt(FMT_TOP8, 31) == FMT_TOP8 && sequence_fmt(FMT_NARROW, 21) == FMT_NARROW);
    CHECK(tight_ok(FMT_NARROW, 65536, true) && !tight_ok(FMT_NARROW, 65535, true) && !tight_ok(FMT_NARROW, 65536, false) && !tight_ok(FMT_TOP8, 65536, true) && !tight_ok(FMT_PACK8, 1 << 20, true));

    // the headline workload: 3 391 488 regions at k = 21
    CHECK(round_regions(3391488, 21) == 3391488);
    const PartCfg h = plan_cfg(shape(21, 3391488), true);
    CHECK(h.narrow == 1 && h.sub_bits == 6 && h.n_coarse == 256 && h.g_shift == 11);
    const LevelCfg last = level_narrow(h, 6), mid = level_narrow(h, 6, true);
    CHECK(last.n_seg == 16384 && last.nb == 207 && last.nr_shift == 6 && last.nr_div == 1 && last.nr_inv == 0 && last.nr_rps == 13248 && last.nr_sub == 207);
    CHECK(last.nr_mid == 0 && last.nr_fshift == 18 && last.nr_fmask == 262143 && last.nr_f24 == 1 && last.narrow == 1 && last.spb == 1 && last.rstart == nullptr);
    CHECK(mid.n_seg == 256 && mid.nb == 64 && mid.nr_shift == 0 && mid.nr_div == 207 && mid.nr_inv == 20748635 && mid.nr_mid == 1 && mid.nr_f24 == 1);
    CHECK(level_narrow(h, 6, false, true).narrow == 2);
    CHECK(with_rep_shift(last).rep_shift == 1 && with_rep_shift(mid).rep_shift == 2);
    CHECK(part_table_ok(shape(21, 3391488), true) && !part_table_ok(shape(21, 3391488), false) && !part_table_ok(shape(25, 3391488), true));
    CHECK(part_table_ok(shape(25, 1 << 20), true) && !part_table_ok(shape(25, (1 << 20) + 256), true));

    // round_regions is not idempotent: 257 regions per sub-bucket at s = 7, which plan_cfg takes as it is
    CHECK(round_regions(8403324, 21) == 8421376 && round_regions(8421376, 21) == 8454144);
    const PartCfg odd = plan_cfg(shape(21, 8421376), true);
    CHECK(odd.narrow == 1 && odd.sub_bits == 7 && odd.g_shift == 13 && level_narrow(odd, 7).nb == 257 && level_narrow(odd, 7).n_seg == 32768);
    // a table created below 2048 regions and grown by doubling stays off the multiples of 256: packed records
    CHECK(round_regions(257, 21) == 257 && round_regions(257, 29) == 512 && round_regions(1, 21) == 16);
    const GrowTarget g3 = grow_target(257ull * 2048, 257, 5 * 257ull * 2048);
    CHECK(g3.ok && g3.regions == 2056 && g3.slots == 2056ull * 2048);
    const PartCfg grown = plan_cfg(shape(21, 2056), true);
    CHECK(grown.narrow == 0 && grown.g_shift == 3 && grown.n_coarse == 257 && plan_fmt(grown, 21) == FMT_PACK8);
    const GrowTarget same = grow_target(1 << 22, 2048, 1 << 22), win = grow_target(2048 * 2048, 8192, 2048 * 2048 + 1), over = grow_target(1ull << 42, 1ull << 31, (1ull << 42) + 1);
    CHECK(same.ok && same.slots == 1 << 22 && same.regions == 2048 && win.ok && win.slots == 1 << 23 && win.regions == 16384 && !over.ok && over.regions == 1ull << 32);
    CHECK(grow_target(1ull << 41, 1ull << 30, 1ull << 42).ok);

    // windows on a 2048-region allocation
    const WindowGeom w1 = window_geometry(2048, 64, 128, 21), w2 = window_geometry(2048, 0, 128, 21), w3 = window_geometry(2048, 0, 256, 21), w4 = window_geometry(2048, 3, 4, 31);
    CHECK(w1.ok && w1.virt == 8192 && w1.alloc_new == 2048 && w2.ok && w2.virt == 4096 && w2.alloc_new == 2048 && w3.ok && w3.virt == 2048 && w3.alloc_new == 2048);
    CHECK(w4.ok && w4.virt == 524288 && w4.alloc_new == 2048);
    CHECK(!window_geometry(1ull << 24, 0, 1, 21).ok && window_geometry((1ull << 24) - 256, 0, 1, 21).ok);

    // main table at load 0.85, side table
    CHECK(main_need(0, 0) == 2048 && main_need(80, 5) == 2148 && main_need(1000000, 234567) == 1454479);
    CHECK(hc_need(0) == 2 && hc_need(255000) == 2002 && hc_need(255ull * ((1 << 23) - 1)) == 1 << 24 && !hc_follows_fill(255ull * (1 << 23) - 1));
    CHECK(hc_follows_fill(255ull << 23) && hc_need(255ull << 23) == HC_CAP_BIG && hc_need(255ull << 23, 1 << 22) == 1 << 25 && hc_need(255ull << 23, (1 << 22) + 1) == (1 << 25) + 8);

    // owner parts
    CHECK(part_first_bucket(0, 3) == 0 && part_first_bucket(1, 3) == 86 && part_first_bucket(2, 3) == 171 && part_first_bucket(3, 3) == 256 && part_first_bucket(1, 256) == 1 && part_first_bucket(7, 8) == 224);
    CHECK(owner_sub_bits(1) == 5 && owner_sub_bits(3) == 5 && owner_sub_bits(8) == 5 && owner_sub_bits(9) == 4 && owner_sub_bits(128) == 1 && owner_sub_bits(129) == 0 && owner_sub_bits(2047) == 0);

    // levels of the coarse plans
    const LevelCfg cr = level_coarse_to_regions(plan_cfg(shape(25, 65536))), fc = level_flat_to_coarse(plan_cfg(shape(25, 65536)));
    CHECK(cr.n_regions == 65536 && cr.n_seg == 512 && cr.nb == 128 && cr.seg_shift == 7 && cr.out_shift == 0 && cr.narrow == 0 && cr.nr_div == 1 && cr.nr_fshift == 24 && cr.nr_fmask == 0xFFFFFFu && cr.spb == 1);
    CHECK(fc.n_seg == 1 && fc.nb == 512 && fc.seg_shift == 32 && fc.out_shift == 7 && fc.in_raw == 0 && fc.top8 == 0 && fc.spb == 1);
    struct { uint32_t nb, rs; } reps[] = {{1, 6}, {3, 6}, {7, 6}, {15, 5}, {64, 2}, {127, 2}, {128, 1}, {207, 1}, {255, 1}, {256, 0}, {2047, 0}};
    for (auto& r : reps) { LevelCfg lv = cr; lv.nb = r.nb; CHECK(with_rep_shift(lv).rep_shift == r.rs && with_rep_shift(lv).nb == r.nb); }
}

static void sets_and_layout_table() {
    // one pending set of 1 000 001 records on 65 536 regions, per format: {has_aux, aux_off, base_off, total}
    struct { int fmt; bool aux; size_t aux_off, base_off, total; } sets[] = {{FMT_PACK8, false, 8000064, 8000064, 8524544}, {FMT_WIDE, true, 8000064, 9000128, 9524480},
        {FMT_NARROW, true, 4000064, 5000128, 5524480}, {FMT_TOP8, false, 8000064, 8000064, 8524544}, {FMT_TIGHT, false, 4000064, 4000064, 4524544}};
    for (auto& s : sets) { const SetLayout l = set_bytes(1000001, s.fmt, 65536); CHECK(l.has_aux == s.aux && l.aux_off == s.aux_off && l.base_off == s.base_off && l.total == s.total); }

    // a plan in full: 1 000 003 starts in 249 tiles at k = 21 on 65 536 regions, 256 CUs
    const PlanSizes p = plan_sizes(shape(21, 65536), 256, 1000003, 249, 256, true, 0);
    CHECK(p.fmt == FMT_NARROW && p.two_level && p.n_max == 1000008 && p.R == 65536 && p.g1 == 249 && p.m1_n == 63744 && p.m2_n == 81664 && p.groups_n == 65538 && p.sums_n == 6);
    CHECK(p.seg_max == 256 && p.rec_words == 500006 && p.aux_words == 125002 && !p.split2);
    const PlanLayout l = plan_layout(p);
    CHECK(l.recs1 == 0 && l.aux1 == 500006 && l.recs2 == 625008 && l.aux2 == 1125014 && l.m1 == 1250016 && l.seg_off == 1313760 && l.unit_base == 1314018 && l.group_base == 1314276);
    CHECK(l.sums == 1379814 && l.total == 1379820 && l.hot == 1379824 && l.m2 == 1445362 && l.words == 1486194 && l.part2_bytes == 0);
    // records handed in (no tiles, one P1 bin) on a 280-region table: with n_max = 8 m the lockstep array has m + 1 words, so
    // the second record array starts on an odd 8-byte word when m is even
    const PlanSizes q = plan_sizes(shape(25, 280), 256, 4090, 0, 1, false, 0);
    CHECK(q.fmt == FMT_PACK8 && !q.two_level && q.n_max == 4096 && q.g1 == 1 && q.m1_n == 1 && q.m2_n == 574000 && q.groups_n == 282 && q.sums_n == 2 && q.seg_max == 2048 && q.rec_words == 4096 && q.aux_words == 513);
    const PlanLayout lq = plan_layout(q);
    CHECK(lq.aux1 == 4096 && lq.recs2 == 4609 && lq.aux2 == 8705 && lq.m1 == 9218 && lq.seg_off == 9219 && lq.unit_base == 11269 && lq.group_base == 13319 && lq.sums == 13601 && lq.total == 13603 && lq.hot == 13607 && lq.m2 == 13889 && lq.words == 300889);
    // a slice of the headline workload: the second record array in a buffer of its own
    const PlanSizes b = plan_sizes(shape(21, 3391488), 256, 1ull << 27, 33289, 256, true, 0);
    CHECK(b.split2 && b.g1 == 4608 && b.m1_n == 1179648 && b.m2_n == 50335744 && b.groups_n == 3391490 && b.sums_n == 209 && b.seg_max == 16384 && b.rec_words == 67108866 && b.aux_words == 16777217);
    const PlanLayout lb = plan_layout(b);
    CHECK(lb.aux1 == 67108866 && lb.recs2 == 0 && lb.aux2 == 67108866 && lb.part2_bytes == 83886083ull * 8 && lb.m1 == 83886083 && lb.seg_off == 85065731 && lb.unit_base == 85082117 && lb.group_base == 85098503);
    CHECK(lb.sums == 88489993 && lb.total == 88490202 && lb.hot == 88490206 && lb.m2 == 91881696 && lb.words == 117049568);
    // scatter workgroups: 18 per CU below 512 P1 bins, 12 from there; an exchange level's segments widen the tables
    CHECK(plan_sizes(shape(21, 2048), 256, 8, 1000000, 511, true, 0).g1 == 4608 && plan_sizes(shape(21, 2048), 256, 8, 1000000, 512, true, 0).g1 == 3072 && plan_sizes(shape(21, 2048), 256, 8, 3071, 512, true, 0).g1 == 3071);
    const PlanSizes x = plan_sizes(shape(21, 2048), 256, 8, 0, 1, true, 4096);
    CHECK(x.seg_max == 4096 && x.groups_n == 4098 && x.m2_n == (0 + 4096 + 2) * 256);
}

static void slice_table() {
    alignas(16) static char text[64];
    alignas(16) static uint16_t inv[4];
    // ASCII: the scan starts one base left of `a` (none at a = 0), at the 16-byte line below it
    SliceView v = slice_view(text, nullptr, 60, 21, 0, 10);
    CHECK(v.ab == (const uint8_t*)text && v.lead == 0 && v.len == 31 && v.er.lo == 0 && v.er.hi == 10 && v.pinv == nullptr);
    v = slice_view(text, nullptr, 60, 21, 16, 30);
    CHECK(v.ab == (const uint8_t*)text && v.lead == 15 && v.len == 36 && v.er.lo == 1 && v.er.hi == 15);
    v = slice_view(text, nullptr, 60, 21, 17, 40);
    CHECK(v.ab == (const uint8_t*)text + 16 && v.lead == 0 && v.len == 44 && v.er.lo == 1 && v.er.hi == 24);      // (clipped at the end of the sequence)
    v = slice_view(text + 3, nullptr, 40, 21, 0, 20);
    CHECK(v.ab == (const uint8_t*)text && v.lead == 3 && v.len == 40 && v.er.hi == 20);
    // packed: words of 16 bases, masks alongside
    v = slice_view(text, inv, 60, 21, 0, 10);
    CHECK(v.ab == (const uint8_t*)text && v.pinv == inv && v.lead == 0 && v.len == 31 && v.er.lo == 0 && v.er.hi == 10);
    v = slice_view(text, inv, 60, 21, 16, 30);
    CHECK(v.ab == (const uint8_t*)text && v.pinv == inv && v.lead == 15 && v.len == 36 && v.er.lo == 1 && v.er.hi == 15);
    v = slice_view(text, inv, 60, 21, 33, 40);
    CHECK(v.ab == (const uint8_t*)text + 8 && v.pinv == inv + 2 && v.lead == 0 && v.len == 28 && v.er.lo == 1 && v.er.hi == 8);

    // slice size: kmers, slice_kmers, slice_user, pend_budget, n_slots, free_b, work_bytes, have_mem_info
    constexpr uint64_t S = 1ull << 28;
    CHECK(choose_slice(S, S, false, -1, 1ull << 34, 0, 0, false) == S && !slice_reads_free(S, S, false, -1, 1ull << 34));          // one slice
    CHECK(choose_slice(3000000000ull, 1000, true, -1, 1ull << 34, ~(size_t)0 >> 1, 0, true) == 1000 && !slice_reads_free(3000000000ull, 1000, true, -1, 1ull << 34));
    // pending sets: equal slices of at most max(2^28, slots / 4), capped at 2^31 -- at 2^30 unless 11 B per start + 2 GiB are free
    CHECK(choose_slice(1300000000, S, false, -1, 1 << 20, 0, 0, false) == 260000000 && !slice_reads_free(1300000000, S, false, -1, 1 << 20));
    CHECK(choose_slice(1ull << 31, S, false, -1, 1ull << 32, 0, 0, false) == 1ull << 30 && !slice_reads_free(1ull << 31, S, false, -1, 1ull << 32));
    CHECK(slice_reads_free(3000000000ull, S, false, -1, 1ull << 34) && slice_reads_free((1ull << 31) + 2, S, false, 5, 1ull << 34));
    CHECK(choose_slice(3000000000ull, S, false, -1, 1ull << 34, 18647483648ull - 5, 5, true) == 1500000000);
    CHECK(choose_slice(3000000000ull, S, false, -1, 1ull << 34, 18647483648ull - 6, 5, true) == 1000000000);
    CHECK(choose_slice(3000000000ull, S, false, -1, 1ull << 34, 18647483648ull, 0, false) == 1000000000);
    // no pending sets: up to two starts per slot, 2^31, and what 24 B per start allow
    CHECK(choose_slice(1ull << 30, S, false, 0, 1 << 27, 24 * GiB, 0, true) == S && !slice_reads_free(1ull << 30, S, false, 0, 1 << 27));
    CHECK(slice_reads_free(1ull << 30, S, false, 0, (1 << 27) + 1) && choose_slice(1ull << 30, S, false, 0, (1 << 27) + 1, 12 * GiB, 0, true) == S + 2);
    CHECK(choose_slice(1ull << 30, S, false, 0, (1 << 27) + 1, 24000, 0, true) == S && choose_slice(1ull << 30, S, false, 0, (1 << 27) + 1, 12 * GiB, 0, false) == S);
    CHECK(choose_slice(1ull << 33, S, false, 0, 1ull << 33, 96 * GiB, 0, true) == 1ull << 31 && choose_slice(1ull << 33, S, false, 0, 1ull << 33, 12 * GiB, 12 * GiB, true) == 1ull << 30);

    // fork: overlap, profile, count_path, kmers, slice, whole table
    CHECK(slices_fork(1, false, 0, 1 << 21, 1 << 20, true) && slices_fork(1, false, 2, (1 << 20) + 1, 1 << 20, true) && slices_fork(2, false, 0, 1 << 21, 1 << 20, false));
    CHECK(!slices_fork(1, false, 0, 1 << 20, 1 << 20, true) && !slices_fork(1, false, 0, 1 << 21, (1 << 20) - 1, true) && !slices_fork(0, false, 0, 1 << 21, 1 << 20, true));
    CHECK(!slices_fork(1, true, 0, 1 << 21, 1 << 20, true) && !slices_fork(1, false, 1, 1 << 21, 1 << 20, true) && !slices_fork(1, false, 0, 1 << 21, 1 << 20, false));

    // partition or direct: n, table_ok, table bytes, regions, pend_budget, pend_records, have_arena, arena_bytes.  A set of 2^20
    // packed records on 2048 regions is 8 405 248 bytes
    CHECK(set_bytes(1 << 20, FMT_PACK8, 2048).total == 8405248);
    CHECK(!slice_partitions((1 << 20) - 1, true, 32 * KiB, 2048, 0, 0, false, 0) && slice_partitions(1 << 20, true, 32 * KiB, 2048, 0, 0, false, 0) && !slice_partitions(1 << 20, false, 32 * KiB, 2048, 0, 0, false, 0));
    CHECK(slice_partitions(1 << 20, true, 209715200, 2048, 0, 0, false, 0) && !slice_partitions(1 << 20, true, 209715216, 2048, 0, 0, false, 0));          // 200 B per record
    CHECK(slice_partitions(1 << 20, true, 1677721600, 2048, -1, 0, false, 0) && !slice_partitions(1 << 20, true, 1677721616, 2048, -1, 0, false, 0));      // ... of 8 slices
    CHECK(slice_partitions(1 << 20, true, 1677721616 + 200000 - 16, 2048, -1, 1000, false, 0) && !slice_partitions(1 << 20, true, 1677721616 + 200000, 2048, -1, 1000, false, 0));
    CHECK(!slice_partitions(1 << 20, true, 209715216, 2048, -1, 0, true, 8405248 / 2) && slice_partitions(1 << 20, true, 2 * 209715200, 2048, -1, 0, true, 2 * 8405248) && !slice_partitions(1 << 20, true, 2 * 209715200 + 16, 2048, 7, 0, true, 2 * 8405248));

    // lookup: per_base, lookup_path, table_ok, kmers, slice_kmers, table bytes
    CHECK(!lookup_partitions(true, 2, true, 1 << 24, S, 32 * KiB) && !lookup_partitions(false, 1, true, 1 << 24, S, 32 * KiB) && !lookup_partitions(false, 2, false, 1 << 24, S, 32 * KiB) && lookup_partitions(false, 2, true, 10, S, 1ull << 40));
    CHECK(!lookup_partitions(false, 0, true, (1 << 20) - 1, S, 32 * KiB) && lookup_partitions(false, 0, true, 1 << 20, S, 64 << 20) && !lookup_partitions(false, 0, true, 1 << 20, S, (64 << 20) + 16));
    CHECK(lookup_partitions(false, 0, true, 1ull << 30, S, 64 * S) && !lookup_partitions(false, 0, true, 1ull << 30, S, 64 * S + 16));

    // arena: need, arena_bytes, was_full, pend_budget -> the size wanted
    CHECK(arena_want(100 * MiB, 0, false, -1) == 400 * MiB && arena_want(MiB, 0, false, -1) == 64 * MiB && arena_want(100 * MiB, 0, false, GiB) == GiB && arena_want(16 * MiB + 1, 16 * MiB, true, -1) == 64 * MiB + 4);
    CHECK(arena_want(100 * MiB, GiB, true, -1) == 2 * GiB && arena_want(100 * MiB, GiB, false, -1) == GiB && arena_want(100 * MiB, GiB, true, 5 * GiB) == GiB && arena_want(GiB, GiB, true, -1) == 2 * GiB);
    // want, need, arena_bytes, pend_budget, free, total, table bytes -> bytes to allocate / 0 = keep / ARENA_STAY
    CHECK(arena_budget(400 * MiB, 100 * MiB, 0, -1, 200 * GiB, 288 * GiB, GiB) == 400 * MiB);
    CHECK(arena_budget(8 * GiB, 100 * MiB, 4 * GiB, -1, 200 * GiB, 288 * GiB, GiB) == 0);                      // four times the table: at its ceiling
    CHECK(arena_budget(8 * GiB, 100 * MiB, 4 * GiB, -1, 200 * GiB, 288 * GiB, GiB + 1) == 4 * GiB + 4);
    CHECK(arena_budget(8 * GiB, 3 * GiB, 4 * GiB, -1, 200 * GiB, 288 * GiB, GiB) == 8 * GiB);                  // ... or four sets
    CHECK(arena_budget(24 * GiB, 6 * GiB, 0, -1, 10 * GiB, 288 * GiB, 100 * GiB) == ARENA_STAY);               // half of what is free when the reserve is tight
    CHECK(arena_budget(20 * GiB, 5 * GiB, 0, -1, 10 * GiB, 288 * GiB, 100 * GiB) == 5 * GiB);
    CHECK(arena_budget(100 * GiB, GiB, 0, -1, 72 * GiB, 288 * GiB, 100 * GiB) == 36 * GiB && arena_budget(100 * GiB, GiB, 0, -1, 72 * GiB + 2, 288 * GiB, 100 * GiB) == 36 * GiB + 2);
    CHECK(arena_budget(100 * GiB, GiB, 2 * GiB, -1, 70 * GiB + 2, 288 * GiB, 100 * GiB) == 36 * GiB + 2);      // (the arena it replaces counts as free)
    CHECK(arena_budget(100 * GiB, GiB, 0, -1, 20 * GiB, 16 * GiB, 100 * GiB) == 12 * GiB);                     // reserve: 1/8 of the device, 8 GiB at least
    CHECK(arena_budget(GiB, 2 * GiB, 0, GiB, 200 * GiB, 288 * GiB, GiB) == ARENA_STAY && arena_budget(GiB, 512 * MiB, 0, GiB, GiB, 288 * GiB, GiB) == GiB);      // a fixed budget is taken as it is
}

// ---- (b) invariants over the sweep ------------------------------------------------------------------------------------
static uint64_t n_cases = 0;
struct Span { uint64_t at, n; };
static void check_spans(Span* s, size_t n, uint64_t words) {
    std::sort(s, s + n, [](const Span& a, const Span& b) { return a.at < b.at; });
    for (size_t i = 0; i + 1 < n; ++i) CHECK(s[i].at + s[i].n <= s[i + 1].at);
    CHECK(s[n - 1].at + s[n - 1].n <= words);
}
// `base_bucketed`: the table was created with a geometry of hash-prefix buckets, so that doubling keeps one
static void check_geometry(int k, uint64_t R, bool base_bucketed) {
    ++n_cases;
    CHECK(R % 256 == 0 || (R < 2048 && k < HI_K) || !base_bucketed);
    const TableShape t = shape(k, R);
    const PartCfg c = plan_cfg(t, true);
    const uint64_t rps = R >> NARROW_CBITS;
    if (c.narrow) {
        CHECK(R % 256 == 0 && rps % (1ull << c.sub_bits) == 0 && (rps >> c.sub_bits) < (uint64_t)NB_MAX && (256ull << c.sub_bits) <= (uint64_t)SEG_MAX && c.n_coarse == 256);
        for (bool middle : {false, true}) {
            if (middle && !c.sub_bits) continue;
            const LevelCfg lv = with_rep_shift(level_narrow(c, c.sub_bits, middle));
            CHECK(((uint64_t)(lv.nb + 1) << lv.rep_shift) <= 512 || lv.rep_shift == 0);
            CHECK(lv.rep_shift <= 6 && lv.nb < (uint32_t)NB_MAX && (uint64_t)lv.n_seg * lv.nb == (middle ? 256ull << c.sub_bits : R));
        }
    } else if (R <= (1ull << 20)) {
        CHECK(c.n_coarse < (uint32_t)NB_MAX && (1ull << c.g_shift) < (uint64_t)NB_MAX && ((uint64_t)c.n_coarse << c.g_shift) >= R);
        const LevelCfg lv = with_rep_shift(level_coarse_to_regions(c));
        CHECK(((uint64_t)(lv.nb + 1) << lv.rep_shift) <= 512 || lv.rep_shift == 0);
        CHECK(lv.rep_shift <= 6);
    }
    // geometries of hash-prefix buckets: what kq_create makes from 2048 regions up at k <= 21, and at k >= 29 at any size (there
    // the buckets exist below 2048 regions too, but records take them only from 2048 regions: see the table above)
    if (R >= 2048 && (k >= HI_K || (k <= (int)NARROW_MAX_K && base_bucketed))) CHECK(c.narrow == 1 && part_table_ok(t, true));
    for (uint64_t n_max : {8ull, 4096ull, 1ull << 20, 1ull << 31})
        for (uint64_t n_tiles : {1ull, 1000000ull}) {
            const PlanSizes p = plan_sizes(t, 256, n_max, n_tiles, c.n_coarse, true, 0);
            const PlanLayout l = plan_layout(p);
            // the second record array and its lockstep bytes last: in a buffer of their own when split2
            Span s[12] = {{l.recs1, p.rec_words}, {l.aux1, p.aux_words}, {l.m1, p.m1_n}, {l.seg_off, p.seg_max + 2}, {l.unit_base, p.seg_max + 2}, {l.group_base, p.groups_n},
                          {l.sums, p.sums_n}, {l.total, 4}, {l.hot, R + 2}, {l.m2, (p.m2_n + 1) / 2}, {l.recs2, p.rec_words}, {l.aux2, p.aux_words}};
            CHECK(p.split2 == ((p.rec_words + p.aux_words) * 8 >= 512 * MiB) && p.split2 == (l.part2_bytes != 0));
            if (p.split2) { check_spans(s + 10, 2, l.part2_bytes / 8); CHECK(l.part2_bytes % 8 == 0); }
            check_spans(s, p.split2 ? 10 : 12, l.words);
            CHECK(p.n_max >= n_max && p.n_max % 8 == 0 && p.rec_words * 8 >= p.n_max * (p.fmt == FMT_NARROW ? 4 : 8) && p.aux_words * 8 >= p.n_max);
            CHECK((l.words - l.m2) * 2 >= p.m2_n && p.sums_n >= std::max(p.m1_n, p.groups_n) / SCAN_CHUNK + 2 && p.groups_n >= R + 2);
            CHECK(p.seg_max >= (c.narrow ? 256ull << c.sub_bits : (uint64_t)c.n_coarse));
        }
    for (int fmt : {FMT_PACK8, FMT_WIDE, FMT_NARROW, FMT_TOP8, FMT_TIGHT})
        for (uint64_t n_max : {8ull, 4099ull, 1ull << 31}) {
            const SetLayout s = set_bytes(n_max, fmt, R);
            CHECK(s.aux_off <= s.base_off && s.base_off < s.total && s.aux_off % 64 == 0 && s.base_off % 64 == 0 && s.total % 256 == 0 && s.total - s.base_off >= (R + 2) * 8);
            CHECK(s.aux_off >= n_max * (fmt == FMT_NARROW || fmt == FMT_TIGHT ? 4 : 8) && s.has_aux == (s.base_off - s.aux_off >= n_max && s.base_off != s.aux_off));
        }
}
static void sweep() {
    for (int e = 4; e <= 24; ++e)
        for (int64_t r = (1ll << e) - 600; r <= (1ll << e) + 600; ++r) {
            if (r < 1) continue;
            for (int k : {15, 21, 25, 29, 32}) {
                const uint64_t base = round_regions((uint64_t)r, k);
                CHECK(base >= (uint64_t)r);
                CHECK(base % 256 == 0 || (base < 2048 && k < HI_K));
                for (int d = 0; d < 4; ++d)
                    if ((base << d) <= (1ull << 24)) check_geometry(k, base << d, base >= 2048 || k >= HI_K);
            }
        }
    for (uint32_t nb = 1; nb < (uint32_t)NB_MAX; ++nb) {
        LevelCfg lv = level_flat_to_coarse(plan_cfg(shape(25, 280))); lv.nb = nb;
        const uint32_t rs = with_rep_shift(lv).rep_shift;
        CHECK((((uint64_t)nb + 1) << rs) <= 512 || rs == 0);
        CHECK(rs <= 6 && (rs == 6 || (((uint64_t)nb + 1) << (rs + 1)) > 512));
    }
}
// consecutive slices tile [0, kmers): every k-mer start is emitted by exactly one slice, whose scan covers its k bases and both
// neighbours
static void slice_walk() {
    std::vector<char> text(5000 + 16);
    std::vector<uint16_t> inv(5000 / 16 + 2);
    for (bool packed : {false, true})
        for (uint64_t off : {0u, 5u})
            for (int k : {2, 21, 32})
                for (uint64_t len : {32ull, 33ull, 4999ull})
                    for (uint64_t slice : {1ull, 15ull, 16ull, 17ull, 1000ull, 4096ull, 1ull << 28}) {
                        const char* d = text.data() + (packed ? 0 : off);
                        const uint64_t kmers = len - k + 1;
                        uint64_t next = 0;
                        for (uint64_t a = 0; a < kmers; a += slice) {
                            const uint64_t b = std::min(kmers, a + slice);
                            const SliceView v = slice_view(d, packed ? inv.data() : nullptr, len, k, a, b);
                            // position of the scan's first base in the sequence
                            const uint64_t first = packed ? (uint64_t)(v.ab - (const uint8_t*)d) / 4 * 16 + v.lead : (uint64_t)(v.ab + v.lead - (const uint8_t*)d);
                            CHECK(first + v.er.lo == next && first + v.er.hi == b && v.er.lo < v.er.hi);
                            CHECK(first == (a ? a - 1 : 0) && first + v.len == std::min(len, b + k) && v.er.hi - 1 + k <= v.len);
                            CHECK(packed ? (v.lead < 16 && v.pinv == inv.data() + (v.ab - (const uint8_t*)d) / 4) : (v.lead < 16 && (uintptr_t)v.ab % 16 == 0 && v.pinv == nullptr));
                            next = b;
                        }
                        CHECK(next == kmers);
                    }
}

int main() {
    geometry_table();
    sets_and_layout_table();
    slice_table();
    sweep();
    slice_walk();
    printf("count-path sizing: %llu geometries, %d failures\n", (unsigned long long)n_cases, bad);
    return bad ? 1 : 0;
}
