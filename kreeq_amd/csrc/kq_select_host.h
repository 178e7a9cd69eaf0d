// kq_select_host.h -- which kernel instantiation every stage of the partitioned path launches (run_p1, run_level, sort_to_regions,
// flush_pending_base and lookup_partitioned in kreeq_amd.hip).  One pure function per decision, from plain values to a descriptor:
// the kernel family and its template arguments.  The launchers in kreeq_amd.hip list the instantiations of each family once and
// refuse a descriptor they do not list.  Host arithmetic only, no device code, so that the decisions are checked by a stand-alone
// program (tests/native/select_main.cpp) against a table written out by hand.
#pragma once
#include "kq_formats.h"

namespace kq {

// KQ_OPT_KERNEL_SET (include/kreeq_amd.h; measurement only): a set bit runs the ALTERNATIVE kernel of its stage
constexpr int KS_P1_ROUND2 = 1,          // P1 scatter of 5-byte and hash-remainder records: k_p1_scatter, not the streamed k_p1_scatter_s
              KS_LV_NARROW_S = 2,        // levels that write narrow records: k_lv_scatter_s<false>, not k_lv_scatter
              KS_LV_TIGHT_UNITS = 4,     // the level that writes tight records: k_lv_scatter, not k_lv_scatter_s<true>
              KS_P3_SET_OFFSETS = 16,    // table pass of 4- and 5-byte records: the sets' own offset arrays, not the region-major matrix
              KS_SEG_NEVER = 32,         // last level behind a middle level: the unit path also for even buckets
              KS_SEG_ALWAYS = 64,        // ... the segment kernel wherever it applies, whatever the buckets look like
              KS_P1_NO_COMPACT = 128,    // filtered narrow P1 scatter: k_p1_scatter_s<4, K, 1>, not k_p1_scatter_c
              KS_ALL = KS_P1_ROUND2 | KS_LV_NARROW_S | KS_LV_TIGHT_UNITS | KS_P3_SET_OFFSETS | KS_SEG_NEVER | KS_SEG_ALWAYS | KS_P1_NO_COMPACT;

enum Kernel { K_P1_HIST, K_P1_SCATTER, K_P1_SCATTER_S, K_P1_SCATTER_C, K_LV_HIST, K_LV_SCATTER, K_LV_SCATTER_S, K_LV_SEGMENT_S, K_LV_UNITS /*the unit path: run_level*/,
              K_COUNT_REGIONS, K_COUNT_REGIONS_Q4, K_COUNT_REGIONS_Q4R, K_LOOKUP_REGIONS };
// A family and its template arguments by name; a family without an argument of that name leaves it 0:
//   k_p1_hist<bin, kc>   k_p1_scatter<fmt, nbc, bin, kc>   k_p1_scatter_s<bin, kc, tpr, flag = TOP8>   k_p1_scatter_c<kc>
//   k_lv_hist<fmt>       k_lv_scatter<fmt, nbc>            k_lv_scatter_s<flag = TIGHT>
//   k_count_regions<fmt, flag = HOT>   k_count_regions_q4 / _q4r<kc, flag = TIGHT>   k_lookup_regions<fmt>
struct KernelSel {
    Kernel fam; int fmt = 0, nbc = 0, bin = 0, kc = 0, tpr = 0; bool flag = false;
    bool operator==(const KernelSel& o) const { return fam == o.fam && fmt == o.fmt && nbc == o.nbc && bin == o.bin && kc == o.kc && tpr == o.tpr && flag == o.flag; }
};
inline KernelSel sel_of(Kernel fam, int fmt, int nbc, int bin, int kc, int tpr = 0, bool flag = false) { KernelSel s{fam}; s.fmt = fmt; s.nbc = nbc; s.bin = bin; s.kc = kc; s.tpr = tpr; s.flag = flag; return s; }

// ---- P1: the scan of the bases.  mode / narrow / map_mask: PartCfg's; full_range: the map-range filter keeps every map; windowed:
// the table is a window of the hash-prefix buckets (PartCfg::win_lo / win_hi are not 0 / 256).  What kind of pass it is:
//   plain: no owner split, no map-range filter (branch-free bin functions)     owner_plain: multi-GPU owner split
//   narrow_filt: map-range pass on a bucketed table                            narrow_win: windowed table, own buckets only
struct P1Case { bool plain, owner_plain, narrow_filt, narrow_win; };
inline P1Case p1_case(int k, uint32_t mode, uint32_t narrow, uint32_t map_mask, bool full_range, bool windowed) {
    const bool plain = mode == 0 && full_range;
    return P1Case{plain, mode == 1 && map_mask != 0 && full_range, mode == 0 && narrow && !plain && map_mask != 0 && k <= (int)NARROW_MAX_K,
                  plain && narrow && (k <= (int)NARROW_MAX_K || k > PART_MAX_K) && windowed};
}
// the histogram goes by bin mode: 3 owner, 4 filtered buckets, 6 windowed buckets, 0 generic, 2 buckets, 1 regions / coarse buckets
inline KernelSel select_p1_hist(int k, uint32_t mode, uint32_t narrow, uint32_t map_mask, bool full_range, bool windowed) {
    const P1Case c = p1_case(k, mode, narrow, map_mask, full_range, windowed);
    const int bin = c.owner_plain ? 3 : c.narrow_filt ? 4 : c.narrow_win ? 6 : !c.plain ? 0 : narrow ? 2 : 1;
    return sel_of(K_P1_HIST, 0, 0, bin, bin == 0 ? 0 : bin == 1 ? (k == 31 ? 31 : 0) : bin == 6 && k == 31 ? 31 : k == 21 ? 21 : 0);
}
// KQ_OPT_COUNT_MAP_PASSES: the one launch that fills the cached count matrix a pass of bin mode 4 (every map range at once: bin
// mode 5) or 6 (every bucket: bin mode 2) takes its counts from.  Its grid is g1, not g1 * P1_F
inline KernelSel select_p1_hist_cached(int k, int pass_bin) { return sel_of(K_P1_HIST, 0, 0, pass_bin == 4 ? 5 : 2, k == 21 ? 21 : 0); }
// lockstep: the scatter writes lockstep bytes (WIDE records when the plan is not narrow); tpr: tiles per round of an unfiltered
// streamed scatter (KQ_P1S_TPR; filtered and windowed ones take 1)
inline KernelSel select_p1_scatter(int k, uint32_t mode, uint32_t narrow, uint32_t map_mask, bool full_range, bool windowed, bool lockstep,
                                   uint32_t n_coarse, int tpr, int kernel_set) {
    const P1Case c = p1_case(k, mode, narrow, map_mask, full_range, windowed);
    const bool small = n_coarse < 512;                       // 48 KiB LDS variant: three workgroups per CU
    const int nbc = small ? 512 : NB_MAX, kc21 = k == 21 ? 21 : 0, kc31 = k == 31 ? 31 : 0;
    if (narrow) {
        const bool top8 = k > PART_MAX_K;                     // hash-remainder records (k = 29..32), else 5-byte records
        int bin, kc, t = 1;
        if (top8) { bin = c.narrow_win ? 6 : c.plain ? 2 : 0; kc = bin ? kc31 : 0; }
        else if (c.narrow_filt) { bin = 4; kc = kc21; }
        else if (c.narrow_win) { bin = 6; kc = kc21; }
        else if (c.plain) { bin = 2; kc = kc21; t = tpr; }    // a pass that keeps every k-mer splits several tiles per round
        else { bin = 0; kc = 0; }
        if (kernel_set & KS_P1_ROUND2) return sel_of(K_P1_SCATTER, top8 ? FMT_TOP8 : FMT_NARROW, 512, bin, kc);
        // behind the map-range filter: survivors compacted ahead of the hash
        if (bin == 4 && !(kernel_set & KS_P1_NO_COMPACT)) return sel_of(K_P1_SCATTER_C, 0, 0, 0, kc);
        return sel_of(K_P1_SCATTER_S, 0, 0, bin, kc, t, top8);
    }
    if (lockstep) return c.plain && k == 31 ? sel_of(K_P1_SCATTER, FMT_WIDE, nbc, 1, 31) /*the HiFi k*/ : sel_of(K_P1_SCATTER, FMT_WIDE, nbc, 0, 0);
    if (c.owner_plain && small) return sel_of(K_P1_SCATTER, FMT_PACK8, 512, 3, kc21);
    return sel_of(K_P1_SCATTER, FMT_PACK8, nbc, c.plain ? 1 : 0, 0);
}

// ---- split levels.  lv_narrow / lv_top8: LevelCfg's narrow (2: hash-remainder records) / top8 (packed in, narrow out); rstart: the
// level writes tight records
inline int level_format(uint32_t lv_narrow, bool lockstep) { return lv_narrow == 2 ? FMT_TOP8 : lv_narrow ? FMT_NARROW : lockstep ? FMT_WIDE : FMT_PACK8; }
inline KernelSel select_level_hist(uint32_t lv_narrow, bool lockstep) { return sel_of(K_LV_HIST, level_format(lv_narrow, lockstep), 0, 0, 0); }
inline KernelSel select_level_scatter(uint32_t lv_narrow, bool lockstep, bool lv_top8, uint32_t nb, bool rstart, int kernel_set) {
    const int fmt = level_format(lv_narrow, lockstep), nbc = nb < 512 ? 512 : NB_MAX;
    if (lv_top8) return sel_of(K_LV_SCATTER, FMT_PACK8_TO_NARROW, 512, 0, 0);
    // narrow records, at most 512 (bin, replica) counters: the streamed scatter for the level that writes tight records
    if (fmt == FMT_NARROW && nb < 512 && (rstart ? !(kernel_set & KS_LV_TIGHT_UNITS) : (kernel_set & KS_LV_NARROW_S) != 0)) return sel_of(K_LV_SCATTER_S, 0, 0, 0, 0, 0, rstart);
    return sel_of(K_LV_SCATTER, fmt == FMT_NARROW && rstart ? FMT_NARROW_TO_TIGHT : fmt, nbc, 0, 0);
}
// The last level of a plan with a middle level (nr_shift != 0), narrow records in and tight records out, fewer than 512 regions
// per segment, one input segment per logical one: one workgroup per segment (k_lv_segment_s) when the slice's buckets are even
// (kq_seg_gate_host.h), else the unit path, which splits a hot sub-bucket over many workgroups
inline KernelSel select_last_level(int plan_fmt, uint32_t lv_narrow, bool rstart, uint32_t nr_shift, uint32_t nb, uint32_t spb, bool even_buckets, int kernel_set) {
    const bool ok = plan_fmt == FMT_NARROW && lv_narrow == 1 && rstart && nr_shift != 0 && nb < 512 && spb == 1;
    return sel_of(ok && ((kernel_set & KS_SEG_ALWAYS) || (even_buckets && !(kernel_set & KS_SEG_NEVER))) ? K_LV_SEGMENT_S : K_LV_UNITS, 0, 0, 0, 0);
}

// ---- table pass and region-wise lookup.  Does the pass over sets of this format read the region-major offset matrix (if there is
// memory for it)?
inline bool table_pass_wants_matrix(int fmt, int kernel_set) { return (fmt == FMT_TIGHT || fmt == FMT_NARROW) && !(kernel_set & KS_P3_SET_OFFSETS); }
// ordinary regions of 4- and 5-byte records: the compact 32-bit-key kernel, from the matrix when the pass has one
inline KernelSel select_table_pass(int fmt, int k, bool matrix) {
    if (fmt == FMT_TIGHT || fmt == FMT_NARROW) return sel_of(matrix ? K_COUNT_REGIONS_Q4R : K_COUNT_REGIONS_Q4, 0, 0, 0, k == 21 ? 21 : 0, 0, fmt == FMT_TIGHT);
    return sel_of(K_COUNT_REGIONS, fmt, 0, 0, 0);
}
// the skewed regions the pass listed: the generic folding kernel (AUX_TIGHT tells it about FMT_TIGHT sets)
inline KernelSel select_hot_pass(int fmt) { return sel_of(K_COUNT_REGIONS, fmt == FMT_TIGHT ? FMT_NARROW : fmt, 0, 0, 0, 0, true); }
inline KernelSel select_lookup(int fmt) { return sel_of(K_LOOKUP_REGIONS, fmt, 0, 0, 0); }

}  // namespace kq
