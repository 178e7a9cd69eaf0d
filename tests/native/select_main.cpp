// Stand-alone check of the kernel selector (kreeq_amd/csrc/kq_select_host.h), meant to be built with -fsanitize=address,undefined.
// Every decision is compared with a table written out by hand from the launch ladders the selector replaced: one row for every
// way a handle reaches an instantiation (k, map range, window, owner mode, lockstep bytes, fan-out on both sides of 512, region
// starts, even buckets, offset matrix, every KQ_OPT_KERNEL_SET bit).  The expected descriptors are printed as "ROW <maker> <args>",
// in the notation of the launcher lists of kreeq_amd.hip, so that tests/test_select_host.py can compare the two sets.
#include <cstdio>
#include <set>
#include <string>

#include "kq_select_host.h"

using namespace kq;

static int bad = 0;
static std::set<std::string> reached;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++bad; } } while (0)

static std::string name(const KernelSel& s) {
    char b[96];
    switch (s.fam) {
        case K_P1_HIST: snprintf(b, sizeof b, "p1h %d,%d", s.bin, s.kc); break;
        case K_P1_SCATTER: snprintf(b, sizeof b, "p1w %d,%d,%d,%d", s.fmt, s.nbc, s.bin, s.kc); break;
        case K_P1_SCATTER_S: snprintf(b, sizeof b, "p1s %d,%d,%d,%d", s.bin, s.kc, s.tpr, (int)s.flag); break;
        case K_P1_SCATTER_C: snprintf(b, sizeof b, "p1c %d", s.kc); break;
        case K_LV_HIST: snprintf(b, sizeof b, "lvh %d", s.fmt); break;
        case K_LV_SCATTER: snprintf(b, sizeof b, "lvw %d,%d", s.fmt, s.nbc); break;
        case K_LV_SCATTER_S: snprintf(b, sizeof b, "lvs %d", (int)s.flag); break;
        case K_COUNT_REGIONS: snprintf(b, sizeof b, "p3g %d,%d", s.fmt, (int)s.flag); break;
        case K_COUNT_REGIONS_Q4: snprintf(b, sizeof b, "p3q %d,%d", s.kc, (int)s.flag); break;
        case K_COUNT_REGIONS_Q4R: snprintf(b, sizeof b, "p3r %d,%d", s.kc, (int)s.flag); break;
        case K_LOOKUP_REGIONS: snprintf(b, sizeof b, "lkr %d", s.fmt); break;
        default: snprintf(b, sizeof b, "form %d", (int)s.fam); break;
    }
    return b;
}
// got == want, field by field (a family's unused fields are 0); the expected descriptor joins the set that is printed
static void expect(int line, const KernelSel& got, const KernelSel& want) {
    reached.insert(name(want));
    if (!(got == want)) { fprintf(stderr, "line %d: selected %s (family %d), expected %s (family %d)\n", line, name(got).c_str(), (int)got.fam, name(want).c_str(), (int)want.fam); ++bad; }
}
#define EXPECT(got, ...) expect(__LINE__, got, sel_of(__VA_ARGS__))

constexpr int TPR = 2;                     // what the library passes (KQ_P1S_TPR)
constexpr uint32_t POW2 = 127, NOPOW2 = 0; // PartCfg::map_mask of 128 maps and of 100 maps
struct P1 { int k; uint32_t mode, narrow, map_mask; bool full, win, lockstep; uint32_t n_coarse; int ks; };
static KernelSel hist(const P1& c) { return select_p1_hist(c.k, c.mode, c.narrow, c.map_mask, c.full, c.win); }
static KernelSel scat(const P1& c, int tpr = TPR) { return select_p1_scatter(c.k, c.mode, c.narrow, c.map_mask, c.full, c.win, c.lockstep, c.n_coarse, tpr, c.ks); }

int main() {
    const int bits[] = {0, 1, 2, 4, 16, 32, 64, 128, 1 | 128};
    CHECK(KS_ALL == (1 | 2 | 4 | 16 | 32 | 64 | 128));
    CHECK(KS_P1_ROUND2 == 1 && KS_LV_NARROW_S == 2 && KS_LV_TIGHT_UNITS == 4 && KS_P3_SET_OFFSETS == 16 && KS_SEG_NEVER == 32 && KS_SEG_ALWAYS == 64 && KS_P1_NO_COMPACT == 128);

    // ---- P1 on a table without hash-prefix buckets (fewer than 2048 regions): packed records up to k = 28, WIDE above -------
    for (int ks : bits) for (uint32_t mask : {POW2, NOPOW2}) for (bool win : {false, true}) for (uint32_t nc : {300u, 511u, 512u, 2047u}) {
        const int nbc = nc < 512 ? 512 : 2048;
        for (int k : {15, 21, 25}) {
            EXPECT(hist({k, 0, 0, mask, true, win, false, nc, ks}), K_P1_HIST, 0, 0, 1, 0);
            EXPECT(scat({k, 0, 0, mask, true, win, false, nc, ks}), K_P1_SCATTER, FMT_PACK8, nbc, 1, 0);
            EXPECT(hist({k, 0, 0, mask, false, win, false, nc, ks}), K_P1_HIST, 0, 0, 0, 0);               // a map-range pass
            EXPECT(scat({k, 0, 0, mask, false, win, false, nc, ks}), K_P1_SCATTER, FMT_PACK8, nbc, 0, 0);
        }
        EXPECT(hist({31, 0, 0, mask, true, win, true, nc, ks}), K_P1_HIST, 0, 0, 1, 31);
        EXPECT(scat({31, 0, 0, mask, true, win, true, nc, ks}), K_P1_SCATTER, FMT_WIDE, nbc, 1, 31);
        EXPECT(hist({30, 0, 0, mask, true, win, true, nc, ks}), K_P1_HIST, 0, 0, 1, 0);
        EXPECT(scat({30, 0, 0, mask, true, win, true, nc, ks}), K_P1_SCATTER, FMT_WIDE, nbc, 0, 0);
        for (int k : {30, 31}) {
            EXPECT(hist({k, 0, 0, mask, false, win, true, nc, ks}), K_P1_HIST, 0, 0, 0, 0);
            EXPECT(scat({k, 0, 0, mask, false, win, true, nc, ks}), K_P1_SCATTER, FMT_WIDE, nbc, 0, 0);
        }
    }
    // ---- the owner split (mode 1): packed records, or WIDE records with the reference edge byte --------------------------------
    for (int ks : bits) for (int k : {15, 21, 25, 30, 31}) {
        const int kc21 = k == 21 ? 21 : 0;
        EXPECT(hist({k, 1, 0, POW2, true, false, false, 256, ks}), K_P1_HIST, 0, 0, 3, kc21);
        EXPECT(hist({k, 1, 0, NOPOW2, true, false, false, 256, ks}), K_P1_HIST, 0, 0, 0, 0);
        EXPECT(scat({k, 1, 0, POW2, true, false, true, 256, ks}), K_P1_SCATTER, FMT_WIDE, 512, 0, 0);
        EXPECT(scat({k, 1, 0, NOPOW2, true, false, true, 256, ks}), K_P1_SCATTER, FMT_WIDE, 512, 0, 0);
        EXPECT(scat({k, 1, 0, POW2, true, false, true, 600, ks}), K_P1_SCATTER, FMT_WIDE, 2048, 0, 0);
        if (k > 28) continue;                                                       // packed records end at k = 28
        EXPECT(scat({k, 1, 0, POW2, true, false, false, 256, ks}), K_P1_SCATTER, FMT_PACK8, 512, 3, kc21);
        EXPECT(scat({k, 1, 0, NOPOW2, true, false, false, 256, ks}), K_P1_SCATTER, FMT_PACK8, 512, 0, 0);
        EXPECT(scat({k, 1, 0, POW2, true, false, false, 600, ks}), K_P1_SCATTER, FMT_PACK8, 2048, 0, 0);
    }
    // ---- P1 on a bucketed table, 5-byte records (k <= 21): 256 bins whatever the table --------------------------------------
    for (int ks : bits) for (int k : {15, 21}) for (bool lockstep : {true, false}) {
        const int kc = k == 21 ? 21 : 0;
        const bool r2 = (ks & 1) != 0;
        // every k-mer kept: KQ_P1S_TPR tiles per round
        EXPECT(hist({k, 0, 1, POW2, true, false, lockstep, 256, ks}), K_P1_HIST, 0, 0, 2, kc);
        if (r2) EXPECT(scat({k, 0, 1, POW2, true, false, lockstep, 256, ks}), K_P1_SCATTER, FMT_NARROW, 512, 2, kc);
        else    EXPECT(scat({k, 0, 1, POW2, true, false, lockstep, 256, ks}), K_P1_SCATTER_S, 0, 0, 2, kc, TPR);
        if (!r2) CHECK(scat({k, 0, 1, NOPOW2, true, false, lockstep, 256, ks}, 3) == sel_of(K_P1_SCATTER_S, 0, 0, 2, kc, 3));    // (the parameter, not a constant)
        // map-range pass, power-of-two map count (with or without a window: the filter goes first)
        for (bool win : {false, true}) {
            EXPECT(hist({k, 0, 1, POW2, false, win, lockstep, 256, ks}), K_P1_HIST, 0, 0, 4, kc);
            if (r2)            EXPECT(scat({k, 0, 1, POW2, false, win, lockstep, 256, ks}), K_P1_SCATTER, FMT_NARROW, 512, 4, kc);
            else if (ks & 128) EXPECT(scat({k, 0, 1, POW2, false, win, lockstep, 256, ks}), K_P1_SCATTER_S, 0, 0, 4, kc, 1);
            else               EXPECT(scat({k, 0, 1, POW2, false, win, lockstep, 256, ks}), K_P1_SCATTER_C, 0, 0, 0, kc);
            // ... any other map count: the generic bin function
            EXPECT(hist({k, 0, 1, NOPOW2, false, win, lockstep, 256, ks}), K_P1_HIST, 0, 0, 0, 0);
            if (r2) EXPECT(scat({k, 0, 1, NOPOW2, false, win, lockstep, 256, ks}), K_P1_SCATTER, FMT_NARROW, 512, 0, 0);
            else    EXPECT(scat({k, 0, 1, NOPOW2, false, win, lockstep, 256, ks}), K_P1_SCATTER_S, 0, 0, 0, 0, 1);
        }
        // bucket window, full map range
        EXPECT(hist({k, 0, 1, NOPOW2, true, true, lockstep, 256, ks}), K_P1_HIST, 0, 0, 6, kc);
        if (r2) EXPECT(scat({k, 0, 1, NOPOW2, true, true, lockstep, 256, ks}), K_P1_SCATTER, FMT_NARROW, 512, 6, kc);
        else    EXPECT(scat({k, 0, 1, NOPOW2, true, true, lockstep, 256, ks}), K_P1_SCATTER_S, 0, 0, 6, kc, 1);
    }
    // ---- P1 on a bucketed table, hash-remainder records (k = 29..32): KC 31 at k = 31 only, and not in the bucket histogram ---
    for (int ks : bits) for (int k : {30, 31}) for (uint32_t mask : {POW2, NOPOW2}) {
        const int kc = k == 31 ? 31 : 0;
        const bool r2 = (ks & 1) != 0;
        EXPECT(hist({k, 0, 1, mask, true, false, false, 256, ks}), K_P1_HIST, 0, 0, 2, 0);
        EXPECT(hist({k, 0, 1, mask, true, true, false, 256, ks}), K_P1_HIST, 0, 0, 6, kc);
        for (bool win : {false, true}) EXPECT(hist({k, 0, 1, mask, false, win, false, 256, ks}), K_P1_HIST, 0, 0, 0, 0);
        if (r2) {
            EXPECT(scat({k, 0, 1, mask, true, false, false, 256, ks}), K_P1_SCATTER, FMT_TOP8, 512, 2, kc);
            EXPECT(scat({k, 0, 1, mask, true, true, false, 256, ks}), K_P1_SCATTER, FMT_TOP8, 512, 6, kc);
            for (bool win : {false, true}) EXPECT(scat({k, 0, 1, mask, false, win, false, 256, ks}), K_P1_SCATTER, FMT_TOP8, 512, 0, 0);
        } else {
            EXPECT(scat({k, 0, 1, mask, true, false, false, 256, ks}), K_P1_SCATTER_S, 0, 0, 2, kc, 1, true);
            EXPECT(scat({k, 0, 1, mask, true, true, false, 256, ks}), K_P1_SCATTER_S, 0, 0, 6, kc, 1, true);
            for (bool win : {false, true}) EXPECT(scat({k, 0, 1, mask, false, win, false, 256, ks}), K_P1_SCATTER_S, 0, 0, 0, 0, 1, true);
        }
    }
    // ---- the cached count matrices of KQ_OPT_COUNT_MAP_PASSES: all map ranges (pass of bin mode 4), all buckets (bin mode 6) ----
    for (int k : {15, 21, 25, 30, 31}) {
        EXPECT(select_p1_hist_cached(k, 4), K_P1_HIST, 0, 0, 5, k == 21 ? 21 : 0);
        EXPECT(select_p1_hist_cached(k, 6), K_P1_HIST, 0, 0, 2, k == 21 ? 21 : 0);
    }

    // ---- split levels ------------------------------------------------------------------------------------------------------
    for (int ks : bits) for (uint32_t nb : {2u, 64u, 511u, 512u, 2047u}) for (bool rstart : {false, true}) {
        const int nbc = nb < 512 ? 512 : 2048;
        // packed and wide records (region starts play no part), hash-remainder records
        EXPECT(select_level_hist(0, false), K_LV_HIST, FMT_PACK8, 0, 0, 0);
        EXPECT(select_level_scatter(0, false, false, nb, rstart, ks), K_LV_SCATTER, FMT_PACK8, nbc, 0, 0);
        EXPECT(select_level_hist(0, true), K_LV_HIST, FMT_WIDE, 0, 0, 0);
        EXPECT(select_level_scatter(0, true, false, nb, rstart, ks), K_LV_SCATTER, FMT_WIDE, nbc, 0, 0);
        for (bool lockstep : {false, true}) {
            EXPECT(select_level_hist(2, lockstep), K_LV_HIST, FMT_TOP8, 0, 0, 0);
            EXPECT(select_level_scatter(2, lockstep, false, nb, rstart, ks), K_LV_SCATTER, FMT_TOP8, nbc, 0, 0);
            EXPECT(select_level_hist(1, lockstep), K_LV_HIST, FMT_NARROW, 0, 0, 0);
        }
        // packed records in, 5-byte records out (the first level of kq_insert_packed_dev on a bucketed table)
        EXPECT(select_level_scatter(0, false, true, nb, rstart, ks), K_LV_SCATTER, FMT_PACK8_TO_NARROW, 512, 0, 0);
        // 5-byte records: the level that writes tight records streams below 512 bins unless bit 4; the others only with bit 2
        if (rstart && nb < 512 && !(ks & 4)) EXPECT(select_level_scatter(1, true, false, nb, true, ks), K_LV_SCATTER_S, 0, 0, 0, 0, 0, true);
        else if (rstart)                     EXPECT(select_level_scatter(1, true, false, nb, true, ks), K_LV_SCATTER, FMT_NARROW_TO_TIGHT, nbc, 0, 0);
        else if (nb < 512 && (ks & 2))       EXPECT(select_level_scatter(1, true, false, nb, false, ks), K_LV_SCATTER_S, 0, 0, 0, 0, 0, false);
        else                                 EXPECT(select_level_scatter(1, true, false, nb, false, ks), K_LV_SCATTER, FMT_NARROW, nbc, 0, 0);
    }
    // ---- last level behind a middle level: segment kernel or unit path ---------------------------------------------------------
    for (int ks : bits) for (bool even : {false, true}) {
        const Kernel form = (ks & 64) || (even && !(ks & 32)) ? K_LV_SEGMENT_S : K_LV_UNITS;
        EXPECT(select_last_level(FMT_NARROW, 1, true, 6, 64, 1, even, ks), form, 0, 0, 0, 0);
        EXPECT(select_last_level(FMT_NARROW, 1, true, 1, 511, 1, even, ks), form, 0, 0, 0, 0);
        // where the segment kernel does not apply: no region starts, no middle level, 512 regions per segment, runs of several
        // peers per segment, hash-remainder records
        EXPECT(select_last_level(FMT_NARROW, 1, false, 6, 64, 1, even, ks), K_LV_UNITS, 0, 0, 0, 0);
        EXPECT(select_last_level(FMT_NARROW, 1, true, 0, 64, 1, even, ks), K_LV_UNITS, 0, 0, 0, 0);
        EXPECT(select_last_level(FMT_NARROW, 1, true, 6, 512, 1, even, ks), K_LV_UNITS, 0, 0, 0, 0);
        EXPECT(select_last_level(FMT_NARROW, 1, true, 6, 64, 2, even, ks), K_LV_UNITS, 0, 0, 0, 0);
        EXPECT(select_last_level(FMT_TOP8, 2, false, 6, 64, 1, even, ks), K_LV_UNITS, 0, 0, 0, 0);
    }
    EXPECT(select_last_level(FMT_NARROW, 1, true, 6, 64, 1, true, 32 | 64), K_LV_SEGMENT_S, 0, 0, 0, 0);      // (64 goes first)
    reached.erase(name(sel_of(K_LV_SEGMENT_S, 0, 0, 0, 0)));                       // forms of the last level, not rows of a launcher list
    reached.erase(name(sel_of(K_LV_UNITS, 0, 0, 0, 0)));

    // ---- table pass ----------------------------------------------------------------------------------------------------------
    for (int ks : bits) {
        CHECK(table_pass_wants_matrix(FMT_TIGHT, ks) == !(ks & 16));
        CHECK(table_pass_wants_matrix(FMT_NARROW, ks) == !(ks & 16));
        for (int fmt : {FMT_PACK8, FMT_WIDE, FMT_TOP8}) CHECK(!table_pass_wants_matrix(fmt, ks));
    }
    for (int k : {15, 21, 25, 30, 31}) for (bool matrix : {false, true}) {
        const int kc = k == 21 ? 21 : 0;
        EXPECT(select_table_pass(FMT_TIGHT, k, matrix), matrix ? K_COUNT_REGIONS_Q4R : K_COUNT_REGIONS_Q4, 0, 0, 0, kc, 0, true);
        EXPECT(select_table_pass(FMT_NARROW, k, matrix), matrix ? K_COUNT_REGIONS_Q4R : K_COUNT_REGIONS_Q4, 0, 0, 0, kc, 0, false);
        for (int fmt : {FMT_PACK8, FMT_WIDE, FMT_TOP8}) EXPECT(select_table_pass(fmt, k, matrix), K_COUNT_REGIONS, fmt, 0, 0, 0);
    }
    // the hot regions behind it: tight and 5-byte sets alike through the FMT_NARROW instantiation
    EXPECT(select_hot_pass(FMT_TIGHT), K_COUNT_REGIONS, FMT_NARROW, 0, 0, 0, 0, true);
    for (int fmt : {FMT_NARROW, FMT_PACK8, FMT_WIDE, FMT_TOP8}) EXPECT(select_hot_pass(fmt), K_COUNT_REGIONS, fmt, 0, 0, 0, 0, true);
    // ---- region-wise lookup --------------------------------------------------------------------------------------------------
    for (int fmt : {FMT_NARROW, FMT_PACK8, FMT_WIDE, FMT_TOP8}) EXPECT(select_lookup(fmt), K_LOOKUP_REGIONS, fmt, 0, 0, 0);

    for (const std::string& r : reached) printf("ROW %s\n", r.c_str());
    printf("kernel selector: %d failures\n", bad);
    return bad ? 1 : 0;
}
