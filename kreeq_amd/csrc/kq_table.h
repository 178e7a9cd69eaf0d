// kq_table.h -- the per-base tables as text on the device (kq_per_base_triples_dev, kq_format_table*; the writers of reference
// src/kreeq-output.cpp:138-303 and the inflate of src/decompressor.cpp:493-585).  Included by kreeq_amd.hip after kq_variants.h.
// The line rules are those of kq_table_core.h; this file places the lines and moves the bytes.
//
// A call's output is a sequence of LINES: the pieces in order, per piece an optional fixedStep header line (KWIG only) and one
// line per position.  line_start[p] = lines before piece p (host-made, n_segs + 1 values), so a line number finds its piece by
// bisection and nothing depends on how lines are dealt to workgroups.  A TILE is TAB_TILE consecutive lines, one per thread.
//
//  1. k_tab_len: every thread computes its line's length from digit counts.  The digit sum of a tile line's triple is staged in
//     LDS once; a line of the expanded formats adds the sums of its k-position window from there, and reads the triples
//     themselves only for the part of the window that lies before the tile or is the piece's history (the k - 1 halo).  The
//     tile's byte count goes to tile_bytes[tile].
//  2. The project's scan (scan_u64) turns tile_bytes into 64-bit tile offsets and the call's size.
//  3. k_tab_write: the same lengths again, a workgroup scan of them, and every thread writes its line through a sink into the
//     WINDOW of the output that the workgroup holds in LDS (TAB_WINDOW bytes, 16-byte aligned in the output's address space;
//     a tile whose text is longer takes several windows, a line may span two).  The window then goes to global memory as one
//     16-byte store per lane, consecutive lanes to consecutive addresses.  A tile owns the 16-byte words that START inside its
//     text: the word that straddles the end of a tile also holds the first bytes of the next tile, so a tile formats up to
//     TAB_EXTRA lines of its successor as well (3 lines are at least 18 bytes).  Only the first and the last word of the whole
//     output can be partial (an output pointer that is not 16-byte aligned, a size that is no multiple of 16): those two are
//     stored byte by byte, by at most 15 lanes each.  Nothing is stored outside [out, out + total).
#pragma once
#include "kq_table_core.h"

namespace kq {

constexpr int TAB_THREADS = 256, TAB_TILE = 256, TAB_EXTRA = 3, TAB_LINES = TAB_TILE + TAB_EXTRA;
constexpr uint32_t TAB_WINDOW = 32768;                                    // bytes of output text per LDS window
constexpr uint32_t TAB_MAX_NAME = 65535;                                   // (a .bkwig stores a header's length in 16 bits)

struct TabArgs {
    const uint32_t* triples;                  // n_triples x (cov, fw, bw)
    const kq_table_seg* segs;                 // the pieces, validated by the host
    const unsigned long long* line_start;     // n_segs + 1
    const char* names;
    uint64_t n_lines;
    uint32_t n_segs;
    int format, k;
};

// one line of the call: its piece's fields and its place in the piece
struct TabLine {
    uint64_t first, abs_pos;                  // of the piece
    const char* name;
    uint32_t name_len, n_ctx;
    uint32_t i;                               // position inside the piece (lines < 2^32 per call)
    bool valid, header;
};

__device__ __forceinline__ TabLine tab_line(const TabArgs& a, uint64_t line) {
    TabLine r;
    r.valid = line < a.n_lines;
    r.header = false; r.first = r.abs_pos = 0; r.name = a.names; r.name_len = r.n_ctx = r.i = 0;
    if (!r.valid) return r;
    uint32_t lo = 0, hi = a.n_segs;                                       // -> the last piece with line_start <= line (it has lines: line < line_start[lo + 1])
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (a.line_start[mid] <= line) lo = mid; else hi = mid; }
    const kq_table_seg s = a.segs[lo];
    uint64_t i = line - a.line_start[lo];
    if (a.format == KQ_TABLE_KWIG && (s.flags & KQ_TABLE_SEG_HEADER)) { r.header = i == 0; i -= r.header ? 0 : 1; }
    r.first = s.first; r.abs_pos = s.abs_pos; r.name = a.names + s.name_off; r.name_len = s.name_len; r.n_ctx = s.n_ctx; r.i = (uint32_t)i;
    return r;
}

// the window of one expanded line: `back` positions before position i of the piece -- from the tile's staged values where that
// line is in the tile (it is then line l - back of the same piece), from the triples where it is the halo or the history,
// 0 before the history
struct TabWin {
    const uint32_t* triples; const uint32_t* s_val; uint64_t at; uint32_t i, n_ctx; int l;
    __device__ __forceinline__ bool staged(int back) const { return (uint32_t)back <= i && back <= l; }
    __device__ __forceinline__ bool known(int back) const { return (uint64_t)back <= (uint64_t)i + n_ctx; }
    __device__ uint32_t operator()(int back, int column) const {
        if (staged(back)) return s_val[(l - back) * 3 + column];
        return known(back) ? triples[(at - (uint64_t)back) * 3 + (uint64_t)column] : 0u;
    }
};

// exclusive scan of one u32 per thread over the workgroup (TAB_THREADS = 4 waves); *total = the sum
__device__ __forceinline__ uint32_t tab_block_scan(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t n = __shfl_up(incl, o, 64); if (lane >= o) incl += n; }
    if (lane == 63) s_wave[w] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < TAB_THREADS / 64; ++j) { const uint32_t x = s_wave[j]; base += j < w ? x : 0u; tot += x; }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

// stage line l of the tile: its triple and digit sum to LDS (a header line: nothing)
__device__ __forceinline__ void tab_stage(const TabArgs& a, const TabLine& ln, int l, uint32_t* s_val, uint8_t* s_dig) {
    uint32_t c = 0, f = 0, b = 0;
    if (ln.valid && !ln.header) { const uint32_t* t = a.triples + (ln.first + ln.i) * 3; c = t[0]; f = t[1]; b = t[2]; }
    s_val[l * 3] = c; s_val[l * 3 + 1] = f; s_val[l * 3 + 2] = b;
    s_dig[l] = (uint8_t)kqtab::fixed_digits(c, f, b);
}
// bytes of line l (0 for a line behind the call's last)
__device__ __forceinline__ uint32_t tab_len(const TabArgs& a, const TabLine& ln, int l, const uint32_t* s_val, const uint8_t* s_dig) {
    if (!ln.valid) return 0;
    if (ln.header) return (uint32_t)kqtab::header_line_len(ln.name_len, ln.abs_pos);
    if (a.format == KQ_TABLE_KWIG) return (uint32_t)s_dig[l] + 3u;
    const TabWin w{a.triples, s_val, ln.first + ln.i, ln.i, ln.n_ctx, l};
    uint32_t sum = 0;
    for (int back = 0; back < a.k; ++back) {
        if (w.staged(back)) sum += s_dig[l - back];
        else if (w.known(back)) { const uint32_t* t = a.triples + (w.at - (uint64_t)back) * 3; sum += kqtab::fixed_digits(t[0], t[1], t[2]); }
        else sum += 3;
    }
    return (uint32_t)kqtab::expanded_line_len(ln.name_len, kqtab::digits_u64(ln.abs_pos + ln.i), sum, a.k);
}

__global__ __launch_bounds__(TAB_THREADS) void k_tab_len(TabArgs a, unsigned long long* __restrict__ tile_bytes) {
    __shared__ uint32_t s_val[TAB_LINES * 3];
    __shared__ uint8_t s_dig[TAB_LINES];
    const int tid = threadIdx.x;
    const uint64_t n_tiles = (a.n_lines + TAB_TILE - 1) / TAB_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const TabLine ln = tab_line(a, tile * TAB_TILE + (uint64_t)tid);
        tab_stage(a, ln, tid, s_val, s_dig);
        __syncthreads();
        const uint64_t total = block_sum(tab_len(a, ln, tid, s_val, s_dig));     // (ends with a barrier: the stage of the next tile may follow)
        if (tid == 0) tile_bytes[tile] = total;
    }
}

// the window of the output in LDS: byte `at` of the output lies at address base + at; the sink keeps [lo, hi)
struct TabSink {
    char* s_text; uint64_t win, lo, hi;       // addresses: the window's first byte, the kept range
    uint64_t base;
    __device__ __forceinline__ void put(uint64_t at, char c) { const uint64_t p = base + at; if (p >= lo && p < hi) s_text[p - win] = c; }
};

__device__ __forceinline__ void tab_put(const TabArgs& a, const TabLine& ln, int l, const uint32_t* s_val, uint64_t at, TabSink& sink) {
    if (ln.header) { kqtab::put_header_line(sink, at, ln.name, ln.name_len, ln.abs_pos); return; }
    if (a.format == KQ_TABLE_KWIG) { kqtab::put_fixed_line(sink, at, s_val[l * 3], s_val[l * 3 + 1], s_val[l * 3 + 2]); return; }
    const TabWin w{a.triples, s_val, ln.first + ln.i, ln.i, ln.n_ctx, l};
    const bool bed = a.format == KQ_TABLE_BED;
    kqtab::put_expanded_line(sink, at, ln.name, ln.name_len, ln.abs_pos + ln.i, a.k, bed ? '\t' : ',', bed ? ':' : ',', w);
}

// tile_off: the exclusive scan of k_tab_len's tile_bytes; total: the call's size (<= the room behind out, the host has checked)
__global__ __launch_bounds__(TAB_THREADS) void k_tab_write(TabArgs a, const unsigned long long* __restrict__ tile_off, uint64_t total, char* __restrict__ out) {
    __shared__ uint4 s_text4[TAB_WINDOW / 16];
    __shared__ uint32_t s_val[TAB_LINES * 3];
    __shared__ uint8_t s_dig[TAB_LINES];
    __shared__ uint32_t s_wave[TAB_THREADS / 64];
    __shared__ uint32_t s_extra[TAB_EXTRA];
    char* const s_text = (char*)s_text4;
    const int tid = threadIdx.x;
    const uint64_t n_tiles = (a.n_lines + TAB_TILE - 1) / TAB_TILE;
    const uint64_t base = (uint64_t)(uintptr_t)out, end = base + total;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t line0 = tile * TAB_TILE;
        const TabLine ln = tab_line(a, line0 + (uint64_t)tid);
        TabLine ex; ex.valid = false;                                      // threads 0 .. TAB_EXTRA-1: a line of the next tile
        if (tid < TAB_EXTRA) ex = tab_line(a, line0 + TAB_TILE + (uint64_t)tid);
        tab_stage(a, ln, tid, s_val, s_dig);
        if (tid < TAB_EXTRA) tab_stage(a, ex, TAB_TILE + tid, s_val, s_dig);
        __syncthreads();
        const uint32_t len = tab_len(a, ln, tid, s_val, s_dig);
        const uint32_t ex_len = tid < TAB_EXTRA ? tab_len(a, ex, TAB_TILE + tid, s_val, s_dig) : 0u;
        if (tid < TAB_EXTRA) s_extra[tid] = ex_len;
        uint32_t tile_total;
        const uint32_t rel = tab_block_scan(len, s_wave, &tile_total);     // (its barriers also publish s_extra)
        const uint64_t t_off = tile_off[tile], t_end = t_off + tile_total;
        const uint64_t at = t_off + rel;
        uint64_t ex_at = t_end;
        for (int j = 0; j < TAB_EXTRA; ++j) if (j < tid) ex_at += s_extra[j];
        // the addresses this tile stores: from the first 16-byte word that starts in its text to the end of the word that holds
        // its last byte, inside the output
        uint64_t own_lo = tile == 0 ? base : (base + t_off + 15) & ~15ull, own_hi = tile + 1 == n_tiles ? end : (base + t_end + 15) & ~15ull;
        if (own_hi > end) own_hi = end;
        if (own_lo > own_hi) own_lo = own_hi;
        for (uint64_t win = own_lo & ~15ull; win < own_hi; win += TAB_WINDOW) {
            const uint64_t lo = win > own_lo ? win : own_lo, hi = win + TAB_WINDOW < own_hi ? win + TAB_WINDOW : own_hi;
            TabSink sink{s_text, win, lo, hi, base};
#pragma unroll 1
            for (int r = 0; r < 2; ++r) {                                  // the thread's own line, then its line of the next tile (one copy of the writers)
                const TabLine& L = r ? ex : ln;
                const uint64_t l_at = r ? ex_at : at, l_len = r ? ex_len : len;
                if (L.valid && base + l_at < hi && base + l_at + l_len > lo) tab_put(a, L, r ? TAB_TILE + tid : tid, s_val, l_at, sink);
            }
            __syncthreads();
            for (uint32_t q = (uint32_t)tid; q * 16 < (uint32_t)(hi - win); q += TAB_THREADS) {
                const uint64_t p = win + (uint64_t)q * 16;
                if (p >= lo && p + 16 <= hi) *(uint4*)(uintptr_t)p = s_text4[q];
                else {                                                     // the output's first / last word only
#pragma unroll 1
                    for (int j = 0; j < 16; ++j) if (p + j >= lo && p + j < hi) ((char*)(uintptr_t)p)[j] = s_text[q * 16 + j];
                }
            }
            __syncthreads();
        }
    }
}

// ---- per-base entries -> oriented triples (the .bkwig payload) ----------------------------------------------------------
// out_start[s] = positions of the segments before s (n_segs + 1 values); position g of the output is entry
// seg_start[s] + g - out_start[s] of per_base.  One position per thread: a 16-byte load, three dword stores.
__global__ __launch_bounds__(256) void k_tab_triples(const kq_dbgbase* __restrict__ per_base, const unsigned long long* __restrict__ seg_start,
                                                      const unsigned long long* __restrict__ out_start, uint32_t n_segs, uint64_t n, uint32_t* __restrict__ triples) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_segs;
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (out_start[mid] <= g) lo = mid; else hi = mid; }
        const uint4 e = *(const uint4*)(per_base + seg_start[lo] + (g - out_start[lo]));      // fw, bw, cov, isFw | pad
        const bool fw = (e.w & 0xFFu) != 0;
        triples[g * 3] = e.z; triples[g * 3 + 1] = fw ? e.x : e.y; triples[g * 3 + 2] = fw ? e.y : e.x;
    }
}

// ---- per-base entries of one map-range pass -> the accumulated triples (kq_per_base_merge_dev) ---------------------------
// The lists are k_tab_triples'.  A position is evaluated in exactly one pass and k_lookup stores only found k-mers, so the
// passes' stored entries are disjoint: a stored entry (any of its 16 bytes set) overwrites its triple and is zeroed, a zero
// entry leaves the triple of an earlier pass alone, and per_base is all zero over the segments again when the kernel ends.
// One position per thread: a 16-byte load, and for a stored entry three dword stores and a 16-byte store.  per_base is read
// and written, hence neither const nor __restrict__; no entry and no triple belongs to two threads.
__global__ __launch_bounds__(256) void k_tab_merge(kq_dbgbase* per_base, const unsigned long long* __restrict__ seg_start,
                                                    const unsigned long long* __restrict__ out_start, uint32_t n_segs, uint64_t n, uint32_t* triples) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_segs;
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (out_start[mid] <= g) lo = mid; else hi = mid; }
        uint4* const p = (uint4*)(per_base + seg_start[lo] + (g - out_start[lo]));
        const uint4 e = *p;                                                                   // fw, bw, cov, isFw | pad
        if ((e.x | e.y | e.z | e.w) == 0) continue;
        const bool fw = (e.w & 0xFFu) != 0;
        triples[g * 3] = e.z; triples[g * 3 + 1] = fw ? e.x : e.y; triples[g * 3 + 2] = fw ? e.y : e.x;
        *p = make_uint4(0, 0, 0, 0);
    }
}

}  // namespace kq
