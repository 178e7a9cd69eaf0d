// kq_table_core.h -- the LINE RULES of the per-base tables (reference src/kreeq-output.cpp:176-219, :275-281 and
// src/decompressor.cpp:510-579), written once for the kernels of kq_table.h, for the host formatter of
// `kreeq-decompressor lookup` and for a plain host program (tests/native/table_core_main.cpp).  No HIP or project header:
// g++ reads this file as it is.
//
// A line is made from oriented u32 triples (cov, fw, bw) -- the payload of a .bkwig -- in one of two layouts:
//   fixedStep  "c,f,b\n" per position, under "fixedStep chrom=<name> start=<abs_pos> step=1\n" header lines (.kwig, inflate,
//              lookup);
//   expanded   "<name><col><coordinate><col>W(cov)<col>W(fw)<col>W(bw)\n" per position, W(x) = the k most recent values of a
//              column, oldest first, joined by <ent> (.bed: col '\t', ent ':'; .csvtable and inflate --expand: both ',').
// Every number is plain decimal (std::to_string of an unsigned value).  A line's LENGTH is a function of digit counts only, so
// a first pass can place every line before a second pass writes it; the writers put every byte through a SINK
//     void put(uint64_t at, char c)
// at its absolute position `at` in the output, so the same code fills a host buffer or the window of the output that a
// workgroup holds in LDS (a sink is free to drop the positions outside its window).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KQ_TAB_HD __host__ __device__
#else
#define KQ_TAB_HD
#endif

namespace kqtab {

KQ_TAB_HD inline int digits_u32(uint32_t v) {                              // 1 .. 10
    return v < 100000u ? (v < 100u ? (v < 10u ? 1 : 2) : (v < 1000u ? 3 : (v < 10000u ? 4 : 5)))
                       : (v < 10000000u ? (v < 1000000u ? 6 : 7) : (v < 100000000u ? 8 : (v < 1000000000u ? 9 : 10)));
}
KQ_TAB_HD inline int digits_u64(uint64_t v) {                              // 1 .. 20
    if (v <= 0xFFFFFFFFull) return digits_u32((uint32_t)v);
    int d = 10;                                                            // v >= 2^32 > 10^9: at least 10 digits
    for (uint64_t p = 10000000000ull; d < 20 && v >= p; p *= 10) ++d;      // (d == 19: p = 10^19 < 2^64, no overflow before the test)
    return d;
}
// the nd = digits(v) decimal digits of v at [at, at + nd)
template <class Sink> KQ_TAB_HD inline void put_u32(Sink& s, uint64_t at, uint32_t v, int nd) {
    for (int i = nd - 1; i >= 0; --i) { s.put(at + (uint64_t)i, (char)('0' + v % 10u)); v /= 10u; }
}
template <class Sink> KQ_TAB_HD inline void put_u64(Sink& s, uint64_t at, uint64_t v, int nd) {
    int i = nd - 1;
    for (; v > 0xFFFFFFFFull; --i) { s.put(at + (uint64_t)i, (char)('0' + (int)(v % 10u))); v /= 10u; }
    put_u32(s, at, (uint32_t)v, i + 1);
}
template <class Sink> KQ_TAB_HD inline void put_text(Sink& s, uint64_t at, const char* t, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) s.put(at + i, t[i]);
}

// ---- fixedStep layout --------------------------------------------------------------------------------------------------
constexpr uint32_t HEADER_FIXED = 16 + 7 + 8;                               // "fixedStep chrom=" + " start=" + " step=1\n"
KQ_TAB_HD inline uint64_t header_line_len(uint32_t name_len, uint64_t abs_pos) { return (uint64_t)HEADER_FIXED + name_len + (uint64_t)digits_u64(abs_pos); }
KQ_TAB_HD inline uint32_t fixed_digits(uint32_t c, uint32_t f, uint32_t b) { return (uint32_t)(digits_u32(c) + digits_u32(f) + digits_u32(b)); }
KQ_TAB_HD inline uint64_t fixed_line_len(uint32_t c, uint32_t f, uint32_t b) { return (uint64_t)fixed_digits(c, f, b) + 3; }
template <class Sink> KQ_TAB_HD inline uint64_t put_header_line(Sink& s, uint64_t at, const char* name, uint32_t name_len, uint64_t abs_pos) {
    const char a[] = "fixedStep chrom=", b[] = " start=", c[] = " step=1\n";
    put_text(s, at, a, 16); at += 16;
    put_text(s, at, name, name_len); at += name_len;
    put_text(s, at, b, 7); at += 7;
    const int nd = digits_u64(abs_pos);
    put_u64(s, at, abs_pos, nd); at += (uint64_t)nd;
    put_text(s, at, c, 8);
    return at + 8;
}
template <class Sink> KQ_TAB_HD inline uint64_t put_fixed_line(Sink& s, uint64_t at, uint32_t c, uint32_t f, uint32_t b) {
    const uint32_t v[3] = {c, f, b};
    for (int j = 0; j < 3; ++j) {
        const int nd = digits_u32(v[j]);
        put_u32(s, at, v[j], nd); at += (uint64_t)nd;
        s.put(at++, j < 2 ? ',' : '\n');
    }
    return at;
}

// ---- expanded layout ---------------------------------------------------------------------------------------------------
// window_digits = the digits of all 3 k window values of the line (a position that reads as 0 counts 1 per column); the rest
// of the line: the name, the coordinate, 3 (k - 1) entry separators, 3 column separators and the '\n' take the place of ... :
//   name <col> coord <col> [k values, k - 1 <ent>] <col> [..] <col> [..] '\n'  =  name + coord + 4 col + 3 (k - 1) ent + 1
KQ_TAB_HD inline uint64_t expanded_line_len(uint32_t name_len, int coord_digits, uint32_t window_digits, int k) {
    return (uint64_t)name_len + (uint64_t)coord_digits + (uint64_t)window_digits + 3ull * (uint64_t)(k - 1) + 5ull;
}
// win(back, column): the value `back` positions before the line's own (0 <= back < k; 0 = the line's position), 0 where the
// window reads before its history
template <class Sink, class Win>
KQ_TAB_HD inline uint64_t put_expanded_line(Sink& s, uint64_t at, const char* name, uint32_t name_len, uint64_t coord, int k, char col, char ent, const Win& win) {
    put_text(s, at, name, name_len); at += name_len;
    s.put(at++, col);
    const int cd = digits_u64(coord);
    put_u64(s, at, coord, cd); at += (uint64_t)cd;
    for (int column = 0; column < 3; ++column) {
        s.put(at++, col);
        for (int back = k - 1; back >= 0; --back) {
            const uint32_t v = win(back, column);
            const int nd = digits_u32(v);
            put_u32(s, at, v, nd); at += (uint64_t)nd;
            if (back) s.put(at++, ent);
        }
    }
    s.put(at++, '\n');
    return at;
}

}  // namespace kqtab
