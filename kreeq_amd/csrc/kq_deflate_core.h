// kq_deflate_core.h -- the code builder of ONE BGZF member (RFC 1951 / 1952): from symbol frequencies to length-limited code
// lengths, canonical codes, the dynamic block header and the choice between a dynamic and a stored block.  Written once for
// the kernel k_bgzf_deflate (kq_deflate.h) and for a plain host program (tests/native/deflate_core_main.cpp).
// No HIP or project header besides kq_inflate_core.h (the CRC-32): g++ reads this file as it is.
//
// The builder does not own memory.  Everything it touches lies in one `Work` record the caller places (heap on the host, LDS in
// the kernel, where one lane runs the builder), and every output byte goes through a sink policy `S`:
//   bool put(uint32_t pos, uint32_t byte)        member byte pos; false = no room (the writer then reports ERR_SINK)
// Who finds the matches is the caller's business: it counts its tokens into Work::lfreq / dfreq (count_literal / count_match,
// or atomics on the same arrays), calls plan_block(), and then emits the header items and the tokens' bits (token_bits) in order.
//
// Code lengths.  The used symbols are sorted by (frequency, symbol) with a heap sort, a Huffman tree is built by the two-queue
// merge (leaves in sorted order, internal nodes in creation order: both queues are ascending), and depths above the limit are
// repaired the way zlib's gen_bitlen does: every leaf deeper than `max` is put at `max`, and while the Kraft sum K (in units
// of 2^-max) exceeds 1, the deepest leaf above level max becomes an internal node over itself and one leaf taken from level
// max: counts[b]--, counts[b + 1] += 2, counts[max]--, which lowers K by exactly one unit and keeps the number of leaves.  The
// loop therefore ends at K = 1 after at most as many rounds as leaves were clamped (<= 286).  Lengths are then handed out by
// frequency: the rarest symbols get the longest codes.  A set whose sum cannot be brought to 1 is an error (ERR_KRAFT); the
// caller falls back to a stored block.
// Sets with fewer than two used symbols: the literal set and the code-length code get a second, unused code of one bit (both
// are then complete, as zlib's inflate demands for the code-length code); the distance set keeps ONE code of one bit: for its
// only symbol, or, without any match, for symbol 0, which is never used -- the incomplete set every inflater accepts.
//
// Bounds.  Frequencies must sum to less than 2^23 (a member holds at most 65 281 symbols): a sort key is freq << 9 | symbol.
// Every loop runs over a fixed range (<= 286 symbols, <= 316 lengths, <= 336 header items) or ends by a counter that only falls.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "kq_inflate_core.h"

#if defined(__HIPCC__)
#define KQ_DEF_HD __host__ __device__
#else
#define KQ_DEF_HD
#endif

namespace kqdef {

enum Err : int {
    OK = 0,
    ERR_KRAFT = 1,      // a code-length set could not be made complete
    ERR_FREQ = 2,       // frequencies of 2^23 or more
    ERR_SINK = 3,       // the output had no room for a byte
    ERR_BOUND = 4,      // (set by the callers: an index or a size left its bound)
    ERR_N = 5
};
KQ_DEF_HD inline const char* err_name(int e) {
    switch (e) {
        case OK: return "ok";
        case ERR_KRAFT: return "incomplete code lengths";
        case ERR_FREQ: return "symbol frequencies too large";
        case ERR_SINK: return "no room in the member";
        case ERR_BOUND: return "a bound was violated";
        default: return "unknown error";
    }
}

constexpr int N_LIT = 286, N_DIST = 30, N_CLEN = 19, MAX_BITS = 15, MAX_CLEN_BITS = 7, EOB = 256;
constexpr uint32_t MIN_MATCH = 3, MAX_MATCH = 258, WINDOW = 32768;
constexpr uint32_t MEMBER_TEXT = 0xff00;                          // text bytes per member (bgzip's choice)
constexpr uint32_t HEADER_BYTES = 18, TRAILER_BYTES = 8, STORED_BYTES = 5;
constexpr uint32_t MEMBER_MAX = HEADER_BYTES + STORED_BYTES + MEMBER_TEXT + TRAILER_BYTES;      // 65 311: BSIZE always fits
constexpr uint32_t MAX_ITEMS = 1 + N_CLEN + N_LIT + N_DIST;       // header items: the counts, 19 x 3 bits, one per run-length token
constexpr uint32_t EOF_BYTES = 28;

// ---- symbols of lengths and distances -------------------------------------------------------------------------------------
KQ_DEF_HD inline uint32_t log2u(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }      // v > 0
// len 3..258 -> symbol 0..28 (code 257 + symbol), the number of extra bits and their value
KQ_DEF_HD inline void len_sym(uint32_t len, uint32_t& sym, uint32_t& nb, uint32_t& extra) {
    const uint32_t l = len - MIN_MATCH;
    if (len >= MAX_MATCH) { sym = 28; nb = 0; extra = 0; return; }
    if (l < 8) { sym = l; nb = 0; extra = 0; return; }
    nb = log2u(l) - 2u;
    sym = 4u * (nb + 1u) + ((l >> nb) & 3u);
    extra = l & ((1u << nb) - 1u);
}
// dist 1..32768 -> symbol 0..29
KQ_DEF_HD inline void dist_sym(uint32_t dist, uint32_t& sym, uint32_t& nb, uint32_t& extra) {
    const uint32_t d = dist - 1u;
    if (d < 4) { sym = d; nb = 0; extra = 0; return; }
    const uint32_t b = log2u(d);
    nb = b - 1u;
    sym = 2u * b + ((d >> nb) & 1u);
    extra = d & ((1u << nb) - 1u);
}
KQ_DEF_HD inline uint32_t len_extra_bits(uint32_t sym) { return sym < 8 || sym >= 28 ? 0u : (sym >> 2) - 1u; }
KQ_DEF_HD inline uint32_t dist_extra_bits(uint32_t sym) { return sym < 4 ? 0u : (sym >> 1) - 1u; }

struct Work {
    uint32_t lfreq[N_LIT], dfreq[N_DIST], cfreq[N_CLEN];         // the caller counts into the first two
    uint8_t llen[N_LIT], dlen[N_DIST], clen[N_CLEN];
    uint16_t lcode[N_LIT], dcode[N_DIST], ccode[N_CLEN];         // bit-reversed: ready for the LSB-first writer
    uint16_t rle[N_LIT + N_DIST];                                // the lengths' run-length tokens: symbol | extra << 8
    uint32_t hlit, hdist, hclen, n_rle, n_items;
    union {
        struct { uint32_t key[N_LIT], ifreq[N_LIT]; uint16_t lpar[N_LIT], ipar[N_LIT]; uint8_t idep[N_LIT]; } b;      // build_lengths
        uint32_t items[MAX_ITEMS];                               // the dynamic header: bits | n_bits << 24, in order
    } u;
};

struct Plan {
    int err = OK;
    bool dynamic = false;            // false: one stored block
    uint32_t hdr_bits = 0;           // of the dynamic header (the items)
    uint32_t dyn_bits = 0;           // header + tokens + end-of-block
    uint32_t payload = 0;            // bytes of DEFLATE data of the chosen form
};

KQ_DEF_HD inline void clear_freq(Work& w) {
    for (int s = 0; s < N_LIT; ++s) w.lfreq[s] = 0;
    for (int s = 0; s < N_DIST; ++s) w.dfreq[s] = 0;
}
KQ_DEF_HD inline void count_literal(Work& w, uint32_t b) { ++w.lfreq[b & 0xFFu]; }
KQ_DEF_HD inline void count_match(Work& w, uint32_t len, uint32_t dist) {
    uint32_t s, nb, e;
    len_sym(len, s, nb, e); ++w.lfreq[257u + s];
    dist_sym(dist, s, nb, e); ++w.dfreq[s];
}

// key[root] sinks inside the max-heap key[0, lim): at most log2(286) + 1 levels
KQ_DEF_HD inline void sift_down(uint32_t* key, int root, int lim) {
    const uint32_t v = key[root];
    int i = root;
    for (;;) {
        int c = 2 * i + 1;
        if (c >= lim) break;
        if (c + 1 < lim && key[c + 1] > key[c]) ++c;
        if (key[c] <= v) break;
        key[i] = key[c];
        i = c;
    }
    key[i] = v;
}

// ---- length-limited code lengths --------------------------------------------------------------------------------------------
// n <= 286 symbols, max <= 15; min_codes: 2 = a set with fewer than two used symbols gets an unused second code (see above).
KQ_DEF_HD inline int build_lengths(Work& w, const uint32_t* freq, int n, int max, int min_codes, uint8_t* lens) {
    uint32_t* key = w.u.b.key;
    uint32_t* ifreq = w.u.b.ifreq;
    uint16_t* lpar = w.u.b.lpar;
    uint16_t* ipar = w.u.b.ipar;
    uint8_t* idep = w.u.b.idep;
    int used = 0;
    uint32_t sum = 0;
    for (int s = 0; s < n; ++s) {
        lens[s] = 0;
        if (!freq[s]) continue;
        if (freq[s] >= (1u << 23) || (sum += freq[s]) >= (1u << 23)) return ERR_FREQ;
        key[used++] = freq[s] << 9 | (uint32_t)s;
    }
    if (used < 2) {
        const int s = used ? (int)(key[0] & 511u) : 0;
        lens[s] = 1;
        if (min_codes >= 2) lens[s ? 0 : 1] = 1;
        return OK;
    }
    for (int start = used / 2 - 1; start >= 0; --start) sift_down(key, start, used);      // heap sort, ascending
    for (int end = used - 1; end > 0; --end) { const uint32_t t = key[0]; key[0] = key[end]; key[end] = t; sift_down(key, 0, end); }
    // two-queue merge: used - 1 internal nodes, the last one is the root
    int li = 0, ii = 0, ni = 0;
    while (ni < used - 1) {
        uint32_t f = 0;
        for (int t = 0; t < 2; ++t) {
            if (li < used && (ii >= ni || (key[li] >> 9) <= ifreq[ii])) { f += key[li] >> 9; lpar[li++] = (uint16_t)ni; }
            else { f += ifreq[ii]; ipar[ii++] = (uint16_t)ni; }      // (ii < ni: two nodes are always left while ni < used - 1)
        }
        ifreq[ni++] = f;
    }
    idep[ni - 1] = 0;
    for (int i = ni - 2; i >= 0; --i) { const uint32_t d = idep[ipar[i]] + 1u; idep[i] = (uint8_t)(d > 255u ? 255u : d); }
    uint32_t count[MAX_BITS + 1];
    for (int l = 0; l <= MAX_BITS; ++l) count[l] = 0;
    for (int i = 0; i < used; ++i) { uint32_t d = idep[lpar[i]] + 1u; if (d > (uint32_t)max) d = (uint32_t)max; ++count[d]; }
    uint32_t kraft = 0;
    const uint32_t one = 1u << max;
    for (int l = 1; l <= max; ++l) kraft += count[l] << (max - l);
    for (int round = 0; kraft > one; ++round) {
        int b = max - 1;
        while (b > 0 && !count[b]) --b;
        if (b == 0 || !count[max] || round > N_LIT) return ERR_KRAFT;
        --count[b]; count[b + 1] += 2; --count[max];
        --kraft;
    }
    if (kraft != one) return ERR_KRAFT;
    int idx = 0;
    for (int l = max; l >= 1; --l)
        for (uint32_t c = 0; c < count[l] && idx < used; ++c) lens[key[idx++] & 511u] = (uint8_t)l;
    return idx == used ? OK : ERR_KRAFT;
}

// canonical codes of n lengths, bit-reversed
KQ_DEF_HD inline void build_codes(const uint8_t* lens, int n, uint16_t* codes) {
    uint32_t count[MAX_BITS + 1], next[MAX_BITS + 2];
    for (int l = 0; l <= MAX_BITS; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[lens[s] & 15u];
    count[0] = 0;
    uint32_t code = 0;
    for (int l = 1; l <= MAX_BITS; ++l) { code = (code + count[l - 1]) << 1; next[l] = code; }
    for (int s = 0; s < n; ++s) {
        const uint32_t l = lens[s] & 15u;
        uint32_t c = l ? next[l]++ : 0u, r = 0;
        for (uint32_t i = 0; i < l; ++i) { r = r << 1 | (c & 1u); c >>= 1; }
        codes[s] = (uint16_t)r;
    }
}

// Kraft sum of a set in units of 2^-15 (32768 = complete); the tests check every emitted set with it
KQ_DEF_HD inline uint32_t kraft_sum(const uint8_t* lens, int n) {
    uint32_t k = 0;
    for (int s = 0; s < n; ++s) if (lens[s]) k += 1u << (MAX_BITS - (lens[s] & 15u));
    return k;
}

KQ_DEF_HD inline uint32_t item(uint32_t bits, uint32_t n) { return bits | n << 24; }

// From the counted frequencies (the end-of-block code is added here) to lengths, codes, the header items and the block choice
// for a member of n_text bytes.
KQ_DEF_HD inline Plan plan_block(Work& w, uint32_t n_text) {
    Plan p;
    const uint32_t stored = STORED_BYTES + n_text;
    p.payload = stored;
    w.lfreq[EOB] = 1;
    int rc = build_lengths(w, w.lfreq, N_LIT, MAX_BITS, 2, w.llen);
    if (!rc) rc = build_lengths(w, w.dfreq, N_DIST, MAX_BITS, 1, w.dlen);
    if (rc) { p.err = rc; return p; }
    build_codes(w.llen, N_LIT, w.lcode);
    build_codes(w.dlen, N_DIST, w.dcode);
    uint32_t hlit = N_LIT, hdist = N_DIST;
    while (hlit > 257 && !w.llen[hlit - 1]) --hlit;
    while (hdist > 1 && !w.dlen[hdist - 1]) --hdist;
    // run-length tokens over the hlit + hdist lengths as one sequence (a run may cross from one set into the other)
    const uint32_t total = hlit + hdist;
    for (int s = 0; s < N_CLEN; ++s) w.cfreq[s] = 0;
    uint32_t n_rle = 0;
    for (uint32_t i = 0; i < total;) {
        const uint32_t v = i < hlit ? w.llen[i] : w.dlen[i - hlit];
        uint32_t run = 1;
        while (i + run < total && (i + run < hlit ? w.llen[i + run] : w.dlen[i + run - hlit]) == v) ++run;
        i += run;
        if (v) { w.rle[n_rle++] = (uint16_t)v; ++w.cfreq[v]; --run; }      // the length itself, then repeats of it
        while (run) {                                                      // every round takes at least one length of the run
            uint32_t sym, take, extra;
            if (!v && run >= 11) { take = run < 138 ? run : 138; sym = 18; extra = take - 11; }
            else if (!v && run >= 3) { take = run; sym = 17; extra = take - 3; }
            else if (v && run >= 3) { take = run < 6 ? run : 6; sym = 16; extra = take - 3; }
            else { take = 1; sym = v; extra = 0; }
            w.rle[n_rle++] = (uint16_t)(sym | extra << 8);
            ++w.cfreq[sym];
            run -= take;
        }
    }
    rc = build_lengths(w, w.cfreq, N_CLEN, MAX_CLEN_BITS, 2, w.clen);
    if (rc) { p.err = rc; return p; }
    build_codes(w.clen, N_CLEN, w.ccode);
    const uint8_t order[N_CLEN] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hclen = N_CLEN;
    while (hclen > 4 && !w.clen[order[hclen - 1]]) --hclen;
    w.hlit = hlit; w.hdist = hdist; w.hclen = hclen; w.n_rle = n_rle;
    // the token costs first (build_lengths above was the last user of the union's other half; the items go there now)
    uint32_t bits = 0;
    for (uint32_t s = 0; s < (uint32_t)N_LIT; ++s) bits += w.lfreq[s] * (w.llen[s] + (s > 256 ? len_extra_bits(s - 257u) : 0u));
    for (uint32_t s = 0; s < (uint32_t)N_DIST; ++s) bits += w.dfreq[s] * (w.dlen[s] + dist_extra_bits(s));
    uint32_t n_items = 0, hdr = 0;
    w.u.items[n_items++] = item(1u | 2u << 1 | (hlit - 257u) << 3 | (hdist - 1u) << 8 | (hclen - 4u) << 13, 17);      // BFINAL, BTYPE = 2, the counts
    hdr += 17;
    for (uint32_t i = 0; i < hclen; ++i) { w.u.items[n_items++] = item(w.clen[order[i]], 3); hdr += 3; }
    for (uint32_t i = 0; i < n_rle; ++i) {
        const uint32_t sym = w.rle[i] & 0xFFu, extra = w.rle[i] >> 8, l = w.clen[sym];
        const uint32_t eb = sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u;
        w.u.items[n_items++] = item(w.ccode[sym] | extra << l, l + eb);
        hdr += l + eb;
    }
    w.n_items = n_items;
    p.hdr_bits = hdr;
    p.dyn_bits = hdr + bits;
    const uint32_t dyn_bytes = (p.dyn_bits + 7u) / 8u;
    p.dynamic = dyn_bytes < stored;
    if (p.dynamic) p.payload = dyn_bytes;
    return p;
}

// the bits of one token, LSB first: at most 15 + 5 + 15 + 13 = 48
KQ_DEF_HD inline void literal_bits(const Work& w, uint32_t b, uint64_t& bits, uint32_t& n) { bits = w.lcode[b]; n = w.llen[b]; }
KQ_DEF_HD inline void match_bits(const Work& w, uint32_t len, uint32_t dist, uint64_t& bits, uint32_t& n) {
    uint32_t s, nb, e;
    len_sym(len, s, nb, e);
    bits = w.lcode[257u + s]; n = w.llen[257u + s];
    bits |= (uint64_t)e << n; n += nb;
    dist_sym(dist, s, nb, e);
    bits |= (uint64_t)w.dcode[s] << n; n += w.dlen[s];
    bits |= (uint64_t)e << n; n += nb;
}

// ---- the container ------------------------------------------------------------------------------------------------------------
// byte i < 18 of the BGZF header of a member of `size` bytes in all
KQ_DEF_HD inline uint32_t header_byte(uint32_t i, uint32_t size) {
    switch (i) {
        case 0: return 0x1f; case 1: return 0x8b; case 2: return 8; case 3: return 4;       // ID1 ID2 CM FLG = FEXTRA
        case 9: return 0xff;                                                                 // OS unknown (MTIME, XFL = 0)
        case 10: return 6;                                                                   // XLEN = 6
        case 12: return 'B'; case 13: return 'C'; case 14: return 2;                         // SI1 SI2 SLEN = 2
        case 16: return (size - 1u) & 0xFFu; case 17: return ((size - 1u) >> 8) & 0xFFu;    // BSIZE = size - 1
        default: return 0;
    }
}
// byte i < 8 of the trailer
KQ_DEF_HD inline uint32_t trailer_byte(uint32_t i, uint32_t crc, uint32_t isize) { return ((i < 4 ? crc : isize) >> (8u * (i & 3u))) & 0xFFu; }
// byte i < 5 of the stored block's header: BFINAL = 1, BTYPE = 0, LEN, ~LEN
KQ_DEF_HD inline uint32_t stored_byte(uint32_t i, uint32_t n) { return i == 0 ? 1u : ((i < 3 ? n : ~n) >> (8u * ((i - 1u) & 1u))) & 0xFFu; }
// byte i < 28 of the end-of-file marker: an empty member (a fixed block that holds only the end-of-block code)
KQ_DEF_HD inline uint32_t eof_byte(uint32_t i) { return i < HEADER_BYTES ? header_byte(i, EOF_BYTES) : i == 18 ? 3u : 0u; }

// LSB-first bit writer into a sink, from byte `pos` on
template <class S>
struct BitWriter {
    S& s;
    uint32_t pos;
    uint64_t acc = 0;
    uint32_t n = 0;
    int err = OK;
    KQ_DEF_HD BitWriter(S& s_, uint32_t pos_) : s(s_), pos(pos_) {}
    KQ_DEF_HD void put(uint64_t bits, uint32_t nb) {               // nb <= 48
        acc |= bits << n;
        n += nb;
        while (n >= 8) { if (!s.put(pos, (uint32_t)acc & 0xFFu)) err = ERR_SINK; ++pos; acc >>= 8; n -= 8; }
    }
    KQ_DEF_HD void finish() { if (n) { if (!s.put(pos, (uint32_t)acc & 0xFFu)) err = ERR_SINK; ++pos; acc = 0; n = 0; } }
};

}  // namespace kqdef
