// kq_inflate_core.h -- ONE raw DEFLATE stream (RFC 1951) with known input and output sizes, which is what a BGZF member holds:
// written once for the kernel k_bgzf_inflate (kq_bgzf.h) and for a plain host program (tests/native/inflate_core_main.cpp).
// No HIP or project header: g++ reads this file as it is.
//
// The decoder does not own memory.  `M` gives it the input, the output window and the tables:
//   uint32_t in_byte(uint32_t i)                 compressed byte i; the core calls it only with i < data_len
//   void     out_put(uint32_t pos, uint32_t b)   text byte pos;     the core calls it only with pos < isize
//   void     out_copy(uint32_t pos, uint32_t dist, uint32_t len)    text[pos + j] = text[pos - dist + j], j = 0 .. len - 1, in that
//                                                order (dist < len repeats the last dist bytes); the core has checked
//                                                1 <= dist <= pos and pos + len <= isize
//   Tables*  tables()                            the decode tables (below)
//   void     st16(uint16_t* p, uint32_t v), st8(uint8_t* p, uint32_t v)      a store into the tables
//   void     tables_ready()                      called after a block's tables were written, before they are read
// The host program runs it on heap arrays of exactly data_len, isize and sizeof(Tables) bytes; the kernel on LDS, where every lane
// of the wave runs this same code on the same values and the stores are made by one lane.
//
// Codes are canonical Huffman codes, decoded from the per-length counts and the symbols sorted by (length, symbol): for each length
// L = 1..15, `first` is the first code of that length and `index` the number of shorter codes; a code of length L is
// first <= code < first + count[L], its symbol is symbol[index + code - first].
//
// Bounds.  The bit reader holds up to 64 bits; it takes byte `in_pos` only after in_pos < data_len, and a decode step uses n bits only
// after n <= the bits it holds: otherwise the stream ended early (ERR_INPUT_END).  Every output goes through out_room(), which checks
// pos + n <= isize first (ERR_OUTPUT).  Table indices: a symbol index is index + (code - first) < index + count[L] <= the number of
// symbols of the set; lengths are 1..15 by construction; length / distance symbols index their 29 / 30 entry tables after the checks
// sym <= 285 and sym <= 29.  Every loop iteration consumes at least one input bit or writes at least one output byte, except the
// table builders, which run over fixed ranges (19, <= 320, 15 entries).  A violated bound or an invalid stream ends the stream with
// an error code; nothing is read or written outside the three arrays and nothing loops without progress.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
// inlined into the kernel: the decoder's state then lives in registers, not behind a `this` pointer in scratch memory
#define KQ_INF_HD __host__ __device__ __attribute__((always_inline))
#else
#define KQ_INF_HD
#endif

namespace kqinf {

enum Err : int {
    OK = 0,
    ERR_BTYPE = 1,           // reserved block type 3
    ERR_STORED_LEN = 2,      // stored block: LEN != ~NLEN
    ERR_HEADER_COUNTS = 3,   // HLIT > 286 or HDIST > 30
    ERR_OVERSUBSCRIBED = 4,  // a code-length set with more codes than its lengths allow
    ERR_INCOMPLETE = 5,      // an incomplete set (other than the single distance code zlib accepts), or no end-of-block code
    ERR_REPEAT = 6,          // code-length repeat with nothing before it, or one that runs past HLIT + HDIST
    ERR_SYMBOL = 7,          // length symbol 286 / 287, or a code no symbol has
    ERR_DIST_CODE = 8,       // distance code 30 / 31
    ERR_DISTANCE = 9,        // distance beyond the bytes written so far
    ERR_INPUT_END = 10,      // the input ended before the final block's end-of-block code
    ERR_OUTPUT = 11,         // more output than isize, or not isize bytes at the end of the final block
    ERR_TRAILING = 12,       // whole bytes of input left behind the final block
    ERR_CRC = 13,            // (set by the callers: the text's CRC-32 differs from the member's)
    ERR_N = 14
};
KQ_INF_HD inline const char* err_name(int e) {
    switch (e) {
        case OK: return "ok";
        case ERR_BTYPE: return "reserved block type";
        case ERR_STORED_LEN: return "stored block length mismatch";
        case ERR_HEADER_COUNTS: return "too many length or distance codes";
        case ERR_OVERSUBSCRIBED: return "over-subscribed code lengths";
        case ERR_INCOMPLETE: return "incomplete code lengths";
        case ERR_REPEAT: return "invalid code length repeat";
        case ERR_SYMBOL: return "invalid literal/length code";
        case ERR_DIST_CODE: return "invalid distance code";
        case ERR_DISTANCE: return "distance too far back";
        case ERR_INPUT_END: return "compressed data ends early";
        case ERR_OUTPUT: return "uncompressed size differs from ISIZE";
        case ERR_TRAILING: return "data behind the final block";
        case ERR_CRC: return "CRC-32 mismatch";
        default: return "unknown error";
    }
}

constexpr int MAX_BITS = 15, N_LIT = 288, N_DIST = 32, N_CLEN = 19;

struct Tables {
    uint16_t lcount[MAX_BITS + 1], lsym[N_LIT];       // literal / length code
    uint16_t dcount[MAX_BITS + 1], dsym[N_DIST];      // distance code
    uint16_t offs[MAX_BITS + 1];                      // scratch of build()
    uint8_t lens[N_CLEN + N_LIT + N_DIST + 1];        // code lengths as read: the 19 of the code-length code, then HLIT + HDIST <= 316
};

// ---- CRC-32 (IEEE, reflected polynomial 0xEDB88320) and its combination over concatenation ------------------------------------
constexpr uint32_t CRC_POLY = 0xEDB88320u;
KQ_INF_HD inline uint32_t crc_byte(uint32_t reg, uint32_t b) {      // reg: the running register (crc ^ 0xFFFFFFFF)
    reg ^= b;
    for (int i = 0; i < 8; ++i) reg = (reg >> 1) ^ (CRC_POLY & (0u - (reg & 1u)));
    return reg;
}
// a(x) b(x) mod P in the reflected representation (x^0 = bit 31); 32 steps
KQ_INF_HD inline uint32_t gf2_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
// x^(8 n) mod P: square and multiply, at most 32 rounds
KQ_INF_HD inline uint32_t gf2_xpow8(uint32_t n) {
    uint32_t r = 0x80000000u, base = 0x00800000u;     // x^0, x^8
    for (int i = 0; i < 32 && n; ++i, n >>= 1) {
        if (n & 1u) r = gf2_mul(r, base);
        base = gf2_mul(base, base);
    }
    return r;
}
// crc(A || B) from crc(A), crc(B) and |B|
KQ_INF_HD inline uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint32_t len_b) { return gf2_mul(gf2_xpow8(len_b), crc_a) ^ crc_b; }

// ---- the decoder --------------------------------------------------------------------------------------------------------------
template <class M>
struct Inflate {
    M& m;
    uint32_t data_len, isize;
    uint64_t bits = 0;           // bit buffer, next bit = bit 0
    uint32_t n_bits = 0;         // bits held
    uint32_t in_pos = 0;         // next input byte to take
    uint32_t out_pos = 0;
    int max_len = 0;             // longest code length of any set built (the host program reports it)

    KQ_INF_HD Inflate(M& m_, uint32_t data_len_, uint32_t isize_) : m(m_), data_len(data_len_), isize(isize_) {}

    // fill the buffer to more than 56 bits, or with all the input that is left
    KQ_INF_HD void refill() {
        while (n_bits <= 56 && in_pos < data_len) {
            bits |= (uint64_t)(m.in_byte(in_pos) & 0xFFu) << n_bits;
            ++in_pos;
            n_bits += 8;
        }
    }
    // n <= 16 bits into v; false: the input ended
    KQ_INF_HD bool take(uint32_t n, uint32_t& v) {
        if (n_bits < n) { refill(); if (n_bits < n) return false; }
        v = (uint32_t)bits & ((1u << n) - 1u);
        bits >>= n;
        n_bits -= n;
        return true;
    }
    KQ_INF_HD bool out_room(uint32_t n) const { return n <= isize - out_pos; }      // (out_pos <= isize always)

    // counts and sorted symbols of n code lengths -> OK, ERR_OVERSUBSCRIBED, or ERR_INCOMPLETE (the set is still built: the
    // caller decides whether an incomplete one is acceptable)
    KQ_INF_HD int build(uint16_t* count, uint16_t* sym, const uint8_t* lens, uint32_t n) {
        Tables* t = m.tables();
        for (int l = 0; l <= MAX_BITS; ++l) m.st16(&count[l], 0);
        m.tables_ready();
        for (uint32_t s = 0; s < n; ++s) { const uint32_t l = lens[s] & 15u; m.st16(&count[l], count[l] + 1u); m.tables_ready(); }
        if (count[0] == n) return ERR_INCOMPLETE;                  // no code at all
        int left = 1;
        for (int l = 1; l <= MAX_BITS; ++l) {
            left <<= 1;
            left -= (int)count[l];
            if (left < 0) return ERR_OVERSUBSCRIBED;
            if (count[l] && l > max_len) max_len = l;
        }
        m.st16(&t->offs[1], 0);
        m.tables_ready();
        for (int l = 1; l < MAX_BITS; ++l) { m.st16(&t->offs[l + 1], t->offs[l] + count[l]); m.tables_ready(); }
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t l = lens[s] & 15u;
            if (!l) continue;
            const uint32_t o = t->offs[l];                         // < the number of coded symbols <= n
            if (o >= n) return ERR_OVERSUBSCRIBED;                 // (cannot happen: the counts were made from the same lengths)
            m.st16(&sym[o], s);
            m.st16(&t->offs[l], o + 1u);
            m.tables_ready();
        }
        return left > 0 ? ERR_INCOMPLETE : OK;
    }

    // one symbol of the code (count, sym) of n_sym coded symbols -> symbol, or -ERR_*
    KQ_INF_HD int decode(const uint16_t* count, const uint16_t* sym) {
        if (n_bits < (uint32_t)MAX_BITS) refill();
        uint32_t code = 0, first = 0, index = 0;
        uint64_t b = bits;
        for (uint32_t l = 1; l <= (uint32_t)MAX_BITS; ++l) {
            if (l > n_bits) return -ERR_INPUT_END;
            code |= (uint32_t)b & 1u;
            b >>= 1;
            const uint32_t c = count[l];
            if (code - first < c) {                                // (code >= first: both grow by the same rule)
                bits >>= l;
                n_bits -= l;
                return sym[index + (code - first)];                // index + c <= coded symbols of the set
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        return -ERR_SYMBOL;                                        // a code of an incomplete set that no symbol has
    }

    KQ_INF_HD int stored() {
        uint32_t v, len, nlen;
        if (!take(n_bits & 7u, v)) return ERR_INPUT_END;           // to the byte boundary (the buffer holds whole bytes behind it)
        if (!take(16, len) || !take(16, nlen)) return ERR_INPUT_END;
        if ((len ^ 0xFFFFu) != nlen) return ERR_STORED_LEN;
        if (!out_room(len)) return ERR_OUTPUT;
        for (uint32_t i = 0; i < len; ++i) {
            if (!take(8, v)) return ERR_INPUT_END;
            m.out_put(out_pos, v);
            ++out_pos;
        }
        return OK;
    }

    KQ_INF_HD int fixed_tables() {
        Tables* t = m.tables();
        for (uint32_t s = 0; s < (uint32_t)N_LIT; ++s) m.st8(&t->lens[s], s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u);
        for (uint32_t s = 0; s < 30; ++s) m.st8(&t->lens[N_LIT + s], 5u);
        m.tables_ready();
        int rc = build(t->lcount, t->lsym, t->lens, N_LIT);
        if (rc) return rc;
        rc = build(t->dcount, t->dsym, t->lens + N_LIT, 30);       // 30 codes of 5 bits: incomplete by design (codes 30 / 31)
        return rc == ERR_INCOMPLETE ? OK : rc;
    }

    KQ_INF_HD int dynamic_tables() {
        Tables* t = m.tables();
        uint32_t hlit, hdist, hclen, v;
        if (!take(5, hlit) || !take(5, hdist) || !take(4, hclen)) return ERR_INPUT_END;
        hlit += 257; hdist += 1; hclen += 4;
        if (hlit > 286 || hdist > 30) return ERR_HEADER_COUNTS;
        static constexpr uint8_t order[N_CLEN] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (uint32_t i = 0; i < (uint32_t)N_CLEN; ++i) {
            v = 0;
            if (i < hclen && !take(3, v)) return ERR_INPUT_END;
            m.st8(&t->lens[order[i]], v);
        }
        m.tables_ready();
        // the code-length code lives in the literal tables until the real ones replace it
        int rc = build(t->lcount, t->lsym, t->lens, N_CLEN);
        if (rc) return rc;                                         // zlib: the code-length code must be complete
        const uint32_t total = hlit + hdist;                       // <= 316
        uint8_t* lens = t->lens + N_CLEN;                          // behind the 19 lengths just used; 19 + total <= 335
        uint32_t i = 0;
        while (i < total) {
            const int s = decode(t->lcount, t->lsym);              // consumes >= 1 bit
            if (s < 0) return -s;
            if (s < 16) { m.st8(&lens[i], (uint32_t)s); ++i; m.tables_ready(); continue; }
            uint32_t prev = 0, rep;
            if (s == 16) {
                if (i == 0) return ERR_REPEAT;
                prev = lens[i - 1];
                if (!take(2, rep)) return ERR_INPUT_END;
                rep += 3;
            } else if (s == 17) {
                if (!take(3, rep)) return ERR_INPUT_END;
                rep += 3;
            } else if (s == 18) {
                if (!take(7, rep)) return ERR_INPUT_END;
                rep += 11;
            } else return ERR_SYMBOL;                              // (the code-length code has 19 symbols)
            if (rep > total - i) return ERR_REPEAT;
            for (uint32_t j = 0; j < rep; ++j) m.st8(&lens[i + j], prev);
            i += rep;
            m.tables_ready();
        }
        if (lens[256] == 0) return ERR_INCOMPLETE;                 // no end-of-block code
        // the distance lengths first, into their own place, then the literal set over the code-length code's tables
        rc = build(t->dcount, t->dsym, lens + hlit, hdist);
        if (rc == ERR_INCOMPLETE) {
            // zlib accepts an incomplete distance set only with at most one code, of one bit (and a set with no code at all)
            uint32_t coded = 0;
            for (int l = 1; l <= MAX_BITS; ++l) coded += t->dcount[l];
            if (!(coded == 0 || (coded == 1 && t->dcount[1] == 1))) return ERR_INCOMPLETE;
        } else if (rc) return rc;
        rc = build(t->lcount, t->lsym, lens, hlit);
        if (rc == ERR_INCOMPLETE) {
            uint32_t coded = 0;
            for (int l = 1; l <= MAX_BITS; ++l) coded += t->lcount[l];
            if (!(coded == 1 && t->lcount[1] == 1)) return ERR_INCOMPLETE;
        } else if (rc) return rc;
        return OK;
    }

    // the symbols of one fixed or dynamic block, up to its end-of-block code
    KQ_INF_HD int codes() {
        static constexpr uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        static constexpr uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        static constexpr uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        static constexpr uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
        const Tables* t = m.tables();
        for (;;) {
            int s = decode(t->lcount, t->lsym);                    // consumes >= 1 bit
            if (s < 0) return -s;
            if (s < 256) {
                if (!out_room(1)) return ERR_OUTPUT;
                m.out_put(out_pos, (uint32_t)s);
                ++out_pos;
                continue;
            }
            if (s == 256) return OK;
            s -= 257;
            if (s >= 29) return ERR_SYMBOL;                        // 286 / 287
            uint32_t v, len = lbase[s], dist;
            if (!take(lext[s], v)) return ERR_INPUT_END;
            len += v;
            const int d = decode(t->dcount, t->dsym);
            if (d < 0) return d == -ERR_SYMBOL ? ERR_DIST_CODE : -d;
            if (d >= 30) return ERR_DIST_CODE;
            if (!take(dext[d], v)) return ERR_INPUT_END;
            dist = dbase[d] + v;
            if (dist > out_pos) return ERR_DISTANCE;
            if (!out_room(len)) return ERR_OUTPUT;
            m.out_copy(out_pos, dist, len);
            out_pos += len;
        }
    }

    // the whole stream -> OK or ERR_*
    KQ_INF_HD int run() {
        uint32_t last = 0, type;
        while (!last) {
            if (!take(1, last) || !take(2, type)) return ERR_INPUT_END;
            int rc;
            if (type == 0) rc = stored();
            else if (type == 1) { rc = fixed_tables(); if (!rc) rc = codes(); }
            else if (type == 2) { rc = dynamic_tables(); if (!rc) rc = codes(); }
            else rc = ERR_BTYPE;
            if (rc) return rc;
        }
        if (out_pos != isize) return ERR_OUTPUT;
        refill();                                                  // (takes every byte that is left, up to the buffer's size)
        if (in_pos != data_len || n_bits >= 8) return ERR_TRAILING;      // the stream must end inside the last byte of data_len
        return OK;
    }
};

}  // namespace kqinf
