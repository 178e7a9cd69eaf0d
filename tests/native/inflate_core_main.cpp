// The BGZF block walk (kq_bgzf_host.h) and the DEFLATE core (kq_inflate_core.h) as a plain host program, built with
// -fsanitize=address,undefined by tests/test_inflate_core_host.py.  Every array the core touches is a heap block of exactly the
// size it may use: the compressed data (data_len), the text (isize) and the tables (sizeof(Tables)).
//
// Case file: u32 n, then per case  u32 expect, u32 member_len, u32 text_len, member bytes, text bytes.
//   expect 0        the member must decode to exactly the text
//   expect 1..13    the member must end in that error code (13 = CRC-32 mismatch, found here as in the kernel: after the decode)
//   expect 255      either: the text exactly, or any error code
// Output: per case one line "case i code max_len max_dist" and one line "name i <err_name(code)>", then "<failures> failures".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "kq_bgzf_host.h"
#include "kq_inflate_core.h"

struct HeapMem {
    std::unique_ptr<uint8_t[]> in, out;
    std::unique_ptr<kqinf::Tables> tab;
    uint32_t max_dist = 0;
    HeapMem(const uint8_t* data, uint32_t data_len, uint32_t isize) : in(new uint8_t[data_len]), out(new uint8_t[isize]), tab(new kqinf::Tables) {
        if (data_len) memcpy(in.get(), data, data_len);
        memset(tab.get(), 0xA5, sizeof(kqinf::Tables));      // no table entry is read before it was written: garbage, not zeros
    }
    uint32_t in_byte(uint32_t i) { return in[i]; }
    void out_put(uint32_t pos, uint32_t b) { out[pos] = (uint8_t)b; }
    void out_copy(uint32_t pos, uint32_t dist, uint32_t len) {
        if (dist > max_dist) max_dist = dist;
        for (uint32_t j = 0; j < len; ++j) out[pos + j] = out[pos - dist + j];
    }
    kqinf::Tables* tables() { return tab.get(); }
    void st16(uint16_t* p, uint32_t v) { *p = (uint16_t)v; }
    void st8(uint8_t* p, uint32_t v) { *p = (uint8_t)v; }
    void tables_ready() {}
};

static uint32_t crc_of(const uint8_t* p, uint32_t n) {
    uint32_t reg = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) reg = kqinf::crc_byte(reg, p[i]);
    return ~reg;
}

static bool read_u32(FILE* f, uint32_t* v) { return fread(v, 4, 1, f) == 1; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: inflate_core <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t n = 0;
    if (!read_u32(f, &n)) return 2;
    int failures = 0;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t expect, mlen, tlen;
        if (!read_u32(f, &expect) || !read_u32(f, &mlen) || !read_u32(f, &tlen)) return 2;
        // the member in a heap block of exactly its size: the walk reads nothing behind it
        std::unique_ptr<uint8_t[]> mem(new uint8_t[mlen]), text(new uint8_t[tlen]);
        if (mlen && fread(mem.get(), 1, mlen, f) != mlen) return 2;
        if (tlen && fread(text.get(), 1, tlen, f) != tlen) return 2;
        kqbgzf::Block b;
        uint64_t nb = 0, used = 0;
        const int src = kqbgzf::scan(mem.get(), mlen, &b, 1, &nb, &used);
        if (src != kqbgzf::OK || nb != 1 || used != mlen || b.data_off + (uint64_t)b.data_len + 8 != mlen) {
            printf("case %u: the block walk failed (%d, %llu blocks, %llu bytes)\n", c, src, (unsigned long long)nb, (unsigned long long)used);
            ++failures;
            continue;
        }
        HeapMem m(mem.get() + b.data_off, b.data_len, b.isize);
        kqinf::Inflate<HeapMem> inf(m, b.data_len, b.isize);
        int code = inf.run();
        if (code == kqinf::OK) {
            // the CRC as the kernel makes it: 64 stripes, combined
            const uint32_t stripe = (b.isize + 63) / 64;
            uint32_t crc = 0;
            for (uint32_t l = 0; l < 64; ++l) {
                const uint32_t lo = l * stripe < b.isize ? l * stripe : b.isize, hi = lo + stripe < b.isize ? lo + stripe : b.isize;
                crc ^= kqinf::gf2_mul(kqinf::gf2_xpow8(b.isize - hi), hi > lo ? crc_of(m.out.get() + lo, hi - lo) : 0u);
            }
            if (crc != crc_of(m.out.get(), b.isize)) { printf("case %u: striped CRC %08x differs from the serial one\n", c, crc); ++failures; }
            if (crc != b.crc32) code = kqinf::ERR_CRC;
        }
        const bool same = code == kqinf::OK && b.isize == tlen && (tlen == 0 || memcmp(m.out.get(), text.get(), tlen) == 0);
        bool ok;
        if (expect == 0) ok = same;
        else if (expect == 255) ok = same || code != kqinf::OK;
        else ok = code == (int)expect;
        if (!ok) { printf("case %u: expected %u, got %d (%s)\n", c, expect, code, kqinf::err_name(code)); ++failures; }
        printf("case %u %d %d %u\n", c, code, inf.max_len, m.max_dist);
        printf("name %u %s\n", c, kqinf::err_name(code));
    }
    fclose(f);
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
