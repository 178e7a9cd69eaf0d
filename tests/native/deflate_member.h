// One BGZF member from a token list through the code builder (kq_deflate_core.h), for the host programs of this directory:
// deflate_core_main.cpp (tokens made there) and deflate_tokens_main.cpp (tokens read from files).  Every array the core touches
// is a heap block of exactly the size it may use, so that the address sanitizer sees an index one past it.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "kq_deflate_core.h"
#include "kq_inflate_core.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Token { uint16_t len; uint16_t dist; uint8_t lit; };      // len 0: a literal; dist is stored minus one

struct HeapMem {                                                  // the inflater's memory, as in inflate_core_main.cpp
    std::unique_ptr<uint8_t[]> in, out;
    std::unique_ptr<kqinf::Tables> tab;
    HeapMem(const uint8_t* data, uint32_t data_len, uint32_t isize) : in(new uint8_t[data_len]), out(new uint8_t[isize]), tab(new kqinf::Tables) {
        if (data_len) memcpy(in.get(), data, data_len);
        memset(tab.get(), 0xA5, sizeof(kqinf::Tables));
    }
    uint32_t in_byte(uint32_t i) { return in[i]; }
    void out_put(uint32_t pos, uint32_t b) { out[pos] = (uint8_t)b; }
    void out_copy(uint32_t pos, uint32_t dist, uint32_t len) { for (uint32_t j = 0; j < len; ++j) out[pos + j] = out[pos - dist + j]; }
    kqinf::Tables* tables() { return tab.get(); }
    void st16(uint16_t* p, uint32_t v) { *p = (uint16_t)v; }
    void st8(uint8_t* p, uint32_t v) { *p = (uint8_t)v; }
    void tables_ready() {}
};

struct HeapSink {
    std::unique_ptr<uint8_t[]> p;
    uint32_t size;
    explicit HeapSink(uint32_t n) : p(new uint8_t[n]), size(n) { memset(p.get(), 0xA5, n); }
    bool put(uint32_t pos, uint32_t b) { if (pos >= size) return false; p[pos] = (uint8_t)b; return true; }
};

static uint32_t crc_of(const uint8_t* p, uint32_t n) {
    uint32_t reg = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) reg = kqinf::crc_byte(reg, p[i]);
    return ~reg;
}

static uint32_t n_codes(const uint8_t* lens, int n) { uint32_t c = 0; for (int s = 0; s < n; ++s) c += lens[s] != 0; return c; }

struct Made { uint32_t size = 0; bool dynamic = false; int max_len = 0, max_dist_len = 0; uint32_t max_token_bits = 0; };      // max_len: of the literal / length set

// tokens (whose expansion is `text`) -> one member, checked and written to <dir>/<name>.gz (and the text to <dir>/<name>.txt,
// unless the caller read it from there).  The caller reports the member.
static Made make_member(const std::string& dir, const std::string& name, const std::vector<uint8_t>& text, const std::vector<Token>& tok, bool write_text = true) {
    Made made;
    const uint32_t n = (uint32_t)text.size();
    std::unique_ptr<kqdef::Work> w(new kqdef::Work);
    memset((void*)w.get(), 0xA5, sizeof(kqdef::Work));
    kqdef::clear_freq(*w);
    for (const Token& k : tok) { if (k.len) kqdef::count_match(*w, k.len, k.dist + 1u); else kqdef::count_literal(*w, k.lit); }
    const kqdef::Plan plan = kqdef::plan_block(*w, n);
    CHECK(plan.err == kqdef::OK, "%s: plan error %d", name.c_str(), plan.err);
    if (plan.err) return made;
    CHECK(plan.payload <= kqdef::STORED_BYTES + n, "%s: payload %u above the stored form", name.c_str(), plan.payload);
    // the sets of the header, whether the block is taken or not
    const uint32_t full = 1u << kqdef::MAX_BITS;
    const uint32_t kl = kqdef::kraft_sum(w->llen, kqdef::N_LIT), kd = kqdef::kraft_sum(w->dlen, kqdef::N_DIST), kc = kqdef::kraft_sum(w->clen, kqdef::N_CLEN);
    CHECK(kl == full, "%s: literal set sums to %u / 32768", name.c_str(), kl);
    CHECK(kc == full, "%s: code-length set sums to %u / 32768", name.c_str(), kc);
    CHECK(kd == full || (n_codes(w->dlen, kqdef::N_DIST) == 1 && kd == full / 2), "%s: distance set sums to %u / 32768", name.c_str(), kd);
    for (int s = 0; s < kqdef::N_LIT; ++s) { CHECK(w->llen[s] <= kqdef::MAX_BITS, "llen"); if (w->llen[s] > made.max_len) made.max_len = w->llen[s]; }
    for (int s = 0; s < kqdef::N_DIST; ++s) { CHECK(w->dlen[s] <= kqdef::MAX_BITS, "dlen"); if (w->dlen[s] > made.max_dist_len) made.max_dist_len = w->dlen[s]; }
    for (int s = 0; s < kqdef::N_CLEN; ++s) CHECK(w->clen[s] <= kqdef::MAX_CLEN_BITS, "%s: code-length code of %u bits", name.c_str(), w->clen[s]);
    made.dynamic = plan.dynamic;
    made.size = kqdef::HEADER_BYTES + plan.payload + kqdef::TRAILER_BYTES;
    HeapSink sink(made.size);
    for (uint32_t i = 0; i < kqdef::HEADER_BYTES; ++i) sink.put(i, kqdef::header_byte(i, made.size));
    if (plan.dynamic) {
        kqdef::BitWriter<HeapSink> bw(sink, kqdef::HEADER_BYTES);
        for (uint32_t i = 0; i < w->n_items; ++i) bw.put(w->u.items[i] & 0xFFFFFFu, w->u.items[i] >> 24);
        uint64_t bits; uint32_t nb;
        for (const Token& k : tok) {
            if (k.len) kqdef::match_bits(*w, k.len, k.dist + 1u, bits, nb); else kqdef::literal_bits(*w, k.lit, bits, nb);
            CHECK(nb >= 1 && nb <= 48, "%s: a token of %u bits", name.c_str(), nb);
            if (nb > made.max_token_bits) made.max_token_bits = nb;
            bw.put(bits, nb);
        }
        kqdef::literal_bits(*w, kqdef::EOB, bits, nb);
        bw.put(bits, nb);
        bw.finish();
        CHECK(bw.err == kqdef::OK && bw.pos == kqdef::HEADER_BYTES + plan.payload, "%s: the writer ended at %u, planned %u", name.c_str(), bw.pos, kqdef::HEADER_BYTES + plan.payload);
    } else {
        for (uint32_t i = 0; i < kqdef::STORED_BYTES; ++i) sink.put(kqdef::HEADER_BYTES + i, kqdef::stored_byte(i, n));
        for (uint32_t i = 0; i < n; ++i) sink.put(kqdef::HEADER_BYTES + kqdef::STORED_BYTES + i, text[i]);
    }
    const uint32_t crc = crc_of(text.data(), n);
    for (uint32_t i = 0; i < kqdef::TRAILER_BYTES; ++i) CHECK(sink.put(kqdef::HEADER_BYTES + plan.payload + i, kqdef::trailer_byte(i, crc, n)), "trailer");
    // the project's own inflater reads it back
    HeapMem m(sink.p.get() + kqdef::HEADER_BYTES, plan.payload, n);
    kqinf::Inflate<HeapMem> inf(m, plan.payload, n);
    const int code = inf.run();
    CHECK(code == kqinf::OK, "%s: inflate says %s", name.c_str(), kqinf::err_name(code));
    CHECK(code != kqinf::OK || n == 0 || memcmp(m.out.get(), text.data(), n) == 0, "%s: the text differs", name.c_str());
    FILE* f = fopen((dir + "/" + name + ".gz").c_str(), "wb");
    FILE* g = write_text ? fopen((dir + "/" + name + ".txt").c_str(), "wb") : nullptr;
    if (!f || (write_text && !g)) { printf("cannot write into %s\n", dir.c_str()); ++failures; if (f) fclose(f); if (g) fclose(g); return made; }
    fwrite(sink.p.get(), 1, made.size, f);
    if (n && g) fwrite(text.data(), 1, n, g);
    fclose(f); if (g) fclose(g);
    return made;
}
