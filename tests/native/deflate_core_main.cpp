// The code builder of the BGZF writer (kq_deflate_core.h) as a plain host program, built with -fsanitize=address,undefined by
// tests/test_deflate_core_host.py.  Every array the core touches is a heap block of exactly the size it may use: the Work record
// (sizeof(Work), filled with garbage first) and the member (its final size).  Two tokenisers live here, not in the core: all
// literals, and a greedy matcher with a one-entry hash table; a third source of tokens is a hand-made list whose expansion IS the
// text (every length and distance symbol).  Every member is built and checked by make_member (deflate_member.h, shared with
// deflate_tokens_main.cpp): inflated in-process by kq_inflate_core.h and written to <dir>/<name>.gz next to <dir>/<name>.txt
// for the pytest side (zlib, wbits = 31).
// Output: one line per member "member <name> <size> <dynamic> <max code length> <n_text>", lines "set ..." for the direct code
// length cases, then "<failures> failures".
#include "deflate_member.h"

// make_member of deflate_member.h, reported
static Made make_and_report(const std::string& dir, const std::string& name, const std::vector<uint8_t>& text, const std::vector<Token>& tok) {
    const Made m = make_member(dir, name, text, tok);
    if (m.size) printf("member %s %u %d %d %u\n", name.c_str(), m.size, m.dynamic ? 1 : 0, m.max_len, (uint32_t)text.size());
    return m;
}

static std::vector<Token> all_literals(const std::vector<uint8_t>& t) {
    std::vector<Token> out;
    for (uint8_t b : t) out.push_back(Token{0, 0, b});
    return out;
}
static std::vector<Token> greedy(const std::vector<uint8_t>& t) {
    std::vector<Token> out;
    std::vector<int32_t> head(1 << 15, -1);
    const uint32_t n = (uint32_t)t.size();
    auto hash = [&](uint32_t p) { return ((t[p] | t[p + 1] << 8 | (uint32_t)t[p + 2] << 16) * 0x9E3779B1u) >> 17; };
    for (uint32_t p = 0; p < n;) {
        uint32_t len = 0, dist = 0;
        if (p + 3 <= n) {
            const uint32_t h = hash(p);
            const int32_t c = head[h];
            if (c >= 0 && p - (uint32_t)c <= kqdef::WINDOW) {
                while (len < kqdef::MAX_MATCH && p + len < n && t[(uint32_t)c + len] == t[p + len]) ++len;
                dist = p - (uint32_t)c;
            }
        }
        const uint32_t step = len >= kqdef::MIN_MATCH ? len : 1;
        if (len >= kqdef::MIN_MATCH) out.push_back(Token{(uint16_t)len, (uint16_t)(dist - 1), 0});
        else out.push_back(Token{0, 0, t[p]});
        for (uint32_t q = p; q < p + step; ++q) if (q + 3 <= n) head[hash(q)] = (int32_t)q;
        p += step;
    }
    return out;
}
static std::vector<uint8_t> expand(const std::vector<Token>& tok) {
    std::vector<uint8_t> t;
    for (const Token& k : tok) {
        if (!k.len) { t.push_back(k.lit); continue; }
        for (uint32_t j = 0; j < k.len; ++j) t.push_back(t[t.size() - (k.dist + 1u)]);
    }
    return t;
}

static uint32_t g_rng = 12345;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

// table-like text: lines of small numbers with repeats
static std::vector<uint8_t> table_text(uint32_t n) {
    std::vector<uint8_t> t;
    while (t.size() < n) {
        char line[64];
        const int len = snprintf(line, sizeof line, "chr%u\t%u\t%u:%u:%u\n", rnd() % 3, (uint32_t)t.size(), rnd() % 40, rnd() % 7, rnd() % 7);
        t.insert(t.end(), line, line + len);
    }
    t.resize(n);
    return t;
}

// a frequency table given directly: lengths within max, Kraft sum 1, rarer symbols never shorter
static void check_set(const char* name, const std::vector<uint32_t>& freq, int max, int min_codes, int expect_max) {
    std::unique_ptr<kqdef::Work> w(new kqdef::Work);
    memset((void*)w.get(), 0xA5, sizeof(kqdef::Work));
    std::unique_ptr<uint8_t[]> lens(new uint8_t[freq.size()]);
    const int rc = kqdef::build_lengths(*w, freq.data(), (int)freq.size(), max, min_codes, lens.get());
    CHECK(rc == kqdef::OK, "%s: error %d", name, rc);
    if (rc) return;
    uint32_t k = 0, codes = 0, used = 0;
    int longest = 0;
    for (uint32_t f : freq) used += f != 0;
    for (size_t s = 0; s < freq.size(); ++s) {
        CHECK(lens[s] <= max, "%s: symbol %zu has %u bits", name, s, lens[s]);
        CHECK(used < 2 ? (lens[s] != 0 || freq[s] == 0) : (lens[s] != 0) == (freq[s] != 0), "%s: symbol %zu frequency %u length %u", name, s, freq[s], lens[s]);
        if (lens[s]) { k += 1u << (15 - lens[s]); ++codes; if (lens[s] > longest) longest = lens[s]; }
        for (size_t r = 0; r < freq.size(); ++r)
            if (freq[s] && freq[r] > freq[s]) CHECK(lens[r] <= lens[s], "%s: the rarer symbol %zu has the shorter code than %zu", name, s, r);
    }
    CHECK(k == 32768u || (codes == 1 && k == 16384u), "%s: Kraft sum %u / 32768 over %u codes", name, k, codes);
    if (expect_max) CHECK(longest == expect_max, "%s: longest code %d, expected %d", name, longest, expect_max);
    printf("set %s %u %d\n", name, codes, longest);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: deflate_core <output directory>\n"); return 2; }
    const std::string dir = argv[1];

    // ---- code lengths from frequency tables ----
    std::vector<uint32_t> fib(kqdef::N_LIT, 0);
    { uint32_t a = 1, b = 1; for (int i = 0; i < 30; ++i) { fib[(size_t)(7 * i)] = a; const uint32_t c = a + b; a = b; b = c; } }      // sum < 2^23, depth 29 unlimited
    check_set("fibonacci_30_of_286", fib, 15, 2, 15);
    std::vector<uint32_t> cl(kqdef::N_CLEN, 0);
    { uint32_t a = 1, b = 1; for (int i = 0; i < 19; ++i) { cl[(size_t)i] = a; const uint32_t c = a + b; a = b; b = c; } }
    check_set("fibonacci_19_limit_7", cl, 7, 2, 7);
    check_set("flat_286", std::vector<uint32_t>(286, 5), 15, 2, 9);
    check_set("flat_30", std::vector<uint32_t>(30, 1), 15, 1, 5);
    check_set("flat_19_limit_7", std::vector<uint32_t>(19, 3), 7, 2, 5);
    { std::vector<uint32_t> f(286, 1); f[0] = 60000; check_set("one_heavy_286", f, 15, 2, 0); }
    { std::vector<uint32_t> f(286, 0); for (int i = 0; i < 286; ++i) f[(size_t)i] = 1u + (uint32_t)(i * i) % 97u; check_set("ragged_286", f, 15, 2, 0); }
    { std::vector<uint32_t> f(286, 0); uint32_t a = 1; for (int i = 0; i < 22; ++i) { f[(size_t)i] = a; a = a * 2 > 4000000u ? a : a * 2; } check_set("powers_of_two", f, 15, 2, 15); }
    { std::vector<uint32_t> f(30, 0); check_set("no_distance", f, 15, 1, 1); }
    { std::vector<uint32_t> f(30, 0); f[17] = 9; check_set("one_distance", f, 15, 1, 1); }
    { std::vector<uint32_t> f(286, 0); f[256] = 1; check_set("only_end_of_block", f, 15, 2, 1); }
    { std::vector<uint32_t> f(19, 0); f[18] = 4; check_set("one_code_length_symbol", f, 7, 2, 1); }
    { std::vector<uint32_t> f(286, 0); f[65] = 100; f[256] = 1; check_set("one_literal_and_end", f, 15, 2, 1); }
    for (int seed = 0; seed < 40; ++seed) {                         // skewed random tables at both limits
        std::vector<uint32_t> f(seed % 2 ? 19 : 286, 0);
        for (auto& x : f) { const uint32_t r = rnd(); x = (r & 3u) ? (1u << (r >> 4) % 14u) + (r >> 9) % 50u : 0u; }
        char name[32]; snprintf(name, sizeof name, "random_%d", seed);
        check_set(name, f, seed % 2 ? 7 : 15, 2, 0);
    }

    // ---- whole members ----
    for (uint32_t n : {0u, 1u, 2u, 3u, 258u, 259u, 65280u}) {
        const std::vector<uint8_t> t = table_text(n);
        make_and_report(dir, "table_" + std::to_string(n) + "_literals", t, all_literals(t));
        const Made m = make_and_report(dir, "table_" + std::to_string(n) + "_greedy", t, greedy(t));
        if (n == 65280) CHECK(m.dynamic && m.size < n / 2, "the table text compresses to %u bytes", m.size);
    }
    { std::vector<uint8_t> t(26); for (int i = 0; i < 26; ++i) t[(size_t)i] = (uint8_t)('a' + i); std::vector<uint8_t> tt; for (int r = 0; r < 40; ++r) { for (auto& b : t) b = (uint8_t)('a' + rnd() % 26); tt.insert(tt.end(), t.begin(), t.end()); }
      const Made m = make_and_report(dir, "no_match", tt, all_literals(tt)); CHECK(m.dynamic, "no_match is dynamic"); }
    { const std::vector<uint8_t> t(1000, 'A'); const Made m = make_and_report(dir, "one_distance_symbol", t, greedy(t)); CHECK(m.dynamic && m.size < 60, "A x 1000 takes %u bytes", m.size); }
    { const std::vector<uint8_t> t(200, 'A'); const Made m = make_and_report(dir, "one_literal", t, all_literals(t)); CHECK(m.dynamic && m.max_len == 1, "one literal: longest code %d", m.max_len); }
    { const std::vector<uint8_t> t(65280, 'A'); const Made m = make_and_report(dir, "A_65280", t, greedy(t)); CHECK(m.dynamic && m.size < 1024, "A x 65280 takes %u bytes", m.size); }
    {   // literal frequencies 1, 2, 4, 7, 12 ... (each the sum of the two before it, plus one: no ties, so the tree is a chain) over 20
        // byte values: an unlimited code would be 20 bits deep
        std::vector<uint8_t> t;
        uint32_t a = 1, b = 2;
        for (int i = 0; i < 20; ++i) { t.insert(t.end(), a, (uint8_t)(40 + i)); const uint32_t c = a + b + 1; a = b; b = c; }
        for (size_t i = t.size(); i > 1; --i) std::swap(t[i - 1], t[rnd() % i]);
        const Made m = make_and_report(dir, "fibonacci_text", t, all_literals(t));
        CHECK(m.dynamic && m.max_len == 15, "fibonacci text: longest code %d", m.max_len);
    }
    {   // all 286 literal / length codes and all 30 distance codes: the token list is made by hand, the text is its expansion
        std::vector<Token> tok;
        for (int i = 0; i < 256; ++i) tok.push_back(Token{0, 0, (uint8_t)i});
        for (int i = 0; i < 40000; ++i) tok.push_back(Token{0, 0, (uint8_t)rnd()});
        const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        for (int r = 0; r < 3; ++r)
            for (int i = 0; i < 30; ++i) {
                const uint32_t extra_l = r == 0 ? 0u : r == 1 && i < 28 ? (uint32_t)(lbase[i + 1] - lbase[i] - 1) : 0u;
                const uint32_t extra_d = r == 0 ? 0u : i < 29 ? (uint32_t)(dbase[i + 1] - dbase[i] - 1) : 32768u - 24577u;
                tok.push_back(Token{(uint16_t)(lbase[i % 29] + (i % 29 < 28 ? extra_l : 0u)), (uint16_t)(dbase[i] + extra_d - 1u), 0});
            }
        const std::vector<uint8_t> t = expand(tok);
        CHECK(t.size() <= kqdef::MEMBER_TEXT, "all symbols: %zu bytes", t.size());
        std::unique_ptr<kqdef::Work> w(new kqdef::Work);
        kqdef::clear_freq(*w);
        for (const Token& k : tok) { if (k.len) kqdef::count_match(*w, k.len, k.dist + 1u); else kqdef::count_literal(*w, k.lit); }
        w->lfreq[256] = 1;
        for (int s = 0; s < kqdef::N_LIT; ++s) CHECK(w->lfreq[s] > 0, "all symbols: literal / length code %d unused", s);
        for (int s = 0; s < kqdef::N_DIST; ++s) CHECK(w->dfreq[s] > 0, "all symbols: distance code %d unused", s);
        make_and_report(dir, "all_symbols", t, tok);
    }
    for (uint32_t n : {1000u, 65280u}) {                            // random bytes: the stored block, at exactly 18 + 5 + n + 8
        std::vector<uint8_t> t(n);
        for (auto& b : t) b = (uint8_t)rnd();
        const Made a = make_and_report(dir, "random_" + std::to_string(n) + "_literals", t, all_literals(t));
        const Made g = make_and_report(dir, "random_" + std::to_string(n) + "_greedy", t, greedy(t));
        CHECK(!a.dynamic && a.size == 18 + 5 + n + 8, "random bytes, literals: %u bytes", a.size);
        CHECK(!g.dynamic && g.size == 18 + 5 + n + 8, "random bytes, greedy: %u bytes", g.size);
    }
    // the symbol tables against RFC 1951's
    for (uint32_t len = 3; len <= 258; ++len) {
        uint32_t s, nb, e; kqdef::len_sym(len, s, nb, e);
        static const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        CHECK(s < 29 && lbase[s] + e == len && e < (1u << nb) && nb == kqdef::len_extra_bits(s) && (s == 28 || len < lbase[s + 1]), "length %u -> symbol %u + %u (%u bits)", len, s, e, nb);
    }
    for (uint32_t dist = 1; dist <= 32768; ++dist) {
        uint32_t s, nb, e; kqdef::dist_sym(dist, s, nb, e);
        static const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        CHECK(s < 30 && dbase[s] + e == dist && e < (1u << nb) && nb == kqdef::dist_extra_bits(s), "distance %u -> symbol %u + %u (%u bits)", dist, s, e, nb);
    }
    { uint8_t eof[28]; for (uint32_t i = 0; i < 28; ++i) eof[i] = (uint8_t)kqdef::eof_byte(i);
      static const uint8_t want[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      CHECK(memcmp(eof, want, 28) == 0, "the end-of-file marker"); }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
