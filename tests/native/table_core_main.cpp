// The line rules of the per-base tables (kreeq_amd/csrc/kq_table_core.h) as a plain host program, built with
// -fsanitize=address,undefined by tests/test_table_core_host.py.  It reads cases from a file, places every line with the LENGTH
// functions, writes it with the WRITERS into a buffer of exactly that size (the sanitizer sees any byte outside), checks that
// each writer ends where the length said, and prints the text; the test compares it with tests/table_ref.py byte for byte.
//
// case file:  n_cases, then per case
//   format k n_triples n_pieces
//   n_triples lines "c f b"
//   n_pieces lines  "first n abs_pos n_ctx header name"
// output: per case "case <bytes>\n" followed by the bytes; the last line is "<n> failures".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "kq_table_core.h"

namespace {

struct Piece { uint64_t first, n, abs_pos; uint32_t n_ctx; int header; std::string name; };
struct BufSink {
    std::vector<char>& b;
    void put(uint64_t at, char c) { b.at((size_t)at) = c; }
};
struct Win {                                                                 // the window of position i of a piece
    const std::vector<uint32_t>& t; const Piece& p; uint64_t i;
    uint32_t operator()(int back, int column) const {
        if ((uint64_t)back > i + p.n_ctx) return 0;
        return t[(size_t)(p.first + i - (uint64_t)back) * 3 + (size_t)column];
    }
};

int failures = 0;

uint64_t line_len(int format, int k, const std::vector<uint32_t>& t, const Piece& p, uint64_t i) {
    if (format == 1) { const uint32_t* v = &t[(size_t)(p.first + i) * 3]; return kqtab::fixed_line_len(v[0], v[1], v[2]); }
    const Win w{t, p, i};
    uint32_t digits = 0;
    for (int back = 0; back < k; ++back) digits += kqtab::fixed_digits(w(back, 0), w(back, 1), w(back, 2));
    return kqtab::expanded_line_len((uint32_t)p.name.size(), kqtab::digits_u64(p.abs_pos + i), digits, k);
}

void run_case(FILE* f) {
    int format, k;
    unsigned long long n_triples, n_pieces;
    if (fscanf(f, "%d %d %llu %llu", &format, &k, &n_triples, &n_pieces) != 4) { ++failures; return; }
    std::vector<uint32_t> t((size_t)n_triples * 3);
    for (auto& v : t) if (fscanf(f, "%" SCNu32, &v) != 1) { ++failures; return; }
    std::vector<Piece> pieces((size_t)n_pieces);
    for (auto& p : pieces) {
        char name[70000];
        if (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu32 " %d %69999s", &p.first, &p.n, &p.abs_pos, &p.n_ctx, &p.header, name) != 6) { ++failures; return; }
        p.name = name;
    }
    // pass 1: where every line starts
    uint64_t total = 0;
    for (auto& p : pieces) {
        if (format == 1 && p.header) total += kqtab::header_line_len((uint32_t)p.name.size(), p.abs_pos);
        for (uint64_t i = 0; i < p.n; ++i) total += line_len(format, k, t, p, i);
    }
    std::vector<char> out((size_t)total);
    BufSink sink{out};
    // pass 2: the writers
    uint64_t at = 0;
    const char col = format == 2 ? '\t' : ',', ent = format == 2 ? ':' : ',';
    for (auto& p : pieces) {
        if (format == 1 && p.header) {
            const uint64_t end = kqtab::put_header_line(sink, at, p.name.data(), (uint32_t)p.name.size(), p.abs_pos);
            if (end != at + kqtab::header_line_len((uint32_t)p.name.size(), p.abs_pos)) ++failures;
            at = end;
        }
        for (uint64_t i = 0; i < p.n; ++i) {
            const uint64_t want = at + line_len(format, k, t, p, i);
            if (format == 1) { const uint32_t* v = &t[(size_t)(p.first + i) * 3]; at = kqtab::put_fixed_line(sink, at, v[0], v[1], v[2]); }
            else at = kqtab::put_expanded_line(sink, at, p.name.data(), (uint32_t)p.name.size(), p.abs_pos + i, k, col, ent, Win{t, p, i});
            if (at != want) ++failures;
        }
    }
    if (at != total) ++failures;
    printf("case %llu\n", (unsigned long long)total);
    fwrite(out.data(), 1, out.size(), stdout);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: table_core <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int n_cases = 0;
    if (fscanf(f, "%d", &n_cases) != 1) return 2;
    for (int c = 0; c < n_cases; ++c) run_case(f);
    fclose(f);
    // the digit counts at every power of ten, both widths
    uint64_t p = 1;
    for (int d = 1; d <= 20; ++d, p *= 10) {
        if (kqtab::digits_u64(p) != d || (d > 1 && kqtab::digits_u64(p - 1) != d - 1)) ++failures;
        if (d <= 10 && (kqtab::digits_u32((uint32_t)p) != d || (d > 1 && kqtab::digits_u32((uint32_t)(p - 1)) != d - 1))) ++failures;
    }
    if (kqtab::digits_u64(~0ull) != 20 || kqtab::digits_u32(~0u) != 10 || kqtab::digits_u64(0) != 1) ++failures;
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
