// Stand-alone host program around kreeq_amd/csrc/kq_variant_core.h (tests/test_variant_core_host.py builds it with
// -fsanitize=address,undefined): one search per position of every segment of a case file whose k-mer is in the table, each
// in a heap block of exactly kqvar::block_bytes(depth, span) bytes -- the size the ABI allocates per search -- and every path
// sequence in a buffer of exactly its length, so that a write past either is a report.
//
// Case file:  k n_table n_segments n_runs
//             n_table    lines   key fw[4] bw[4]      the database
//             n_segments lines   a run of ACGTacgt
//             n_runs     lines   depth max_span cov_cutoff
// Output:     per run "run <depth> <max_span> <cutoff>", then per path "<segment> <pos> <type> <ref_len> <sequence or ->" in
//             segment, position and destination order (pos = c + k); the last line is "<n> failures" (searches that ended
//             with an error code, or whose counts differ from their paths).  In front of it "probe <errors> <searches>
//             <refused heads>": every position of the first segment searched once more at depth 253 in a block sized for depth
//             0 -- the pool or the destination list overflows, which must end the search with an error code and nothing
//             else (the sanitizers watch the block's ends) -- and path() on a head that no search wrote.
#include <array>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "kq_variant_core.h"

namespace {

using Counters = std::array<uint32_t, 8>;

struct Graph {
    const std::unordered_map<uint64_t, Counters>* db;
    const std::string* seg;
    uint32_t cutoff;
    uint32_t edge_mask(uint64_t key) const {
        const auto it = db->find(key);
        if (it == db->end()) return 0;
        uint32_t m = 0;
        for (int i = 0; i < 4; ++i) {
            if (it->second[(size_t)i] != 0) m |= 1u << i;
            if (it->second[(size_t)(4 + i)] > cutoff) m |= 1u << (4 + i);
        }
        return m;
    }
    uint32_t base(uint64_t p) const {
        switch (seg->at((size_t)p) & 0xDF) { case 'A': return 0; case 'C': return 1; case 'G': return 2; default: return 3; }
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s case-file\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int k = 0; size_t n_table = 0, n_segs = 0, n_runs = 0;
    if (fscanf(f, "%d %zu %zu %zu", &k, &n_table, &n_segs, &n_runs) != 4 || k < 2 || k > 32) { fprintf(stderr, "bad header\n"); return 2; }
    std::unordered_map<uint64_t, Counters> db;
    for (size_t i = 0; i < n_table; ++i) {
        uint64_t key; Counters c;
        if (fscanf(f, "%" SCNu64, &key) != 1) { fprintf(stderr, "bad entry line\n"); return 2; }
        for (auto& v : c) if (fscanf(f, "%" SCNu32, &v) != 1) { fprintf(stderr, "bad entry line\n"); return 2; }
        db[key] = c;
    }
    std::vector<std::string> segs(n_segs);
    std::vector<char> line(1 << 20);
    for (auto& s : segs) {
        if (fscanf(f, "%1048575s", line.data()) != 1) { fprintf(stderr, "bad segment line\n"); return 2; }
        s = line.data();
        if (s.find_first_not_of("ACGTacgt") != std::string::npos) { fprintf(stderr, "segment with a non-base\n"); return 2; }
    }
    size_t failures = 0;
    for (size_t r = 0; r < n_runs; ++r) {
        int depth = 0, span = 0; uint32_t cutoff = 0;
        if (fscanf(f, "%d %d %" SCNu32, &depth, &span, &cutoff) != 3 || depth < 0 || depth > kqvar::MAX_DEPTH || span < 0 || span > kqvar::MAX_SPAN) {
            fprintf(stderr, "bad run line\n"); return 2;
        }
        printf("run %d %d %u\n", depth, span, cutoff);
        const size_t bytes = kqvar::block_bytes(depth, span);
        for (size_t si = 0; si < n_segs; ++si) {
            const std::string& seg = segs[si];
            if (seg.size() < (size_t)k) continue;
            const uint64_t kcount = seg.size() - (size_t)k + 1;
            const Graph g{&db, &seg, cutoff};
            for (uint64_t c = 0; c < kcount; ++c) {
                uint64_t fw = 0, rv = 0;
                for (int j = 0; j < k; ++j) { const uint64_t b = g.base(c + (uint64_t)j); fw |= b << (2 * j); rv |= (3 - b) << (2 * (k - 1 - j)); }
                if (!db.count(fw < rv ? fw : rv)) continue;             // :149-152: nothing to search from
                void* block = malloc(bytes);
                if (!block) return 2;
                memset(block, 0xA5, bytes);                              // nothing but the index is expected to be initialised
                memset(kqvar::index_of(block, depth, span), 0xFF, (size_t)kqvar::index_slots(depth) * 2);
                const uint32_t n_paths = kqvar::search(block, depth, span, k, c, kcount, g);
                const kqbf::Head* hd = kqvar::head_of(block);
                if (hd->err) { fprintf(stderr, "segment %zu position %" PRIu64 " depth %d span %d: error code %u\n", si, c, depth, span, (unsigned)hd->err); ++failures; }
                if (hd->n_found != n_paths || hd->n_nodes > kqvar::node_bound(depth) || n_paths > kqvar::dest_bound(depth) || hd->pops > depth + 1) {
                    fprintf(stderr, "segment %zu position %" PRIu64 ": %u paths, head says %u, %u nodes, %u pops\n", si, c, n_paths, (unsigned)hd->n_found, (unsigned)hd->n_nodes,
                            (unsigned)hd->pops);
                    ++failures;
                }
                uint64_t seq_bytes = 0;
                for (uint32_t d = 0; d < n_paths; ++d) {
                    kqvar::Path p, q;
                    if (!kqvar::path(block, depth, span, k, d, g, &p, nullptr)) { fprintf(stderr, "segment %zu position %" PRIu64 " path %u: failed\n", si, c, d); ++failures; continue; }
                    char* out = (char*)malloc(p.seq_len ? p.seq_len : 1);
                    if (!out) return 2;
                    if (!kqvar::path(block, depth, span, k, d, g, &q, out) || q.seq_len != p.seq_len || q.type != p.type || q.ref_len != p.ref_len) ++failures;
                    seq_bytes += p.seq_len;
                    printf("%zu %" PRIu64 " %u %u %s\n", si, c + (uint64_t)k, (unsigned)p.type, (unsigned)p.ref_len, p.seq_len ? std::string(out, p.seq_len).c_str() : "-");
                    free(out);
                }
                if (!hd->err && seq_bytes != kqvar::seq_bytes_of(hd)) { fprintf(stderr, "segment %zu position %" PRIu64 ": sequence bytes %" PRIu64 " != %u\n", si, c, seq_bytes, kqvar::seq_bytes_of(hd)); ++failures; }
                free(block);
            }
        }
    }
    fclose(f);
    size_t probe_err = 0, probe_n = 0, probe_refused = 0;
    if (n_segs && segs[0].size() >= (size_t)k) {
        const std::string& seg = segs[0];
        const uint64_t kcount = seg.size() - (size_t)k + 1;
        const Graph g{&db, &seg, 0};
        const int span = 8;
        const size_t bytes = kqvar::block_bytes(0, span);
        for (uint64_t c = 0; c < kcount; ++c, ++probe_n) {
            void* block = malloc(bytes);
            if (!block) return 2;
            memset(block, 0xA5, bytes);
            memset(kqvar::index_of(block, 0, span), 0xFF, (size_t)kqvar::index_slots(0) * 2);
            kqvar::Search<Graph> s(block, 0, span, k, g);               // a block for depth 0 ...
            const uint32_t n_paths = s.run(c, kcount, kqvar::MAX_DEPTH);       // ... and a search that wants far more
            const kqbf::Head* hd = kqvar::head_of(block);
            if (hd->err) { ++probe_err; if (n_paths || hd->n_found || kqvar::seq_bytes_of(hd)) ++failures; }
            memset(block, 0xA5, sizeof(kqbf::Head));                    // not a head that run() wrote
            kqvar::Path p;
            if (!kqvar::path(block, 0, span, k, 0, g, &p, nullptr)) ++probe_refused;
            free(block);
        }
    }
    printf("probe %zu %zu %zu\n", probe_err, probe_n, probe_refused);
    printf("%zu failures\n", failures);
    return failures ? 1 : 0;
}
