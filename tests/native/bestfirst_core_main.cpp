// Stand-alone host program around kreeq_amd/csrc/kq_bestfirst_core.h (tests/test_bestfirst_core_host.py builds it with
// -fsanitize=address,undefined): one search per seed of a case file, each in a heap block of exactly
// kqbf::block_bytes(depth) bytes -- the size the ABI allocates per search -- so that a write past the block is a report.
//
// Case file:  k n_table n_seeds n_runs
//             n_table lines   key fw[4] bw[4]      the database
//             n_seeds lines   key fw[4] bw[4]      the seed k-mers with their merged counters
//             n_runs  lines   depth cov_cutoff
// Output:     per run "run <depth> <cutoff>", then per seed "<source>: <discovered keys, ascending>"; the last line is
//             "<n> failures" (searches that ended with an error code, or a count that differs from the flags).
#include <algorithm>
#include <array>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "kq_bestfirst_core.h"

namespace {

using Counters = std::array<uint32_t, 8>;

struct Graph {
    const std::unordered_map<uint64_t, Counters>* db;
    const std::unordered_map<uint64_t, Counters>* seeds;
    uint32_t cutoff;
    bool is_seed(uint64_t key) const { return seeds->count(key) != 0; }
    int db_mask(uint64_t key) const {
        const auto it = db->find(key);
        if (it == db->end()) return -1;
        int m = 0;
        for (int e = 0; e < 8; ++e) if (it->second[(size_t)e] > cutoff) m |= 1 << e;
        return m;
    }
};

bool read_entries(FILE* f, size_t n, std::vector<uint64_t>& order, std::unordered_map<uint64_t, Counters>& out) {
    for (size_t i = 0; i < n; ++i) {
        uint64_t key; Counters c;
        if (fscanf(f, "%" SCNu64, &key) != 1) return false;
        for (auto& v : c) if (fscanf(f, "%" SCNu32, &v) != 1) return false;
        out[key] = c; order.push_back(key);
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s case-file\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int k = 0; size_t n_table = 0, n_seeds = 0, n_runs = 0;
    if (fscanf(f, "%d %zu %zu %zu", &k, &n_table, &n_seeds, &n_runs) != 4 || k < 1 || k > 32) { fprintf(stderr, "bad header\n"); return 2; }
    std::unordered_map<uint64_t, Counters> db, seeds;
    std::vector<uint64_t> db_order, seed_order;
    if (!read_entries(f, n_table, db_order, db) || !read_entries(f, n_seeds, seed_order, seeds)) { fprintf(stderr, "bad entry line\n"); return 2; }
    size_t failures = 0;
    for (size_t r = 0; r < n_runs; ++r) {
        int depth = 0; uint32_t cutoff = 0;
        if (fscanf(f, "%d %" SCNu32, &depth, &cutoff) != 2 || depth < 0 || depth > kqbf::MAX_DEPTH) { fprintf(stderr, "bad run line\n"); return 2; }
        printf("run %d %u\n", depth, cutoff);
        const Graph g{&db, &seeds, cutoff};
        const size_t bytes = kqbf::block_bytes(depth);
        for (uint64_t source : seed_order) {
            void* block = malloc(bytes);
            if (!block) return 2;
            memset(block, 0xA5, bytes);                                  // nothing but the index is expected to be initialised
            memset(kqbf::index_of(block, depth), 0xFF, (size_t)kqbf::index_slots(depth) * 2);
            uint32_t mask = 0;
            const Counters& c = seeds[source];
            for (int e = 0; e < 8; ++e) if (c[(size_t)e] > cutoff) mask |= 1u << e;
            const uint32_t n_found = kqbf::search(block, depth, k, source, mask, g);
            const kqbf::Head* hd = kqbf::head_of(block);
            const kqbf::Node* nodes = kqbf::nodes_of(block);
            std::vector<uint64_t> found;
            for (uint32_t i = 0; i < hd->n_nodes; ++i) if (nodes[i].flags & kqbf::F_FOUND) found.push_back(nodes[i].key);
            if (hd->err) { fprintf(stderr, "source %" PRIu64 " depth %d: error code %u\n", source, depth, (unsigned)hd->err); ++failures; }
            if (found.size() != n_found || hd->n_found != n_found || hd->n_nodes > kqbf::node_bound(depth)) {
                fprintf(stderr, "source %" PRIu64 " depth %d: count %u, %zu flagged, %u nodes\n", source, depth, n_found, found.size(), (unsigned)hd->n_nodes);
                ++failures;
            }
            std::sort(found.begin(), found.end());
            printf("%" PRIu64 ":", source);
            for (uint64_t key : found) printf(" %" PRIu64, key);
            printf("\n");
            free(block);
        }
    }
    fclose(f);
    printf("%zu failures\n", failures);
    return failures ? 1 : 0;
}
