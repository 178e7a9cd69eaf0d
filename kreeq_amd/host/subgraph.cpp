// Best-first expansion of `kreeq subgraph` (reference DBG::bestFirst / dijkstra, src/subgraph.cpp:417-579) on top of two
// GPU tables: `db`, the database, and `sub`, the seeded subgraph.
//
// The search is pointer chasing, serial per source k-mer, so it runs on the host like the candidate-error search of
// variants.cpp and in the same lockstep: all live searches advance by one pop of their queue per round, the neighbour
// keys they need go to the device in ONE kq_lookup_keys call on `db` (entries) and ONE on `sub` (seed membership), and they
// resume.  Visiting order, distances and the walk back from the destinations follow the reference statement by statement
// (line numbers cited below), including the order in which its Fibonacci heap hands out nodes of equal key.
// One map range is resident, so every search is "explored" (:574) the first time and no seed is searched twice.
#include "subgraph.h"

#include <algorithm>
#include <stdexcept>
#include <vector>

#include "graph_search.h"

namespace kqhost {

namespace {

struct Known { kq_entry e; bool in_db, in_sub; };                        // what a round's two lookups said about a key
using Cache = FlatMap<Known>;

struct Cand { uint64_t key; bool cont; };                                // neighbour + the direction a walk continues in behind it

struct Search {
    uint64_t source = 0;
    const kq_entry* source_entry = nullptr;                              // the merged subgraph entry (:470)
    NodeQueue Q;
    FlatMap<uint8_t> dist;
    FlatMap<std::pair<uint64_t, bool>> prev;
    std::vector<uint64_t> destinations;
    int depth = 0;
    bool direction = true, started = false, done = false, have_u = false;
    uint64_t u = 0;
    std::vector<Cand> cand;
};

void check(int rc) { if (rc != KQ_OK) throw std::runtime_error(std::string("Error: ") + kq_last_error()); }

// Runs one search until its next pop needs keys the cache does not hold (appended to `want`) or it is finished; a
// finished search appends what it discovered to `found`.
void advance(Search& s, const Cache& cache, int k, int kmer_depth, uint32_t cov_cutoff, std::vector<uint64_t>& want, std::vector<uint64_t>& found) {
    if (s.done) return;
    if (!s.started) {
        s.dist[s.source] = 1;                                            // :469-471
        s.Q.insert(s.source, 1);
        s.started = true;
    }
    if (!s.have_u) {
        if (!(s.Q.size() > 0 && s.depth < kmer_depth + 1)) {             // :477
            // the nodes on the prev chains of the destinations, source excluded (:563-570)
            for (uint64_t node : s.destinations) {
                while (node != s.source) {
                    found.push_back(node);
                    const auto* p = s.prev.find(node);
                    if (!p) break;                                       // (a chain of 254 nodes saturates dist: no prev)
                    node = p->first;
                }
            }
            s.done = true;
            s.dist.release(); s.prev.release(); s.Q = NodeQueue();
            std::vector<uint64_t>().swap(s.destinations);
            return;
        }
        s.u = s.Q.extract_min();                                         // :482
        if (const auto* got = s.prev.find(s.u)) s.direction = got->second;   // :483-486
        const kq_entry& nu = s.u == s.source ? *s.source_entry : cache.find(s.u)->e;
        s.cand.clear();
        for (int i = 0; i < 4; ++i) {                                    // :520-558, the two ifs in their order
            if (s.direction || s.depth == 0) {
                if (s.depth == 0) s.direction = true;
                if (nu.fw[i] > cov_cutoff) {
                    bool is_fw = false;
                    const uint64_t key = next_key(s.u, i, true, k, &is_fw);
                    s.cand.push_back(Cand{key, is_fw ? s.direction : !s.direction});
                }
            }
            if (!s.direction || s.depth == 0) {
                if (s.depth == 0) s.direction = false;
                if (nu.bw[i] > cov_cutoff) {
                    bool is_fw = false;
                    const uint64_t key = next_key(s.u, i, false, k, &is_fw);
                    s.cand.push_back(Cand{key, is_fw ? s.direction : !s.direction});
                }
            }
        }
        s.have_u = true;
    }
    bool missing = false;
    for (auto& c : s.cand) if (!cache.count(c.key)) { want.push_back(c.key); missing = true; }
    if (missing) return;                                                 // resumed after the round's lookups
    for (auto& c : s.cand) {                                             // checkNext :488-518
        const Known& n = *cache.find(c.key);
        if (n.in_sub) { s.destinations.push_back(s.u); continue; }       // :534-535, :552-553: the popped node is the destination
        if (!n.in_db) continue;                                          // the reference dereferences end() here (:497-498): not followed
        uint8_t alt = s.dist[s.u];
        if (alt < 255) ++alt;
        if (!s.dist.count(c.key)) { s.dist[c.key] = 255; s.Q.insert(c.key, 0); }
        if (alt < s.dist[c.key]) { s.prev[c.key] = std::make_pair(s.u, c.cont); s.dist[c.key] = alt; }   // decreaseKey: a no-op (alt > 0)
    }
    ++s.depth;                                                           // :559
    s.have_u = false;
}

}  // namespace

uint64_t subgraph_best_first(kq_handle* db, kq_handle* sub, int k, int map_count, int kmer_depth, uint32_t cov_cutoff, const std::function<void(const std::string&)>& log) {
    uint64_t n_seed = 0;
    check(kq_export(sub, 0, (uint16_t)map_count, nullptr, 0, &n_seed));
    std::vector<kq_entry> seeds((size_t)n_seed);
    if (n_seed) check(kq_export(sub, 0, (uint16_t)map_count, seeds.data(), n_seed, &n_seed));
    std::vector<uint64_t> found, want;
    std::vector<kq_entry> in_db, in_sub, add;
    Cache cache;
    size_t n_rounds = 0, n_keys = 0;
    const size_t kBatch = 1 << 16;
    for (size_t lo = 0; lo < seeds.size(); lo += kBatch) {
        const size_t hi = std::min(seeds.size(), lo + kBatch);
        std::vector<Search> searches(hi - lo);
        for (size_t i = lo; i < hi; ++i) { searches[i - lo].source = seeds[i].key; searches[i - lo].source_entry = &seeds[i]; }
        for (;;) {
            want.clear();
            bool any = false;
            for (auto& s : searches) { advance(s, cache, k, kmer_depth, cov_cutoff, want, found); any = any || !s.done; }
            if (!any) break;
            std::sort(want.begin(), want.end());
            want.erase(std::unique(want.begin(), want.end()), want.end());
            if (!want.empty()) {
                in_db.resize(want.size()); in_sub.resize(want.size());
                check(kq_lookup_keys(db, want.data(), want.size(), in_db.data()));
                check(kq_lookup_keys(sub, want.data(), want.size(), in_sub.data()));
                cache.reserve(cache.size() + want.size());
                for (size_t i = 0; i < want.size(); ++i) { Known& n = cache[want[i]]; n.e = in_db[i]; n.in_db = in_db[i].cov != 0; n.in_sub = in_sub[i].cov != 0; }
                ++n_rounds; n_keys += want.size();
            }
        }
        // discoveries of this batch, with their database entries, before the cache may go
        std::sort(found.begin(), found.end());
        found.erase(std::unique(found.begin(), found.end()), found.end());
        for (uint64_t key : found) add.push_back(cache.find(key)->e);
        found.clear();
        if (cache.size() > (1u << 24)) cache.clear();                    // bounded memory on large inputs
    }
    // inserted after all searches, without overwriting (:453): discoveries are never seeds, so a plain add of distinct keys
    std::sort(add.begin(), add.end(), [](const kq_entry& a, const kq_entry& b) { return a.key < b.key; });
    add.erase(std::unique(add.begin(), add.end(), [](const kq_entry& a, const kq_entry& b) { return a.key == b.key; }), add.end());
    if (!add.empty()) check(kq_import(sub, add.data(), add.size()));
    if (log) log("Best-first: " + std::to_string(seeds.size()) + " searches, " + std::to_string(n_rounds) + " lookup rounds, " + std::to_string(n_keys) + " keys fetched, " +
                 std::to_string(add.size()) + " k-mers added");
    return add.size();
}

}  // namespace kqhost
