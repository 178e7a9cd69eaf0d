// kq_bestfirst_core.h -- ONE source's best-first search of `kreeq subgraph` (reference DBG::dijkstra, src/subgraph.cpp:460-579),
// written once for the kernel k_sg_bf_search (kq_subgraph.h) and for a plain host program (tests/native/bestfirst_core_main.cpp).
// It restates advance() of host/subgraph.cpp and NodeQueue of host/graph_search.h statement by statement, on a caller-provided
// fixed-size state block instead of vectors and maps.  No HIP or project header: g++ reads this file as it is.
//
// Why the state is bounded.  A search makes at most depth + 1 pops (:477).  Pop 0 follows both directions of the source, so it
// inserts at most 8 nodes; every later pop follows one direction, so it inserts at most 4.  With the source itself that is
// N = 9 + 4 depth nodes, depth <= 255: N <= 1029, and 16-bit node numbers suffice.
//
// The state block of one search (block_bytes(depth), a multiple of 8):
//   Head            48 B    node count, result count, error code, the 16-entry degree table of consolidate
//   Node[N]         24 B    one record per key the search has met: a key enters `dist` and the queue in the same statement
//                           (:507-509), so ONE node number serves the dist map, the prev map and the heap's index pool
//   uint16_t[cap]           key -> node number, open addressing, cap = the power of two at or above 2 N; a free slot holds
//                           NONE, a node number and never a key (at k = 32 a key has no spare bit pattern)
// The caller fills the index with 0xFF bytes (NONE) before a search; everything else is initialised here.
//
// The heap key is dropped.  The source is the only node inserted with key 1 (:471) and it is popped first, as the sole node of
// the queue.  Every other node is inserted with key 0 (:509) and decreaseKey never changes a key (alt >= 1 > 0 returns at
// include/fibonacci-heap.h:141).  So from the second pop on every comparison of two keys (:76, :152, :236) compares equal, and
// the one comparison before that (insert of the source into an empty queue) is decided by the queue being empty.
//
// Every loop has a bound derived from N, and every node number is checked before it indexes the block: a corrupt state
// becomes an error code in Head::err and ends the search, it does not loop or touch memory outside the block.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KQ_BF_HD __host__ __device__
#else
#define KQ_BF_HD
#endif

namespace kqbf {

constexpr uint32_t NONE = 0xFFFFu;                 // "no node": free index slot, no prev, no parent / child, empty queue
constexpr int MAX_DEPTH = 255;                     // uint8_t in the reference (src/subgraph.cpp:460)
constexpr uint32_t DEG_SLOTS = 16;                 // a Fibonacci heap of n nodes has degrees <= log_phi n: 14 for n = 1029

enum : uint32_t {
    ERR_POOL = 1,      // more than N nodes
    ERR_INDEX = 2,     // an index probe visited every slot
    ERR_ROOTS = 4,     // a root list longer than N
    ERR_DEGREE = 8,    // a degree >= DEG_SLOTS
    ERR_CHAIN = 16,    // a prev chain longer than N
    ERR_LINK = 32      // a node number outside the pool
};
enum : uint8_t { F_MARK = 1, F_DEST = 2, F_FOUND = 4 };      // heap mark; a destination (:534, :552); on a destination's prev chain
constexpr uint16_t PREV_DIR = 0x8000u;             // prev = node number | PREV_DIR when the walk continues forward behind it

struct Node {
    uint64_t key;
    uint16_t left, right, parent, child;           // include/fibonacci-heap.h:13-21
    uint16_t prev;                                 // NONE: no prev (the source, or dist saturated at 255)
    uint8_t dist, degree, flags, emask;            // emask: edge counters > cov_cutoff, bits 0-3 fw, 4-7 bw
    uint16_t pad;
};
struct Head {
    uint16_t n_nodes, n_found, err, pops;
    uint16_t pad[4];
    uint16_t deg[DEG_SLOTS];
};
static_assert(sizeof(Node) == 24 && sizeof(Head) == 48, "state block layout");

KQ_BF_HD inline uint32_t node_bound(int depth) { return 9u + 4u * (uint32_t)depth; }
KQ_BF_HD inline uint32_t index_slots(int depth) {
    uint32_t c = 32;
    for (int i = 0; i < 8 && c < 2 * node_bound(depth); ++i) c *= 2;      // 32 .. 4096 for depth 0 .. 255
    return c;
}
KQ_BF_HD inline size_t block_bytes(int depth) {
    return (sizeof(Head) + (size_t)node_bound(depth) * sizeof(Node) + (size_t)index_slots(depth) * 2 + 7) & ~(size_t)7;
}
KQ_BF_HD inline Head* head_of(void* block) { return (Head*)block; }
KQ_BF_HD inline Node* nodes_of(void* block) { return (Node*)((char*)block + sizeof(Head)); }
KQ_BF_HD inline uint16_t* index_of(void* block, int depth) { return (uint16_t*)((char*)block + sizeof(Head) + (size_t)node_bound(depth) * sizeof(Node)); }

// reverse complement of a 2-bit packed k-mer, first base in the low bits
KQ_BF_HD inline uint64_t revcomp(uint64_t fw, int k) {
    uint64_t x = ~fw;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    x = (x >> 32) | (x << 32);
    return x >> (64 - 2 * k);
}
// DBG::buildNextKmer + hash, src/subgraph.cpp:581-597: the k-mer one step along edge `base` of the canonical string of `key`
KQ_BF_HD inline uint64_t next_key(uint64_t key, uint32_t base, bool fw, int k, bool* is_fw) {
    const uint64_t kmask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1;
    const uint64_t nxt = fw ? (key >> 2) | ((uint64_t)base << (2 * k - 2)) : ((key << 2) | base) & kmask;
    const uint64_t rv = revcomp(nxt, k);
    *is_fw = nxt < rv;
    return nxt < rv ? nxt : rv;
}

// G answers two questions about a key:
//   bool is_seed(uint64_t key) const      is it in the seed set?
//   int  db_mask(uint64_t key) const      -1: not in the database; else which of its eight LOGICAL edge counters are > cov_cutoff
template <class G>
struct Search {
    Head* hd; Node* n; uint16_t* idx;
    uint32_t N, imask, n_nodes = 0, count = 0, min = NONE, err = 0;
    const G& g;
    int k;

    KQ_BF_HD Search(void* block, int depth, int k_, const G& g_)
        : hd(head_of(block)), n(nodes_of(block)), idx(index_of(block, depth)), N(node_bound(depth)), imask(index_slots(depth) - 1), g(g_), k(k_) {}

    KQ_BF_HD Node& at(uint32_t x) {                                      // every node number passes here before it indexes the block
        if (x >= N) { err |= ERR_LINK; x = 0; }
        return n[x];
    }

    // ---- NodeQueue of host/graph_search.h (include/fibonacci-heap.h), keys dropped ----
    KQ_BF_HD void to_root(uint32_t x) {                                  // _existingToRoot :145-164
        at(x).parent = (uint16_t)NONE; at(x).flags &= (uint8_t)~F_MARK;
        if (min != NONE) {
            const uint32_t ml = at(min).left;
            at(min).left = (uint16_t)x; at(x).right = (uint16_t)min; at(x).left = (uint16_t)ml; at(ml).right = (uint16_t)x;
        } else { min = x; at(x).left = at(x).right = (uint16_t)x; }
    }
    KQ_BF_HD void unlink(uint32_t x) {                                   // _removeNodeFromRoot :165-179
        if (at(x).right != x) { at(at(x).right).left = at(x).left; at(at(x).left).right = at(x).right; }
        const uint32_t p = at(x).parent;
        if (p != NONE) {
            at(p).child = at(p).degree == 1 ? (uint16_t)NONE : at(x).right;
            --at(p).degree;
        }
    }
    KQ_BF_HD void add_child(uint32_t p, uint32_t c) {                    // _addChild :184-201
        if (at(p).degree == 0) { at(p).child = (uint16_t)c; at(c).left = at(c).right = (uint16_t)c; }
        else {
            const uint32_t c1 = at(p).child, l = at(c1).left;
            at(c1).left = (uint16_t)c; at(c).right = (uint16_t)c1; at(c).left = (uint16_t)l; at(l).right = (uint16_t)c;
        }
        at(c).parent = (uint16_t)p; ++at(p).degree;
    }
    KQ_BF_HD void consolidate() {                                        // :218-268
        if (count <= 1) return;
        for (uint32_t d = 0; d < DEG_SLOTS; ++d) hd->deg[d] = (uint16_t)NONE;
        uint32_t roots = 0, it = min;
        do { ++roots; it = at(it).right; } while (it != min && roots <= N);
        if (roots > N) { err |= ERR_ROOTS; return; }
        uint32_t cur = min;
        for (uint32_t r = 0; r < roots && !err; ++r) {
            const uint32_t x = cur;
            cur = at(cur).right;
            uint32_t d = at(x).degree;
            for (;;) {                                                   // at most DEG_SLOTS rounds: d grows or the loop ends
                if (d >= DEG_SLOTS) { err |= ERR_DEGREE; return; }
                if (hd->deg[d] == NONE) { hd->deg[d] = (uint16_t)x; break; }
                const uint32_t y = hd->deg[d];                           // (equal keys: x stays the parent, :236)
                if (y == x) break;
                unlink(y); add_child(x, y); at(y).flags &= (uint8_t)~F_MARK;      // _link
                hd->deg[d] = (uint16_t)NONE;
                ++d;
            }
        }
        min = NONE;
        for (uint32_t d = 0; d < DEG_SLOTS; ++d) if (hd->deg[d] != NONE) to_root(hd->deg[d]);
    }
    KQ_BF_HD void heap_insert(uint32_t x) {                              // :57-86
        Node& nx = at(x);
        nx.degree = 0; nx.parent = (uint16_t)NONE; nx.child = (uint16_t)NONE; nx.left = nx.right = (uint16_t)x; nx.flags &= (uint8_t)~F_MARK;
        if (min != NONE) { const uint32_t ml = at(min).left; at(min).left = (uint16_t)x; nx.right = (uint16_t)min; nx.left = (uint16_t)ml; at(ml).right = (uint16_t)x; }
        else min = x;
        ++count;
    }
    KQ_BF_HD uint32_t extract_min() {                                    // :87-126
        const uint32_t m = min;
        uint32_t c = at(m).child;
        const uint32_t dg = at(m).degree;
        if (dg >= DEG_SLOTS) { err |= ERR_DEGREE; return m; }
        for (uint32_t i = 0; i < dg; ++i) { const uint32_t rem = c; c = at(c).right; to_root(rem); }
        unlink(m);
        --count;
        if (count == 0) min = NONE;
        else {
            min = at(m).right;
            const uint32_t ml = at(m).left;
            at(min).left = (uint16_t)ml; at(ml).right = (uint16_t)min;
            consolidate();
        }
        return m;
    }

    // ---- key -> node number ----
    // the key's node, or NONE with *slot = the free slot where it would go
    KQ_BF_HD uint32_t lookup(uint64_t key, uint32_t* slot) {
        uint64_t h = key * 0x9E3779B97F4A7C15ull;
        uint32_t i = (uint32_t)(h >> 40) & imask;
        for (uint32_t probe = 0; probe <= imask; ++probe, i = (i + 1) & imask) {
            const uint32_t s = idx[i];
            if (s == NONE) { *slot = i; return NONE; }
            if (s >= n_nodes) { err |= ERR_LINK; return NONE; }
            if (n[s].key == key) return s;
        }
        err |= ERR_INDEX;
        return NONE;
    }

    // checkNext :488-518 for the neighbour `key` of the popped node u; `cont`: the direction a walk continues in behind it
    KQ_BF_HD void check_next(uint32_t u, uint64_t key, bool cont) {
        uint32_t slot = 0;
        uint32_t j = lookup(key, &slot);
        if (err) return;
        if (j == NONE) {
            if (g.is_seed(key)) { at(u).flags |= F_DEST; return; }       // :534-535, :552-553: the popped node is the destination
            const int m = g.db_mask(key);
            if (m < 0) return;                                           // the reference dereferences end() here (:497-498): not followed
            if (n_nodes >= N) { err |= ERR_POOL; return; }
            j = n_nodes++;
            Node& nj = n[j];
            nj.key = key; nj.prev = (uint16_t)NONE; nj.dist = 255; nj.flags = 0; nj.emask = (uint8_t)m; nj.pad = 0;      // :507-509
            idx[slot] = (uint16_t)j;
            heap_insert(j);
        } else if (j == 0) { at(u).flags |= F_DEST; return; }            // the source: the one node that is a seed
        uint32_t alt = at(u).dist;
        if (alt < 255) ++alt;
        if (alt < at(j).dist) { at(j).prev = (uint16_t)(u | (cont ? PREV_DIR : 0u)); at(j).dist = (uint8_t)alt; }      // decreaseKey: a no-op (alt > 0)
    }

    // the whole search of `source`, whose edge mask comes from its merged subgraph entry (:470) -> nodes flagged F_FOUND
    KQ_BF_HD uint32_t run(uint64_t source, uint32_t source_mask, int depth) {
        uint32_t slot = 0;
        lookup(source, &slot);                                           // (empty index: the free home slot)
        n_nodes = 1;
        Node& s = n[0];
        s.key = source; s.prev = (uint16_t)NONE; s.dist = 1; s.flags = 0; s.emask = (uint8_t)source_mask; s.pad = 0;     // :469-471
        if (!err) idx[slot] = 0;
        heap_insert(0);
        uint32_t d = 0;
        bool direction = true;
        while (!err && count > 0 && d < (uint32_t)depth + 1) {           // :477
            const uint32_t u = extract_min();                            // :482
            if (err) break;
            if (at(u).prev != NONE) direction = (at(u).prev & PREV_DIR) != 0;      // :483-486
            const uint32_t m = at(u).emask;
            const uint64_t ukey = at(u).key;
            for (uint32_t i = 0; i < 4 && !err; ++i) {                   // :520-558, the two ifs in their order
                if (direction || d == 0) {
                    if (d == 0) direction = true;
                    if ((m >> i) & 1u) {
                        bool is_fw = false;
                        const uint64_t key = next_key(ukey, i, true, k, &is_fw);
                        check_next(u, key, is_fw ? direction : !direction);
                    }
                }
                if (!direction || d == 0) {
                    if (d == 0) direction = false;
                    if ((m >> (4 + i)) & 1u) {
                        bool is_fw = false;
                        const uint64_t key = next_key(ukey, i, false, k, &is_fw);
                        check_next(u, key, is_fw ? direction : !direction);
                    }
                }
            }
            ++d;                                                         // :559
        }
        // the nodes on the prev chains of the destinations, source excluded (:563-570)
        uint32_t n_found = 0;
        for (uint32_t j = 1; j < n_nodes && !err; ++j) {
            if (!(n[j].flags & F_DEST)) continue;
            uint32_t node = j, steps = 0;
            while (node != 0 && !(at(node).flags & F_FOUND)) {
                if (++steps > N) { err |= ERR_CHAIN; break; }
                at(node).flags |= F_FOUND; ++n_found;
                const uint32_t p = at(node).prev;
                if (p == NONE) break;                                    // (a chain of 254 nodes saturates dist: no prev)
                node = p & ~(uint32_t)PREV_DIR;
            }
        }
        if (err) { n_found = 0; n_nodes = 0; }                           // nothing of a failed search is collected
        hd->n_nodes = (uint16_t)n_nodes; hd->n_found = (uint16_t)n_found; hd->err = (uint16_t)err; hd->pops = (uint16_t)d;
        return n_found;
    }
};

// One source's search in `block` (block_bytes(depth) bytes, 8-byte aligned, index filled with 0xFF).  Returns the number of
// k-mers it discovered: the nodes i < head_of(block)->n_nodes with F_FOUND.  head_of(block)->err != 0: the search failed.
template <class G>
KQ_BF_HD inline uint32_t search(void* block, int depth, int k, uint64_t source, uint32_t source_mask, const G& g) {
    Search<G> s(block, depth, k, g);
    return s.run(source, source_mask, depth);
}

}  // namespace kqbf
