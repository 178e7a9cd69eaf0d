// kq_nodequeue_core.h -- what the bounded graph searches share (kq_bestfirst_core.h: `kreeq subgraph` best-first;
// kq_variant_core.h: the candidate-error search of `validate -o vcf`): the node record, the head of a state block, NodeQueue
// of host/graph_search.h (the reference's include/fibonacci-heap.h) with the heap keys dropped, the key -> node number index
// and the k-mer step.  No HIP or project header: g++ reads this file as it is.
//
// The heap key is dropped.  In both searches the source is the only node inserted with key 1 and it is popped first, as the
// sole node of the queue.  Every other node is inserted with key 0 and decreaseKey never changes a key (alt >= 1 > 0 returns
// at include/fibonacci-heap.h:141).  So from the second pop on every comparison of two keys (:76, :152, :236) compares equal,
// and the one comparison before that (insert of the source into an empty queue) is decided by the queue being empty.
//
// Every loop has a bound derived from N, the node capacity of the block, and every node number is checked before it indexes
// the block: a corrupt state becomes an error code in Heap::err and ends the search, it does not loop or touch memory outside
// the block.
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
    uint8_t dist, degree, flags, emask;            // emask: the edge counters that qualify, bits 0-3 fw, 4-7 bw
    uint16_t pad;
};
struct Head {
    uint16_t n_nodes, n_found, err, pops;
    uint16_t pad[4];                               // (the candidate-error search keeps its counts here)
    uint16_t deg[DEG_SLOTS];
};
static_assert(sizeof(Node) == 24 && sizeof(Head) == 48, "state block layout");

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

// The queue and the index of one search over a pool of N nodes: `hd` (its degree table), `n` and `idx` (imask + 1 slots,
// a power of two at or above 2 N; a free slot holds NONE, a node number and never a key: at k = 32 a key has no spare bit
// pattern) point into the caller's state block.  The caller fills the index with 0xFF bytes before a search.
struct Heap {
    Head* hd; Node* n; uint16_t* idx;
    uint32_t N, imask, n_nodes = 0, count = 0, min = NONE, err = 0;

    KQ_BF_HD Heap(Head* hd_, Node* n_, uint16_t* idx_, uint32_t N_, uint32_t imask_) : hd(hd_), n(n_), idx(idx_), N(N_), imask(imask_) {}

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
};

}  // namespace kqbf
