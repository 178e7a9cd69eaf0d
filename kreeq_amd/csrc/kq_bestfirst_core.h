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
// The queue, the index and the node record are those of kq_nodequeue_core.h, which explains why the heap key is dropped.
//
// Every loop has a bound derived from N, and every node number is checked before it indexes the block: a corrupt state
// becomes an error code in Head::err and ends the search, it does not loop or touch memory outside the block.
#pragma once
#include "kq_nodequeue_core.h"

namespace kqbf {

constexpr int MAX_DEPTH = 255;                     // uint8_t in the reference (src/subgraph.cpp:460)

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

// G answers two questions about a key:
//   bool is_seed(uint64_t key) const      is it in the seed set?
//   int  db_mask(uint64_t key) const      -1: not in the database; else which of its eight LOGICAL edge counters are > cov_cutoff
template <class G>
struct Search : Heap {
    const G& g;
    int k;

    KQ_BF_HD Search(void* block, int depth, int k_, const G& g_)
        : Heap(head_of(block), nodes_of(block), index_of(block, depth), node_bound(depth), index_slots(depth) - 1), g(g_), k(k_) {}

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
