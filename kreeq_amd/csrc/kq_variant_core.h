// kq_variant_core.h -- ONE position's candidate-error search of `kreeq validate -o vcf` (reference DBG::searchVariants,
// src/variants.cpp:171-303, with the part of DBGtoVariants :53-169 that prepares it), written once for the kernels
// k_var_search / k_var_emit (kq_variants.h) and for a plain host program (tests/native/variant_core_main.cpp).  It restates
// advance() and the target window of host/variants.cpp statement by statement, on a caller-provided fixed-size state block
// instead of vectors and maps.  No HIP or project header: g++ reads this file as it is.  The queue, the key -> node index and
// the node record are those of kq_nodequeue_core.h (shared with kq_bestfirst_core.h); the argument for dropping the heap keys
// holds unchanged: the source is the only key-1 insert (:181) and is popped first, every other insert has key 0 (:219) and
// decreaseKey(alt >= 1) is a no-op.
//
// What one search is.  Position c of a segment (a run of ACGT with kcount k-mers) has the source k-mer c, the reference
// successor `ref` (k-mer c + 1, none at the last k-mer) and the targets: the k-mers starting at c+k+1 .. min(c+k+max_span,
// kcount-1), in that order (targets_queue; at max_span 0 it is the one k-mer c+k, see build_targets).  targetsMap carries the erase quirk of :104/:108 (a key is a target iff no
// occurrence of it left the window after its latest occurrence entered); ref_len of a destination counts from the FIRST
// occurrence of its key in the queue.  All of that is built here from the text, with a rolling 2-bit pack over k-mers
// c+k+2-max_span .. c+k+max_span (clamped to the segment; the erase test starts at k-mer k): there is no key array.
// Every pop follows ONE direction: the source's orientation at pop 0, later the `prev` direction of the popped node.  A
// candidate equal to `ref` is dropped first (:241).  A candidate that is a target never becomes a node: it gets
// prev[key] = (u, direction), overwriting, and is appended to the destinations (repeats kept).  A candidate that is neither a
// target nor in the table becomes a node without edges (G::edge_mask gives 0).  The paths are built after the loop from the
// FINAL prev, one per destination entry; the walk may run past the source, where prev of a key that has none is (0, false)
// and key 0 is looked up like any key -- it may be a node, a target or nothing.
//
// Why the state is bounded.  A search makes at most depth + 1 pops (:187) with at most 4 candidates each: with the source
// that is N = 5 + 4 depth nodes and 4 (depth + 1) destination entries; the window has at most max_span target slots.
//
// The limits: 0 <= depth <= 253, 0 <= max_span <= 255.  The depth bound is what makes `while (node != source)` (:271)
// terminate.  dist[source] = 1, and a node discovered at pop q gets alt <= q + 2 (induction: the node popped at pop q was
// discovered at a pop q' <= q - 1, so its dist is at most q' + 2 <= q + 1).  A node receives a prev only with alt < 255
// (:214-222).  A chain runs through POPPED nodes only (the first member of a prev pair is always the popped u), and the node
// of the last pop, pop `depth`, has alt <= depth + 1 at its discovery: depth <= 253 keeps that below 255, so every popped
// node but the source has a prev and every chain ends at the source.  (Nodes discovered AT pop 253 may saturate at 255 and
// stay without prev, but they are never popped.  "No alt ever reaches 255" would ask for depth <= 252; it is sufficient, not
// necessary.)  At depth 254 a straight chain leaves the node of the last pop without prev and the reference walks off
// through key 0 for ever.  max_span <= 255 keeps window offsets in a byte and the index of a target slot below NONE.
//
// The state block of one search (block_bytes(depth, max_span), a multiple of 8):
//   kqbf::Head          48 B   n_nodes, n_found = paths (= destination entries), err, pops, the degree table;
//                              pad[0] = target slots, pad[1] = the slot whose key is the source (NONE: none), pad[2..3] = the
//                              bytes of all path sequences (low, high half)
//   kqbf::Node[N]       24 B   as in kq_bestfirst_core.h: one node number serves dist, prev and the heap
//   Target[max(max_span, 1)] 16 B  one slot per DISTINCT key of the window, in order of first occurrence
//   uint16_t[4(depth+1)]       the destinations: target slot numbers
//   uint16_t[cap]              key -> node number, cap = the power of two at or above 2 N
// The caller fills the index with 0xFF bytes (NONE) before a search; everything else is initialised here.
//
// Every loop has a bound derived from the block, and every node, slot and destination number is checked before it indexes
// the block: a violated bound becomes an error code in Head::err and ends the search; it neither loops nor writes outside.
#pragma once
#include "kq_nodequeue_core.h"

namespace kqvar {

using kqbf::Head;
using kqbf::Node;
using kqbf::NONE;
using kqbf::PREV_DIR;

constexpr int MAX_DEPTH = 253;
constexpr int MAX_SPAN = 255;
enum : uint32_t {                                  // beside kqbf::ERR_*
    ERR_DEST = 64,     // more than 4 (depth + 1) destination entries
    ERR_TARGET = 128,  // a target slot number outside the window's slots
    ERR_TEXT = 256     // the position lies outside its segment
};
enum : uint8_t { VAR_SNV = 0, VAR_INS = 1, VAR_DEL = 2, VAR_COM = 3 };      // KQ_VAR_* of include/kreeq_amd.h

struct Target {
    uint64_t key;
    uint16_t prev;                                 // NONE until a pop reaches the key; then popped node | PREV_DIR (the pop's direction)
    uint8_t first, last;                           // first and latest occurrence in targets_queue
    uint8_t in_map, pad[3];                        // in targetsMap (the erase quirk)
};
static_assert(sizeof(Target) == 16, "state block layout");
struct Path { uint8_t type; uint16_t ref_len, seq_len; };

KQ_BF_HD inline uint32_t node_bound(int depth) { return 5u + 4u * (uint32_t)depth; }
KQ_BF_HD inline uint32_t dest_bound(int depth) { return 4u * ((uint32_t)depth + 1u); }
KQ_BF_HD inline uint32_t slot_bound(int span) { return span > 0 ? (uint32_t)span : 1u; }      // max_span 0: one target, see build_targets
KQ_BF_HD inline uint32_t index_slots(int depth) {
    uint32_t c = 32;
    for (int i = 0; i < 8 && c < 2 * node_bound(depth); ++i) c *= 2;      // 32 .. 2048 for depth 0 .. 253
    return c;
}
KQ_BF_HD inline size_t targets_at(int depth) { return sizeof(Head) + (size_t)node_bound(depth) * sizeof(Node); }
KQ_BF_HD inline size_t dests_at(int depth, int span) { return targets_at(depth) + (size_t)slot_bound(span) * sizeof(Target); }
KQ_BF_HD inline size_t index_at(int depth, int span) { return dests_at(depth, span) + (size_t)dest_bound(depth) * 2; }
KQ_BF_HD inline size_t block_bytes(int depth, int span) { return (index_at(depth, span) + (size_t)index_slots(depth) * 2 + 7) & ~(size_t)7; }
KQ_BF_HD inline Head* head_of(void* block) { return (Head*)block; }
KQ_BF_HD inline uint16_t* index_of(void* block, int depth, int span) { return (uint16_t*)((char*)block + index_at(depth, span)); }
KQ_BF_HD inline uint32_t seq_bytes_of(const Head* hd) { return (uint32_t)hd->pad[2] | (uint32_t)hd->pad[3] << 16; }

// G answers two questions:
//   uint32_t edge_mask(uint64_t key) const   the edges of `key` that the search follows, with the precedence quirk of :237
//                                            (`direction ? fw[i] : bw[i] > covCutOff`): bit i = fw[i] != 0, bit 4 + i =
//                                            bw[i] > cov_cutoff, LOGICAL counters; 0 for a key that is not in the table
//   uint32_t base(uint64_t p) const          the 2-bit code of base p of the SEGMENT (0 <= p < kcount + k - 1)
template <class G>
struct Search : kqbf::Heap {
    static constexpr uint32_t TGT = 0x4000u, ABSENT = 0x8000u;           // a walk stands on a node (its number), a target slot (TGT | slot) or on key 0 that nothing holds
    Target* T; uint16_t* dest;
    const G& g;
    int k;
    uint32_t S, TS, D, n_t = 0, n_dest = 0, src_slot = NONE;
    uint64_t source = 0, kmask;

    KQ_BF_HD Search(void* block, int depth, int span, int k_, const G& g_)
        : Heap(head_of(block), (Node*)((char*)block + sizeof(Head)), index_of(block, depth, span), node_bound(depth), index_slots(depth) - 1),
          T((Target*)((char*)block + targets_at(depth))), dest((uint16_t*)((char*)block + dests_at(depth, span))), g(g_), k(k_), S((uint32_t)span), TS(slot_bound(span)),
          D(dest_bound(depth)), kmask(k_ == 32 ? ~0ull : (1ull << (2 * k_)) - 1) {}

    KQ_BF_HD Target& tgt(uint32_t t) {                                   // every slot number passes here before it indexes the block
        if (t >= n_t) { err |= ERR_TARGET; t = 0; }
        return T[t];
    }

    // ---- the rolling 2-bit pack: k-mer p of the segment and its reverse complement ----
    struct Roll { uint64_t fw, rv; };
    KQ_BF_HD Roll roll_at(uint64_t p) const {
        Roll r{0, 0};
        for (int j = 0; j < k; ++j) { const uint64_t c = g.base(p + (uint64_t)j) & 3u; r.fw |= c << (2 * j); r.rv |= (3 - c) << (2 * (k - 1 - j)); }
        return r;
    }
    KQ_BF_HD void roll_step(Roll& r, uint64_t p_next) const {            // -> the k-mer that ENDS at base p_next
        const uint64_t c = g.base(p_next) & 3u;
        r.fw = (r.fw >> 2) | c << (2 * k - 2);
        r.rv = ((r.rv << 2) | (3 - c)) & kmask;
    }
    static KQ_BF_HD uint64_t canon(const Roll& r) { return r.fw < r.rv ? r.fw : r.rv; }

    // the slot of a key that is in targetsMap, or NONE
    KQ_BF_HD uint32_t target_of(uint64_t key) const {
        for (uint32_t t = 0; t < n_t; ++t) if (T[t].key == key && T[t].in_map) return t;
        return NONE;
    }

    // targets_queue and targetsMap while position c is processed (host/variants.cpp find_candidate_errors, reference :92-110)
    KQ_BF_HD void build_targets(uint64_t c, uint64_t kcount) {
        // max_span 0: the reference pops an EMPTY queue (:104-105, undefined) and then pushes k-mer c + k (:106-110).  The
        // Read as "the pop is skipped" (the suite's CPU restatement does the same), the queue holds that one k-mer while c is processed.
        const uint64_t w_lo = c + (uint64_t)k + (S ? 1 : 0);
        if (w_lo >= kcount) return;                                      // empty window (also every segment with kcount <= k + 1)
        const uint64_t w_hi = c + (uint64_t)k + S < kcount - 1 ? c + (uint64_t)k + S : kcount - 1;
        Roll r = roll_at(w_lo);
        for (uint64_t t = w_lo; t <= w_hi; ++t) {                        // at most S rounds
            if (t > w_lo) roll_step(r, t + (uint64_t)k - 1);
            const uint64_t key = canon(r);
            const uint8_t off = (uint8_t)(t - w_lo);
            uint32_t s = 0;
            while (s < n_t && T[s].key != key) ++s;
            if (s < n_t) { T[s].last = off; continue; }
            if (n_t >= TS) { err |= ERR_TARGET; return; }                // cannot happen: at most max(S, 1) k-mers in the window
            Target& x = T[n_t++];
            x.key = key; x.prev = (uint16_t)NONE; x.first = x.last = off; x.in_map = 1; x.pad[0] = x.pad[1] = x.pad[2] = 0;
        }
        // the erase quirk: an occurrence at t1 <= c + k left the window; it took the key along unless the key's latest
        // occurrence t_max entered after that, i.e. unless t1 < t_max - S + 1
        if (S == 0) return;                                              // the one k-mer was pushed after the pop
        const uint64_t hi1 = c + (uint64_t)k;
        uint64_t lo1 = w_lo + 1 > S ? w_lo + 1 - S : 0;                  // the smallest `from` any slot can have
        if (lo1 < (uint64_t)k) lo1 = (uint64_t)k;
        if (lo1 > hi1) return;
        r = roll_at(lo1);
        for (uint64_t t1 = lo1; t1 <= hi1; ++t1) {                       // at most S rounds
            if (t1 > lo1) roll_step(r, t1 + (uint64_t)k - 1);
            const uint64_t key = canon(r);
            for (uint32_t s = 0; s < n_t; ++s) {
                if (T[s].key != key) continue;
                const uint64_t t_max = w_lo + T[s].last, from = t_max >= S ? t_max - S + 1 : 0;
                if (t1 >= from) T[s].in_map = 0;
            }
        }
    }

    // checkNext :197-228 and :247-260 for the candidate `key` of the popped node u, which is followed in `direction`
    KQ_BF_HD void candidate(uint32_t u, uint64_t key, bool is_fw, bool direction) {
        const uint32_t t = target_of(key);
        if (t != NONE) {                                                 // :255-258: a target is never a node
            T[t].prev = (uint16_t)(u | (direction ? PREV_DIR : 0u));
            if (n_dest >= D) { err |= ERR_DEST; return; }
            dest[n_dest++] = (uint16_t)t;
            return;
        }
        uint32_t slot = 0;
        uint32_t j = lookup(key, &slot);
        if (err) return;
        if (j == NONE) {
            if (n_nodes >= N) { err |= kqbf::ERR_POOL; return; }
            j = n_nodes++;
            Node& nj = n[j];
            nj.key = key; nj.prev = (uint16_t)NONE; nj.dist = 255; nj.flags = 0; nj.emask = (uint8_t)g.edge_mask(key); nj.pad = 0;      // :216-219
            idx[slot] = (uint16_t)j;
            heap_insert(j);
        }
        const bool cont = is_fw ? direction : !direction;
        uint32_t alt = at(u).dist;
        if (alt < 255) ++alt;
        if (alt < at(j).dist) { at(j).prev = (uint16_t)(u | (cont ? PREV_DIR : 0u)); at(j).dist = (uint8_t)alt; }      // decreaseKey: a no-op (alt > 0)
    }

    // ---- the walk over the final prev map, which is keyed by k-mer ----
    KQ_BF_HD uint64_t key_of(uint32_t cur) { return cur == ABSENT ? 0 : (cur & TGT) ? tgt(cur & ~TGT).key : at(cur).key; }
    KQ_BF_HD uint32_t prev_word(uint32_t cur) {
        if (cur == ABSENT) return NONE;
        if (cur & TGT) return tgt(cur & ~TGT).prev;
        if (cur == 0 && src_slot != NONE && tgt(src_slot).prev != NONE) return tgt(src_slot).prev;      // the source's key was reached as a target
        return at(cur).prev;
    }
    // prev_of(cur): -> .first, *second = .second; a key without prev gives (0, false), and key 0 is looked up like any key
    KQ_BF_HD uint32_t back(uint32_t cur, bool* second) {
        const uint32_t p = prev_word(cur);
        if (p != NONE) { *second = (p & PREV_DIR) != 0; return p & ~(uint32_t)PREV_DIR; }
        *second = false;
        const uint32_t t = target_of(0);
        if (t != NONE) return TGT | t;
        uint32_t slot = 0;
        const uint32_t j = lookup(0, &slot);
        return j == NONE ? ABSENT : j;
    }
    // destination entry d -> its path (:266-303); out (may be null) receives seq_len bases.  false: the search has an error code
    KQ_BF_HD bool path(uint32_t d, Path* p, char* out) {
        p->type = 0; p->ref_len = 0; p->seq_len = 0;
        if (d >= n_dest || d >= D) { err |= ERR_DEST; return false; }
        const uint32_t t = dest[d];
        const int ref_len = (int)tgt(t).first + k;                       // std::find: the first occurrence
        bool dirn = false, unused = false;
        int i = 0;
        uint32_t node = back(TGT | t, &unused);
        while (key_of(node) != source && !err) {                         // :271
            if ((uint32_t)i >= N) { err |= kqbf::ERR_CHAIN; break; }
            node = back(node, &unused); ++i;
        }
        if (err) return false;
        node = back(TGT | t, &unused);
        (void)back(node, &dirn);
        int b = i - ref_len;
        if (ref_len > k) { p->type = VAR_COM; p->ref_len = (uint16_t)(ref_len - k + 1); b = ref_len - k; }
        else if (i == ref_len) p->type = VAR_SNV;
        else if (i > ref_len) { p->type = VAR_DEL; --b; node = back(node, &unused); (void)back(node, &dirn); }
        else p->type = VAR_INS;
        const int len = b >= 0 ? b + 1 : 0;                              // <= max(max_span, depth + 1)
        p->seq_len = (uint16_t)len;
        for (int j = 0; j < len && out && !err; ++j) {                   // written back to front: the reference reverses (:300)
            const uint64_t key = key_of(node);
            const uint32_t code = dirn ? (uint32_t)(key & 3u) : 3u - (uint32_t)((key >> (2 * k - 2)) & 3u);
            out[len - 1 - j] = (char)((0x54474341u >> (8 * code)) & 0xFFu);      // "ACGT"[code]
            node = back(node, &unused);
            (void)back(node, &dirn);
        }
        return !err;
    }

    // the whole search of position c of a segment with kcount k-mers -> the number of paths
    KQ_BF_HD uint32_t run(uint64_t c, uint64_t kcount, int depth) {
        uint64_t ref = 0;
        bool has_ref = false, source_fw = false;
        if (c >= kcount) err |= ERR_TEXT;
        else {
            Roll r = roll_at(c);                                         // :114
            source = canon(r); source_fw = r.fw < r.rv;
            if (c + 1 < kcount) { roll_step(r, c + (uint64_t)k); ref = canon(r); has_ref = true; }
            build_targets(c, kcount);
            src_slot = target_of(source);
        }
        uint32_t d = 0;
        if (!err) {
            uint32_t slot = 0;
            lookup(source, &slot);                                       // (empty index: the free home slot)
            n_nodes = 1;
            Node& s = n[0];
            s.key = source; s.prev = (uint16_t)NONE; s.dist = 1; s.flags = 0; s.emask = (uint8_t)g.edge_mask(source); s.pad = 0;      // :180-181
            if (!err) idx[slot] = 0;
            heap_insert(0);
        }
        bool direction = true;
        while (!err && count > 0 && d < (uint32_t)depth + 1) {           // :187
            const uint32_t u = extract_min();                            // :192
            if (err) break;
            const uint32_t pw = prev_word(u);                            // :193-196
            if (pw != NONE) direction = (pw & PREV_DIR) != 0;
            if (d == 0) direction = source_fw;                           // :233
            const uint32_t m = at(u).emask;
            const uint64_t ukey = at(u).key;
            for (uint32_t i = 0; i < 4 && !err; ++i) {                   // :232-260; a candidate depends on u alone, so it is handled where it is found
                if (!((m >> (direction ? i : 4 + i)) & 1u)) continue;    // :237
                bool is_fw = false;
                const uint64_t key = kqbf::next_key(ukey, i, direction, k, &is_fw);
                if (has_ref && key == ref) continue;                     // :241: the reference path is never rediscovered
                candidate(u, key, is_fw, direction);
            }
            ++d;                                                         // :261
        }
        uint32_t seq_bytes = 0;
        for (uint32_t e = 0; e < n_dest && !err; ++e) { Path p; if (path(e, &p, nullptr)) seq_bytes += p.seq_len; }
        if (err) { n_dest = 0; n_nodes = 0; seq_bytes = 0; }             // nothing of a failed search is emitted
        hd->n_nodes = (uint16_t)n_nodes; hd->n_found = (uint16_t)n_dest; hd->err = (uint16_t)err; hd->pops = (uint16_t)d;
        hd->pad[0] = (uint16_t)n_t; hd->pad[1] = (uint16_t)src_slot; hd->pad[2] = (uint16_t)(seq_bytes & 0xFFFFu); hd->pad[3] = (uint16_t)(seq_bytes >> 16);
        return n_dest;
    }

    // takes up the block of a finished search, for path()
    KQ_BF_HD void reopen() {
        n_nodes = hd->n_nodes; n_dest = hd->n_found; err = hd->err; n_t = hd->pad[0]; src_slot = hd->pad[1];
        if (n_nodes > N || n_dest > D || n_t > TS || (src_slot != NONE && src_slot >= n_t)) {      // not a head that run() wrote
            err |= kqbf::ERR_LINK; n_nodes = 0; n_dest = 0; n_t = 0; src_slot = NONE;
        }
        source = n_nodes ? n[0].key : 0;
    }
};

// One position's search in `block` (block_bytes(depth, span) bytes, 8-byte aligned, index filled with 0xFF).  Returns the
// number of paths; head_of(block)->err != 0: the search failed.  seq_bytes_of(head) is the sum of their sequence lengths.
template <class G>
KQ_BF_HD inline uint32_t search(void* block, int depth, int span, int k, uint64_t c, uint64_t kcount, const G& g) {
    Search<G> s(block, depth, span, k, g);
    return s.run(c, kcount, depth);
}
// Path d (< the count search() returned) of the finished search in `block`; out: room for its sequence, or null.
template <class G>
KQ_BF_HD inline bool path(void* block, int depth, int span, int k, uint32_t d, const G& g, Path* p, char* out) {
    Search<G> s(block, depth, span, k, g);
    s.reopen();
    return s.path(d, p, out);
}

}  // namespace kqvar
