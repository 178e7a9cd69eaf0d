// kq_gfa.h -- kernels of kq_subgraph_gfa: the trimmed subgraph table as the graph the reference hands to its GFA writer
// (DBG::DBGgraphToGFA / DBG::collapseNodes, reference src/kreeq.cpp:360-600): non-branching runs of k-mers compacted into
// unitigs, every other edge counter a link.  gfx950 only.  Host side: kq_subgraph_gfa in kreeq_amd.hip; the rules, with the
// reference lines they restate, are spelled out in tests/gfa_ref.py, and DESIGN.md §8c says where they leave the reference.
//
// The input is the table's entries in ascending key order (ents[n]; keys[n] the same keys alone, for the bisection that turns a
// neighbour key into its rank).  An ORIENTED k-mer has the id v = 2 * rank + rc: (x,+) is the canonical string of key x, (x,-)
// its reverse complement, flip(v) = v ^ 1.  The out-edges of (x,+) are the non-zero fw counters, those of (x,-) the non-zero
// bw counters.
//   k_gfa_links     succ[v]: the link v -> w (v has one out-edge, w is present, another key, no palindromes, and flip(w) has one
//                   out-edge, which leads to flip(v)).  The rule is its own mirror: succ[flip(w)] = flip(v), so the
//                   predecessor of v is flip(succ[flip(v)]) and needs no scatter.
//   k_gfa_rank_*    pointer jumping over the predecessors, double-buffered: per oriented k-mer the head of its chain, its
//                   distance from it and the smallest id seen.  1 + ceil(log2(2n)) rounds at most; what still has a live
//                   pointer then is on a cycle.  k_gfa_cut opens every cycle pair once -- in front of the smallest id of the
//                   two cycles and, in the mirror cycle, behind its flip -- and the ranking runs again.
//   k_gfa_heads     keep flag (head id < the mirror chain's head id) and length per chain head; two prefix sums number the
//                   segments and place their sequences.
//   k_gfa_segments  one work item per oriented k-mer of a kept chain: the head writes the record and k bases, the others one.
//   k_gfa_edges     one work item per (oriented k-mer, base): <false> flags the records, <true> writes them where the prefix
//                   sum of the flags says.
// No kernel waits for another workgroup, every loop is bounded, every index is compared with its bound before it is used;
// a violated bound sets a bit of GfaState::err, which fails the call.  Everything here is a gather over random ranks:
// one item per thread at full occupancy, as in kq_subgraph.h.
#pragma once
#include "kq_subgraph.h"

namespace kq {

constexpr uint32_t GFA_NONE = 0xFFFFFFFFu;
enum : uint32_t { GFA_ERR_INDEX = 1, GFA_ERR_MIRROR = 2, GFA_ERR_OUTPUT = 4 };

struct GfaNode { uint32_t ptr, head, dist, mn; };      // live predecessor pointer (GFA_NONE: head holds the chain's head), distance to it, smallest id on the way
struct GfaState { unsigned long long n_dropped, n_cycles; unsigned int changed, err; };

// rank of `key` in the ascending keys[n], GFA_NONE when absent (n < 2^31: 32 halvings end the search)
__device__ __forceinline__ uint32_t gfa_rank(const uint64_t* __restrict__ keys, uint32_t n, uint64_t key) {
    uint32_t lo = 0, hi = n;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && keys[lo] == key ? lo : GFA_NONE;
}
// the oriented k-mer one step along out-edge `base` of the oriented k-mer (key, rc) -> its key, *minus = its orientation
// ((x,+): '+' iff isFw; (x,-): '-' iff isFw; src/kreeq.cpp:566, :589).  The key is sg_neighbour's.
__device__ __forceinline__ uint64_t gfa_step(uint64_t key, uint32_t rc, uint32_t base, uint32_t k, uint32_t* minus) {
    const uint64_t kmask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1;
    const uint64_t nxt = rc ? ((key << 2) | base) & kmask : (key >> 2) | ((uint64_t)base << (2 * k - 2));
    const uint64_t rv = revcomp2(nxt, (int)k);
    const bool is_fw = nxt < rv;
    *minus = rc ? (uint32_t)is_fw : (uint32_t)!is_fw;
    return is_fw ? nxt : rv;
}
__device__ __forceinline__ uint32_t gfa_counter(const kq_entry& e, uint32_t rc, uint32_t base) { return rc ? e.bw[base] : e.fw[base]; }
// number of out-edges of an oriented k-mer, *base = the last one
__device__ __forceinline__ uint32_t gfa_out_degree(const kq_entry& e, uint32_t rc, uint32_t* base) {
    uint32_t n = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) if (gfa_counter(e, rc, i) != 0) { ++n; *base = i; }
    return n;
}
// the string of an oriented k-mer as a key (first base in the low bits)
__device__ __forceinline__ uint64_t gfa_oriented(uint64_t key, uint32_t rc, uint32_t k) { return rc ? revcomp2(key, (int)k) : key; }

__global__ __launch_bounds__(256) void k_gfa_keys(const kq_entry* __restrict__ ents, uint32_t n, uint64_t* __restrict__ keys) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) keys[i] = ents[i].key;
}

__global__ __launch_bounds__(256) void k_gfa_links(const kq_entry* __restrict__ ents, const uint64_t* __restrict__ keys, uint32_t n, uint32_t k,
                                                    uint32_t* __restrict__ succ) {
    const uint64_t n2 = 2ull * n;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n2; v += (uint64_t)gridDim.x * blockDim.x) {
        const kq_entry e = ents[v >> 1];
        const uint32_t rc = (uint32_t)v & 1u;
        uint32_t base = 0, link = GFA_NONE;
        if (gfa_out_degree(e, rc, &base) == 1 && e.key != revcomp2(e.key, (int)k)) {
            uint32_t minus = 0;
            const uint64_t y = gfa_step(e.key, rc, base, k, &minus);
            const uint32_t r = y != e.key && y != revcomp2(y, (int)k) ? gfa_rank(keys, n, y) : GFA_NONE;
            if (r != GFA_NONE) {
                const kq_entry f = ents[r];
                uint32_t back = 0, back_minus = 0;
                // flip(w) = (y, !minus) has one out-edge, and it leads to flip(v) = (x, !rc)
                if (gfa_out_degree(f, minus ^ 1u, &back) == 1 && gfa_step(y, minus ^ 1u, back, k, &back_minus) == e.key && back_minus == (rc ^ 1u))
                    link = 2u * r + minus;
            }
        }
        succ[v] = link;
    }
}

__global__ __launch_bounds__(256) void k_gfa_rank_init(const uint32_t* __restrict__ succ, uint32_t n, GfaNode* __restrict__ node, GfaState* __restrict__ st) {
    const uint64_t n2 = 2ull * n;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n2; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t s = succ[v ^ 1];
        uint32_t pred = GFA_NONE;
        if (s != GFA_NONE) { if (s < n2) pred = s ^ 1u; else atomicOr(&st->err, (unsigned int)GFA_ERR_INDEX); }
        node[v] = GfaNode{pred, (uint32_t)v, pred != GFA_NONE ? 1u : 0u, (uint32_t)v};
    }
}
// one round: every live pointer jumps over its target.  (On a cycle dist wraps; a cycle is ranked again after its cut.)
__global__ __launch_bounds__(256) void k_gfa_rank_round(const GfaNode* __restrict__ in, GfaNode* __restrict__ out, uint32_t n, GfaState* __restrict__ st) {
    const uint64_t n2 = 2ull * n;
    bool changed = false;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n2; v += (uint64_t)gridDim.x * blockDim.x) {
        GfaNode a = in[v];
        if (a.ptr != GFA_NONE) {
            if (a.ptr < n2) {
                const GfaNode b = in[a.ptr];
                a.dist += b.dist;
                a.mn = a.mn < b.mn ? a.mn : b.mn;
                a.head = b.head;
                a.ptr = b.ptr;
                changed = true;
            } else { atomicOr(&st->err, (unsigned int)GFA_ERR_INDEX); a.ptr = GFA_NONE; }
        }
        out[v] = a;
    }
    if (changed) st->changed = 1u;                      // (every writer stores the same value)
}
// after the round limit: a live pointer = on a cycle, mn = the cycle's smallest id.  The smaller of a cycle pair's two minima
// opens both cycles: the link into it, and the mirror of that link.
__global__ __launch_bounds__(256) void k_gfa_cut(const GfaNode* __restrict__ node, uint32_t n, uint32_t* __restrict__ succ, GfaState* __restrict__ st) {
    const uint64_t n2 = 2ull * n, stride = (uint64_t)gridDim.x * blockDim.x, n_iter = (n2 + stride - 1) / stride;      // whole waves stay in the loop
    uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t it = 0; it < n_iter; ++it, v += stride) {
        bool cut = false;
        if (v < n2) {
            const GfaNode a = node[v];
            if (a.ptr != GFA_NONE && a.mn == (uint32_t)v) {
                const GfaNode m = node[v ^ 1];
                const uint32_t s = succ[v ^ 1];                          // flip(v) -> flip(pred(v))
                if (m.ptr == GFA_NONE || s == GFA_NONE || s >= n2) atomicOr(&st->err, (unsigned int)GFA_ERR_MIRROR);
                else if ((uint32_t)v < m.mn) { succ[s ^ 1u] = GFA_NONE; succ[v ^ 1] = GFA_NONE; cut = true; }
            }
        }
        const uint64_t mask = __ballot(cut);
        if (mask && __lane_id() == (uint32_t)__ffsll((unsigned long long)mask) - 1u) atomicAdd(&st->n_cycles, (unsigned long long)__popcll(mask));
    }
}

// flag[v] = 1 and len[v] = bases of the segment where v is the head of a kept chain (room for 2n + 1 each: the scans' totals)
__global__ __launch_bounds__(256) void k_gfa_heads(const GfaNode* __restrict__ node, uint32_t n, uint32_t k, unsigned long long* __restrict__ flag,
                                                    unsigned long long* __restrict__ len, GfaState* __restrict__ st) {
    const uint64_t n2 = 2ull * n;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= n2; v += (uint64_t)gridDim.x * blockDim.x) {
        unsigned long long f = 0, l = 0;
        if (v < n2) {
            const GfaNode a = node[v];
            if (a.ptr != GFA_NONE) atomicOr(&st->err, (unsigned int)GFA_ERR_INDEX);      // not ranked
            else if (a.head == (uint32_t)v) {
                const uint32_t mirror_head = node[v ^ 1].head;           // flip(tail of this chain)
                if (mirror_head >= n2 || mirror_head == (uint32_t)v) atomicOr(&st->err, (unsigned int)GFA_ERR_MIRROR);
                else if ((uint32_t)v < mirror_head) { f = 1; l = (unsigned long long)node[mirror_head ^ 1u].dist + k; }
            }
        }
        flag[v] = f; len[v] = l;
    }
}

__device__ __forceinline__ char gfa_base(uint64_t code) { return "ACGT"[code & 3]; }

__global__ __launch_bounds__(256) void k_gfa_segments(const kq_entry* __restrict__ ents, const GfaNode* __restrict__ node, uint32_t n, uint32_t k,
                                                       const unsigned long long* __restrict__ seg_id, const unsigned long long* __restrict__ seq_off,
                                                       kq_gfa_segment* __restrict__ segs, uint64_t n_segs, char* __restrict__ seq, uint64_t n_seq,
                                                       GfaState* __restrict__ st) {
    const uint64_t n2 = 2ull * n;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n2; v += (uint64_t)gridDim.x * blockDim.x) {
        const GfaNode a = node[v];
        const uint32_t mirror_head = node[v ^ 1].head;
        if (a.head >= n2 || mirror_head >= n2) { atomicOr(&st->err, (unsigned int)GFA_ERR_INDEX); continue; }
        if (!(a.head < mirror_head)) continue;                           // the mirror chain is the kept one
        const kq_entry e = ents[v >> 1];
        const uint64_t s = gfa_oriented(e.key, (uint32_t)v & 1u, k);
        const uint64_t off = seq_off[a.head];
        if (a.head == (uint32_t)v) {
            const uint64_t id = seg_id[v];
            const uint32_t n_kmers = node[mirror_head ^ 1u].dist + 1u;
            if (id >= n_segs || off + k > n_seq) { atomicOr(&st->err, (unsigned int)GFA_ERR_OUTPUT); continue; }
            kq_gfa_segment r{};
            r.seq_off = off; r.head_key = e.key; r.n_kmers = n_kmers; r.cov = e.cov; r.head_rc = (uint8_t)(v & 1u);
            segs[id] = r;
            for (uint32_t c = 0; c < k; ++c) seq[off + c] = gfa_base(s >> (2 * c));
        } else {
            const uint64_t at = off + (k - 1) + a.dist;
            if (at >= n_seq) { atomicOr(&st->err, (unsigned int)GFA_ERR_OUTPUT); continue; }
            seq[at] = gfa_base(s >> (2 * (k - 1)));
        }
    }
}

// (segment, rc) of an oriented k-mer at the end of a chain: '+' when it lies on the kept chain
__device__ __forceinline__ bool gfa_end(const GfaNode* __restrict__ node, const unsigned long long* __restrict__ seg_id, uint64_t n2, uint32_t u, uint32_t* seg, uint8_t* rc) {
    const uint32_t h = node[u].head, mh = node[u ^ 1u].head;
    if (h >= n2 || mh >= n2) return false;
    *rc = (uint8_t)!(h < mh);
    const uint64_t id = seg_id[h < mh ? h : mh];
    *seg = (uint32_t)id;
    return id < n2;
}
// One work item per (oriented k-mer v, base i), item = 4 v + i: the record order.
//   collapsed    a non-zero counter that is no link and whose target w is present: emitted when w is the first k-mer of its chain,
//                dropped otherwise; when the mirror flip(w) -> flip(v) has a counter too, the smaller (source, target) is the one
//   no-collapse  src/kreeq.cpp:549-593: fw line this + -> next, bw line prev -> this +; nothing deduplicated
// WRITE = false: flag[item] (room for 8n + 1), n_dropped.  WRITE = true: the records at pos[item].
template <bool WRITE>
__global__ __launch_bounds__(256) void k_gfa_edges(const kq_entry* __restrict__ ents, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ succ,
                                                    const GfaNode* __restrict__ node, const unsigned long long* __restrict__ seg_id, uint32_t n, uint32_t k,
                                                    uint32_t collapse, unsigned long long* __restrict__ flag, const unsigned long long* __restrict__ pos,
                                                    kq_gfa_edge* __restrict__ edges, uint64_t n_edges, GfaState* __restrict__ st) {
    const uint64_t n2 = 2ull * n, n_items = 4 * n2;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n_iter = (n_items + 1 + stride - 1) / stride;      // whole waves stay in the loop
    uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t it = 0; it < n_iter; ++it, item += stride) {
        bool emit = false, dropped = false;
        kq_gfa_edge r{};
        if (item < n_items) {
            const uint32_t v = (uint32_t)(item >> 2), base = (uint32_t)item & 3u, rc = v & 1u;
            const kq_entry* e = ents + (v >> 1);                          // (read in place: a copy indexed by `base` would live in scratch)
            const uint32_t cnt = rc ? e->bw[base] : e->fw[base];
            const uint64_t key = keys[v >> 1];
            uint32_t minus = 0, rank = GFA_NONE;
            if (cnt != 0) rank = gfa_rank(keys, n, gfa_step(key, rc, base, k, &minus));
            if (rank != GFA_NONE) {
                const uint32_t w = 2u * rank + minus;
                r.count = cnt;
                if (!collapse) {
                    emit = true;
                    if (!rc) { r.from = v >> 1; r.to = rank; r.to_rc = (uint8_t)minus; }
                    else { r.from = rank; r.from_rc = (uint8_t)(minus ^ 1u); r.to = v >> 1; }
                } else if (succ[v] != w) {
                    if (node[w].head != w) dropped = true;
                    else {
                        // the mirror's counter: flip(w) appends the last base of flip(v) = the complement of v's first base
                        const uint64_t sv = gfa_oriented(key, rc, k);
                        const uint32_t b = 3u - (uint32_t)(sv & 3u);
                        const kq_entry* f = ents + rank;
                        const uint32_t j = minus ? b : 3u - b;                     // flip(w) is (y,+) when w is (y,-): fw[b]; else bw[3 - b]
                        uint32_t mirror = minus ? f->fw[j] : f->bw[j], back_minus = 0;
                        // where a key is its own reverse complement both orientations are one string and the step decides which id it is
                        if (mirror != 0 && !(gfa_step(keys[rank], minus ^ 1u, j, k, &back_minus) == key && back_minus == (rc ^ 1u))) mirror = 0;
                        const bool mirror_first = (w ^ 1u) < v || ((w ^ 1u) == v && (v ^ 1u) < w);
                        if (!(mirror != 0 && mirror_first)) {
                            emit = gfa_end(node, seg_id, n2, v, &r.from, &r.from_rc) && gfa_end(node, seg_id, n2, w, &r.to, &r.to_rc);
                            if (!emit) atomicOr(&st->err, (unsigned int)GFA_ERR_INDEX);
                        }
                    }
                }
            }
        }
        if (!WRITE) {
            if (item <= n_items) flag[item] = emit;
            const uint64_t mask = __ballot(dropped);
            if (mask && __lane_id() == (uint32_t)__ffsll((unsigned long long)mask) - 1u) atomicAdd(&st->n_dropped, (unsigned long long)__popcll(mask));
        } else if (emit) {
            const uint64_t o = pos[item];
            if (o < n_edges) edges[o] = r; else atomicOr(&st->err, (unsigned int)GFA_ERR_OUTPUT);
        }
    }
}

}  // namespace kq
