// kq_variants.h -- the candidate-error searches of `kreeq validate -o vcf` on the device (kq_search_variants; reference
// DBG::DBGtoVariants / searchVariants, src/variants.cpp:53-310).  Included by kreeq_amd.hip after kq_subgraph.h.
//
// One search per flagged position and per LANE, for the reasons of the best-first kernels (kq_subgraph.h): a search is serial
// within one source and independent between sources (read-only table, read-only text), and its state is bounded
// (kq_variant_core.h), so each lane runs the whole search -- at most depth + 1 pops -- on a state block of its own in a global
// arena, with no host round trip.  Every heap step is a dependent access to that block; occupancy is what hides it.
//
//  1. k_branch_scan (kq_kernels.h) flags the positions; k_var_flag turns "(flag & 3) == 3" into 0 / 1 words, whose exclusive
//     prefix sum places them: k_var_scatter writes the ascending position list.  The same two steps over k_sg_invalid's
//     "not a base" words give the ascending list of BREAKS; a search finds its segment's bounds by bisection in it, so no
//     lane walks the text backwards.
//  2. k_var_search: the searches of one batch; a lane leaves its paths and sequence bytes in its block's head and in two
//     count arrays.  The batch totals and the OR of the error codes are wave-reduced into one VarState.
//  3. Exclusive prefix sums of the counts, then k_var_emit: a lane walks its block's prev chains once more and writes its
//     records and bases at their final places.
#pragma once
#include "kq_variant_core.h"

namespace kq {

// the two questions of the search core: edges by table probe with the LOGICAL counters (the high-copy tier's for a high-copy
// k-mer), bases from the text of the segment
struct VarGraph {
    const TableView& t;
    const uint8_t* seg;
    uint32_t cov_cutoff;
    __device__ uint32_t edge_mask(uint64_t key) const {
        const uint64_t h = table_hash(key, t.k);
        const Slot* s = table_find(t, h);
        if (!s) return 0;                                                // an absent neighbour: a node without edges
        const Logical L = logical_of(t, h, s->w0, s->e8);
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) m |= (uint32_t)(L.e[i] != 0) << i | (uint32_t)(L.e[4 + i] > cov_cutoff) << (4 + i);      // src/variants.cpp:237
        return m;
    }
    __device__ uint32_t base(uint64_t p) const {                         // ACGTacgt -> 0..3
        const uint32_t u = seg[p];
        return ((u >> 1) & 3u) ^ ((u >> 2) & 1u);
    }
};
struct VarState { unsigned long long n_paths, n_seq; unsigned int err, pad; };      // of one batch: paths, sequence bytes, OR of the error codes

__global__ __launch_bounds__(256) void k_var_flag(const uint8_t* __restrict__ flags, uint64_t len, uint32_t* __restrict__ word) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (uint64_t)gridDim.x * blockDim.x) word[i] = (flags[i] & 3u) == 3u;
}
// out[rank[i]] = i for every i with word[i] != 0 (rank: the exclusive prefix sum of word): the ascending list; out has cap entries
__global__ __launch_bounds__(256) void k_var_scatter(const uint32_t* __restrict__ word, const uint32_t* __restrict__ rank, uint64_t len, uint32_t* __restrict__ out,
                                                      uint64_t cap) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (uint64_t)gridDim.x * blockDim.x)
        if (word[i] && rank[i] < cap) out[rank[i]] = (uint32_t)i;
}

// the segment (run of bases) around text position p: [*start, *end), from the ascending breaks
__device__ __forceinline__ void var_segment(const uint32_t* __restrict__ breaks, uint32_t n_breaks, uint64_t len, uint32_t p, uint64_t* start, uint64_t* end) {
    uint32_t lo = 0, hi = n_breaks;                                      // -> the number of breaks below p
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (breaks[mid] < p) lo = mid + 1; else hi = mid; }
    *start = lo ? (uint64_t)breaks[lo - 1] + 1 : 0;
    *end = lo < n_breaks ? breaks[lo] : len;
}

// pos[i] (i < n): the text position of the source k-mer of search i; arena + i * block_bytes: its state block, whose index the
// host has filled with 0xFF.  The state stays in the block for k_var_emit.
__global__ __launch_bounds__(256) void k_var_search(TableView t, const uint8_t* __restrict__ text, uint64_t len, const uint32_t* __restrict__ pos, uint64_t n,
                                                     const uint32_t* __restrict__ breaks, uint32_t n_breaks, int depth, int span, uint32_t cov_cutoff,
                                                     uint8_t* __restrict__ arena, uint64_t block_bytes, unsigned long long* __restrict__ cnt_paths,
                                                     unsigned long long* __restrict__ cnt_seq, VarState* __restrict__ st) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n_iter = (n + stride - 1) / stride;      // whole waves stay in the loop
    const int k = (int)t.k;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t it = 0; it < n_iter; ++it, i += stride) {
        uint32_t paths = 0, seq = 0, err = 0;
        if (i < n) {
            const uint32_t p = pos[i];
            uint64_t s0, s1;
            var_segment(breaks, n_breaks, len, p, &s0, &s1);
            void* block = arena + i * block_bytes;
            if (p < s0 || p >= s1 || s1 > len || s1 - s0 < (uint64_t)k) err = kqvar::ERR_TEXT;      // cannot happen: a flagged position starts a k-mer
            else {
                const VarGraph g{t, text + s0, cov_cutoff};
                paths = kqvar::search(block, depth, span, k, (uint64_t)p - s0, s1 - s0 - (uint64_t)k + 1, g);
                const kqbf::Head* hd = kqvar::head_of(block);
                err = hd->err;
                seq = kqvar::seq_bytes_of(hd);
            }
            if (err) { paths = 0; seq = 0; }
            cnt_paths[i] = paths; cnt_seq[i] = seq;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { paths += __shfl_xor(paths, o, 64); seq += __shfl_xor(seq, o, 64); err |= __shfl_xor(err, o, 64); }      // <= 64 * 1016 * 255: 32 bits
        if (__lane_id() == 0) {
            if (paths) atomicAdd(&st->n_paths, (unsigned long long)paths);
            if (seq) atomicAdd(&st->n_seq, (unsigned long long)seq);
            if (err) atomicOr(&st->err, err);
        }
    }
}
// off_paths / off_seq: the exclusive prefix sums of the batch's counts; base_*: what the batches before wrote.  Search i writes
// its records at paths[base_paths + off_paths[i] ..] in destination order and their bases behind one another from
// seq[base_seq + off_seq[i]].  Nothing is written at or beyond path_cap / seq_cap (the host launches this only when the
// totals fit; a violation is reported, not written).
__global__ __launch_bounds__(256) void k_var_emit(TableView t, const uint8_t* __restrict__ text, uint64_t len, const uint32_t* __restrict__ pos, uint64_t n,
                                                   const uint32_t* __restrict__ breaks, uint32_t n_breaks, int depth, int span, uint8_t* __restrict__ arena,
                                                   uint64_t block_bytes, const unsigned long long* __restrict__ off_paths, const unsigned long long* __restrict__ off_seq,
                                                   uint64_t base_paths, uint64_t base_seq, kq_variant_path* __restrict__ paths, uint64_t path_cap, char* __restrict__ seq,
                                                   uint64_t seq_cap, VarState* __restrict__ st) {
    const int k = (int)t.k;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        void* block = arena + i * block_bytes;
        if (kqvar::head_of(block)->n_found == 0) continue;
        const uint32_t p = pos[i];
        uint64_t s0, s1;
        var_segment(breaks, n_breaks, len, p, &s0, &s1);
        const VarGraph g{t, text + s0, 0};
        kqvar::Search<VarGraph> s(block, depth, span, k, g);
        s.reopen();
        uint64_t at_path = base_paths + off_paths[i], at_seq = base_seq + off_seq[i];
        const uint32_t n_paths = s.n_dest;
        for (uint32_t d = 0; d < n_paths; ++d) {                         // <= 4 (depth + 1)
            kqvar::Path q;
            if (!s.path(d, &q, nullptr) || at_path >= path_cap || at_seq + q.seq_len > seq_cap) { atomicOr(&st->err, s.err ? s.err : (unsigned)kqvar::ERR_DEST); break; }
            s.path(d, &q, seq + at_seq);
            kq_variant_path r;
            r.pos = (uint64_t)p + (uint64_t)k; r.seg_start = s0; r.seq_off = at_seq; r.seq_len = q.seq_len; r.ref_len = q.ref_len; r.type = q.type;
            r.pad[0] = r.pad[1] = r.pad[2] = 0;
            paths[at_path] = r;
            ++at_path; at_seq += q.seq_len;
        }
    }
}

}  // namespace kq
