// kq_subgraph.h -- kernels of the subgraph mode (reference src/subgraph.cpp): seed a second table from the k-mers of a set
// of sequences, expand it level by level along the edge counters of the database or by one best-first search per seed, clear
// the edges that lead outside it.
// gfx950 only.  Host side: kq_subgraph_seed(_dev) / kq_subgraph_expand / kq_subgraph_best_first / kq_subgraph_trim in kreeq_amd.hip.
//
// Every probe here is one random 64-byte sector read of a table region (table_find), as in k_lookup; nothing in this
// file is bound by anything else, so the kernels keep the one-item-per-thread form at full occupancy.
#pragma once
#include "kq_bestfirst_core.h"

namespace kq {

constexpr uint32_t SG_NONE = 0xFFFFFFFFu;          // free slot of the seed's (segment, key) set

// the k-mer one step along edge e (0..3 = fw[A,C,G,T]: append the base, 4..7 = bw: prepend it) of the canonical string
// of `key` (DBG::buildNextKmer + hash, src/subgraph.cpp:581-597); keys hold the first base in the low bits
__device__ __forceinline__ uint64_t sg_neighbour(uint64_t key, uint32_t e, uint32_t k) {
    const uint64_t kmask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1;
    const uint64_t base = e & 3u;
    const uint64_t nxt = e < 4 ? (key >> 2) | (base << (2 * k - 2)) : ((key << 2) | base) & kmask;
    const uint64_t rv = revcomp2(nxt, (int)k);
    return nxt < rv ? nxt : rv;
}

// ---- seed ------------------------------------------------------------------------------------------------------------
// 1. k_sg_invalid: one flag per byte (not ACGTacgt); its exclusive prefix sum numbers the segments (the ACGT runs).
// 2. k_sg_keys: canonical key and neighbour codes of every k-mer start (EMPTY_KEY where none starts).
// 3. k_sg_first: an open-addressing set of (segment, key) whose slots hold a POSITION of that pair; atomicMin leaves the
//    first one (DBGsubgraphFromSegment inserts into a per-segment map, which keeps the first: :242, :276).  The pair a
//    slot stands for is read back through the position, so a slot is one 32-bit word and the claim one CAS.
// 4. k_sg_seed_add: one thread per slot of the set; the winning position contributes the database entry (:238-249) or a
//    constructed k-mer (:250-277) to the subgraph table.  Sums over segments are add_logical's (:58-85; the table keeps
//    64-bit sums and clamps at LARGEST on read).
__global__ __launch_bounds__(256) void k_sg_invalid(const uint8_t* __restrict__ bases, uint64_t len, uint32_t* __restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t u = bases[i] & 0xDFu;
        flag[i] = !(u == 'A' || u == 'C' || u == 'G' || u == 'T');
    }
}
__global__ __launch_bounds__(TILE_THREADS) void k_sg_keys(const uint8_t* __restrict__ ab, uint64_t lead, uint64_t len, int k,
                                                           uint64_t* __restrict__ key_at, uint8_t* __restrict__ info_at) {
    scan_tiles(ab, lead, len, k, [&](uint64_t pos, uint64_t fw, uint64_t rv, uint32_t prev, uint32_t next) {
        const bool is_fw = fw < rv;
        key_at[pos] = is_fw ? fw : rv;
        info_at[pos] = (uint8_t)(prev | (next << 3) | ((uint32_t)is_fw << 6));
    });
}
__device__ __forceinline__ uint64_t sg_pair_hash(uint64_t key, uint32_t seg) { return mix64(key ^ mix64((uint64_t)seg + 0x9E3779B97F4A7C15ull)); }
__global__ __launch_bounds__(256) void k_sg_first(const uint64_t* __restrict__ key_at, const uint32_t* __restrict__ seg_at, uint64_t n_pos,
                                                   uint32_t* __restrict__ set, uint64_t set_mask, unsigned int* __restrict__ err) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pos; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = key_at[p];
        if (key == EMPTY_KEY) continue;
        const uint32_t seg = seg_at[p];
        uint64_t i = sg_pair_hash(key, seg) & set_mask;
        bool done = false;
        for (uint64_t probe = 0; probe <= set_mask && !done; ++probe, i = (i + 1) & set_mask) {
            uint32_t cur = __hip_atomic_load(&set[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == SG_NONE) {
                cur = atomicCAS(&set[i], SG_NONE, (uint32_t)p);
                if (cur == SG_NONE) { done = true; break; }
            }
            // whatever position the slot holds now or later, it is one of this slot's pair
            if (key_at[cur] == key && seg_at[cur] == seg) { atomicMin(&set[i], (uint32_t)p); done = true; }
        }
        if (!done) atomicOr(err, 1u);
    }
}
struct SgSeedOut { unsigned long long n_kmers, n_instances; };
template <bool ADD>
__global__ __launch_bounds__(256) void k_sg_seed_add(TableView db, TableView sub, const uint32_t* __restrict__ set, uint64_t set_size,
                                                      const uint64_t* __restrict__ key_at, const uint8_t* __restrict__ info_at,
                                                      uint32_t no_reference, SgSeedOut* __restrict__ out) {
    uint32_t n_new = 0;
    uint64_t n_cov = 0, n_kmers = 0, n_inst = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < set_size; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t p = set[i];
        if (p == SG_NONE) continue;
        const uint64_t h = table_hash(key_at[p], db.k);
        const Slot* s = table_find(db, h);
        uint32_t e[8], cov;
        if (s) {
            const Logical L = logical_of(db, h, s->w0, s->e8);
#pragma unroll
            for (int w = 0; w < 8; ++w) e[w] = L.e[w];
            cov = L.cov;
        } else {
            if (no_reference) continue;
            const uint32_t info = info_at[p];
            const uint64_t pack = edge_pack((info >> 6) & 1u, info & 7u, (info >> 3) & 7u);
#pragma unroll
            for (int w = 0; w < 8; ++w) e[w] = (uint32_t)(pack >> (8 * w)) & 0xFFu;
            cov = 1;
        }
        ++n_kmers; n_inst += cov;
        if (ADD) add_logical(sub, h, e, cov, n_new, n_cov);
    }
    if (ADD) {
        const uint64_t a = block_sum(n_new), b = block_sum(n_cov);
        if (threadIdx.x == 0) {
            if (a) atomicAdd(&sub.st->slots_used, (unsigned long long)a);
            if (b) atomicAdd(&sub.st->kmers_added, (unsigned long long)b);
        }
    } else {
        const uint64_t a = block_sum(n_kmers), b = block_sum(n_inst);
        if (threadIdx.x == 0) {
            if (a) atomicAdd(&out->n_kmers, (unsigned long long)a);
            if (b) atomicAdd(&out->n_instances, (unsigned long long)b);
        }
    }
}

// ---- expand (DBG::traversal, src/subgraph.cpp:301-415) ------------------------------------------------------------------
// ents[0, n_seed) = the seed k-mers with their subgraph entries, ents[n_seed, ...) = what the rounds found, in the order
// found; the frontier of a round is the slice the round before appended.  One work item per (frontier k-mer, edge):
// a counter != 0 (no cutoff here, :331 / :372) gives the neighbour key; it is a candidate when it is no seed (probe of
// `sub`, which holds the seeds and nothing else until the last round is over: :344), is in the database, and has not
// been found before (claim in `visited`, an open-addressing key set: the reference finds a k-mer again in later rounds,
// the union over the rounds is the same).  The winners of a wave reserve their output range with one atomic.
struct SgExpandState { unsigned long long n_ents, n_instances; unsigned int err, pad; };
// claims `key` in the visited set (open addressing, EMPTY_KEY = free): true for the one work item that found it first
__device__ __forceinline__ bool sg_claim(uint64_t* __restrict__ visited, uint64_t visited_mask, uint64_t key, SgExpandState* __restrict__ st) {
    uint64_t j = mix64(key ^ 0x9E3779B97F4A7C15ull) & visited_mask;
    for (uint64_t probe = 0; probe <= visited_mask; ++probe, j = (j + 1) & visited_mask) {
        uint64_t cur = ld_relaxed(&visited[j]);
        if (cur == EMPTY_KEY) {
            cur = atomicCAS((unsigned long long*)&visited[j], (unsigned long long)EMPTY_KEY, (unsigned long long)key);
            if (cur == EMPTY_KEY) return true;
        }
        if (cur == key) return false;
    }
    atomicOr(&st->err, 1u);
    return false;
}
// the logical entry of the database slot `s` of `key` (hash h), as kq_export writes it
__device__ __forceinline__ kq_entry sg_entry_of(const TableView& db, uint64_t key, uint64_t h, const Slot* s) {
    const Logical L = logical_of(db, h, s->w0, s->e8);
    kq_entry e;
    e.key = key;
#pragma unroll
    for (int w = 0; w < 4; ++w) { e.fw[w] = L.e[w]; e.bw[w] = L.e[4 + w]; }
    e.cov = L.cov;
    e.hc = L.cov > LOW_TIER_MAX;
    return e;
}
// appends the entries of the winners of a wave to the found list: one atomic per wave reserves their range.  Every lane of
// the wave calls this.
__device__ __forceinline__ void sg_append(bool win, const kq_entry& found, kq_entry* ents, uint64_t ents_cap, SgExpandState* __restrict__ st) {
    const uint64_t mask = __ballot(win);
    if (!mask) return;
    const uint32_t lane = __lane_id();
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)mask) - 1u;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(&st->n_ents, (unsigned long long)__popcll(mask));
    base = __shfl(base, (int)leader, 64);
    if (win) {
        const uint64_t o = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (o < ents_cap) ents[o] = found; else atomicOr(&st->err, 2u);
    }
}
__global__ __launch_bounds__(256) void k_sg_expand(TableView db, TableView sub, kq_entry* ents, uint64_t f_lo, uint64_t f_hi,
                                                    uint64_t ents_cap, uint64_t* __restrict__ visited, uint64_t visited_mask,
                                                    SgExpandState* __restrict__ st) {
    const uint64_t n_items = (f_hi - f_lo) * 8;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n_iter = (n_items + stride - 1) / stride;      // whole waves stay in the loop
    uint64_t n_inst = 0;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t it = 0; it < n_iter; ++it, i += stride) {
        bool win = false;
        kq_entry found;
        if (i < n_items) {
            const kq_entry* src = ents + f_lo + (i >> 3);
            const uint32_t e = (uint32_t)i & 7u;
            const uint32_t cnt = e < 4 ? src->fw[e] : src->bw[e - 4];
            if (cnt != 0) {
                const uint64_t key = sg_neighbour(src->key, e, db.k);
                const uint64_t h = table_hash(key, db.k);
                if (!table_find(sub, h)) {
                    const Slot* s = table_find(db, h);
                    if (s) {
                        win = sg_claim(visited, visited_mask, key, st);
                        if (win) { found = sg_entry_of(db, key, h, s); n_inst += found.cov; }
                    }
                }
            }
        }
        sg_append(win, found, ents, ents_cap, st);
    }
    const uint64_t a = block_sum(n_inst);
    if (threadIdx.x == 0 && a) atomicAdd(&st->n_instances, (unsigned long long)a);
}
// the visited set after it was enlarged: the keys found so far
__global__ __launch_bounds__(256) void k_sg_visited_fill(const kq_entry* __restrict__ ents, uint64_t lo, uint64_t hi, uint64_t* __restrict__ visited,
                                                          uint64_t visited_mask, SgExpandState* __restrict__ st) {
    for (uint64_t i = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = ents[i].key;
        uint64_t j = mix64(key ^ 0x9E3779B97F4A7C15ull) & visited_mask;
        bool placed = false;
        for (uint64_t probe = 0; probe <= visited_mask && !placed; ++probe, j = (j + 1) & visited_mask)
            placed = atomicCAS((unsigned long long*)&visited[j], (unsigned long long)EMPTY_KEY, (unsigned long long)key) == EMPTY_KEY;
        if (!placed) atomicOr(&st->err, 1u);
    }
}

// ---- best-first (DBG::bestFirst / dijkstra, src/subgraph.cpp:417-579) ----------------------------------------------------
// One search per seed k-mer and per LANE: the search is serial within one source and independent between sources (read-only
// database, read-only seed set), and its state is bounded (kq_bestfirst_core.h), so each lane runs the whole search -- at
// most depth + 1 pops -- on a state block of its own in a global arena, with no host round trip.  Every heap step is a
// dependent access to that block; occupancy is what hides it.
//
// the two questions of the search core, answered by table probes; counters are the LOGICAL ones (the high-copy tier's for a
// high-copy k-mer), membership is against `sub`, which holds the seeds and nothing else until the last batch is over (:453)
struct SgBfGraph {
    const TableView& db;
    const TableView& sub;
    uint32_t cov_cutoff;
    __device__ bool is_seed(uint64_t key) const { return table_find(sub, table_hash(key, sub.k)) != nullptr; }
    __device__ int db_mask(uint64_t key) const {
        const uint64_t h = table_hash(key, db.k);
        const Slot* s = table_find(db, h);
        if (!s) return -1;
        const Logical L = logical_of(db, h, s->w0, s->e8);
        int m = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) m |= (int)(L.e[e] > cov_cutoff) << e;
        return m;
    }
};
struct SgBfState { unsigned long long n_found; unsigned int err, pad; };      // of one batch: discovered nodes (with repeats), OR of the error codes
// seeds[i] (i < n): the source of search i with its merged subgraph entry (:470), as k_export lists it; arena + i * block_bytes:
// its state block, whose index the host has filled with 0xFF.  The flagged nodes stay in the block for k_sg_bf_collect.
__global__ __launch_bounds__(256) void k_sg_bf_search(TableView db, TableView sub, const kq_entry* __restrict__ seeds, uint64_t n, int depth,
                                                       uint32_t cov_cutoff, uint8_t* __restrict__ arena, uint64_t block_bytes, SgBfState* __restrict__ st) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n_iter = (n + stride - 1) / stride;      // whole waves stay in the loop
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t it = 0; it < n_iter; ++it, i += stride) {
        uint32_t found = 0, err = 0;
        if (i < n) {
            const kq_entry src = seeds[i];
            uint32_t mask = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) mask |= (uint32_t)(src.fw[e] > cov_cutoff) << e | (uint32_t)(src.bw[e] > cov_cutoff) << (4 + e);
            void* block = arena + i * block_bytes;
            const SgBfGraph g{db, sub, cov_cutoff};
            found = kqbf::search(block, depth, (int)db.k, src.key, mask, g);
            err = kqbf::head_of(block)->err;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { found += __shfl_xor(found, o, 64); err |= __shfl_xor(err, o, 64); }
        if (__lane_id() == 0) {
            if (found) atomicAdd(&st->n_found, (unsigned long long)found);
            if (err) atomicOr(&st->err, err);
        }
    }
}
// One work item per (search, node slot) of the batch: a flagged node claims its key in the visited set, so that a k-mer that
// many searches discovered is listed once, and the winner appends the k-mer's database entry to the found list.
__global__ __launch_bounds__(256) void k_sg_bf_collect(TableView db, const uint8_t* __restrict__ arena, uint64_t block_bytes, uint64_t n, uint32_t n_slots,
                                                        kq_entry* ents, uint64_t ents_cap, uint64_t* __restrict__ visited, uint64_t visited_mask,
                                                        SgExpandState* __restrict__ st) {
    const uint64_t n_items = n * n_slots;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n_iter = (n_items + stride - 1) / stride;
    uint64_t n_inst = 0;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t it = 0; it < n_iter; ++it, i += stride) {
        bool win = false;
        kq_entry found;
        if (i < n_items) {
            const uint64_t search = i / n_slots;
            const uint32_t slot = (uint32_t)(i - search * n_slots);
            const uint8_t* block = arena + search * block_bytes;
            const kqbf::Head* hd = (const kqbf::Head*)block;
            if (slot < hd->n_nodes && hd->n_nodes <= n_slots) {
                const kqbf::Node* node = (const kqbf::Node*)(block + sizeof(kqbf::Head)) + slot;
                if (node->flags & kqbf::F_FOUND) {
                    const uint64_t key = node->key;
                    const uint64_t h = table_hash(key, db.k);
                    const Slot* s = table_find(db, h);                   // present: the search met the key in the database
                    if (!s) atomicOr(&st->err, 4u);
                    else {
                        win = sg_claim(visited, visited_mask, key, st);
                        if (win) { found = sg_entry_of(db, key, h, s); n_inst += found.cov; }
                    }
                }
            }
        }
        sg_append(win, found, ents, ents_cap, st);
    }
    const uint64_t a = block_sum(n_inst);
    if (threadIdx.x == 0 && a) atomicAdd(&st->n_instances, (unsigned long long)a);
}

// ---- trim (DBG::removeMissingEdges, src/subgraph.cpp:599-625) -----------------------------------------------------------
// One thread per slot.  Tests read the key words (w0) of other slots, which nothing writes here; a thread clears
// counters of its own slot and of its own high-copy entry only.
__global__ __launch_bounds__(256) void k_sg_trim(TableView t, uint32_t cov_cutoff) {
    const uint64_t s0 = t.reg_lo << REGION_SHIFT, n = (t.reg_hi - t.reg_lo) << REGION_SHIFT;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        Slot* s = t.slots + s0 + i;
        const uint64_t w0 = s->w0;
        if (w0 == 0) continue;
        const uint64_t h = slot_hash_at(t, s, w0);
        const uint64_t key = key_of_hash(h, t.k);
        uint64_t e8 = s->e8;
        const Logical L = logical_of(t, h, w0, e8);
        uint32_t drop = 0;
#pragma unroll
        for (uint32_t e = 0; e < 8; ++e)
            if (L.e[e] > cov_cutoff && !table_find(t, table_hash(sg_neighbour(key, e, t.k), t.k))) drop |= 1u << e;
        if (!drop) continue;
        HcSlot* hs = (w0 >> COV_SHIFT) == COV8_TOMB ? const_cast<HcSlot*>(hc_find(t, key)) : nullptr;
#pragma unroll
        for (uint32_t e = 0; e < 8; ++e) {
            if (!((drop >> e) & 1u)) continue;
            e8 &= ~(0xFFull << (8 * e));
            if (hs) hs->cnt[e] = 0;
        }
        s->e8 = e8;
    }
}

}  // namespace kq
