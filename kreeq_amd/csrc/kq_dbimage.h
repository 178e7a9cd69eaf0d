// kq_dbimage.h -- <db>/.map.<m>.bin images built and parsed on the device (kq_export_map_images / kq_import_map_image).
//
// Writer: the image is what gfalibs' dumpMap writes after inserting the map's k-mers one by one in ascending key order
// (the host writer, kreeq_amd/host/kreeq_db.cpp, emulates exactly that).  Insertion order matters only inside a submap,
// and submaps are independent, so:
//   k_dbi_hist      table -> k-mers per (map, submap) and the high-copy count        (the size query stops here)
//   k_dbi_records   key-sorted entries -> u64 records (map, submap) << 32 | index; high-copy entries are collected
//   k_dbi_split_*   stable split of the records by one 8-bit digit of (map, submap): least significant digit first, so
//                   two passes (three beyond 256 maps) leave every submap's records contiguous and in key order.  A
//                   workgroup owns a contiguous chunk; within a wave the rank among equal digits is a ballot match, the
//                   waves of a round and the workgroups are ordered by count matrices: no atomic decides a position
//   k_dbi_build     one wave per submap inserts its entries in order: 16 lanes read a control group, a ballot finds the
//                   first empty byte, 24 lanes write the slot bytes, two lanes the H2 byte and its clone
// Reader: k_dbi_check validates every occupied slot of an image and counts, k_dbi_add adds them to the table.
#pragma once
#include "kq_dbimage_host.h"      // (included behind kq_kernels.h, whose device functions the kernels here use)

namespace kq {

__device__ __forceinline__ uint64_t dbi_mix(uint64_t a) {                  // phmap_mix<8>: high + low half of a * k
    constexpr uint64_t m = 0xde5fb9d2630458e9ull;
    return __umul64hi(a, m) + a * m;
}
__device__ __forceinline__ uint32_t dbi_submap(uint64_t h) { return (uint32_t)((h >> 8) ^ (h >> 16) ^ (h >> 24)) & (DBI_SUBMAPS - 1); }

// cnt[(m - lo) * 256 + submap] = k-mers of the table in that submap of map m, cnt[(hi - lo) * 256] = high-copy k-mers of the range
__global__ __launch_bounds__(256) void k_dbi_hist(TableView t, uint32_t map_count, uint32_t lo, uint32_t hi, unsigned long long* __restrict__ cnt) {
    const uint64_t s0 = t.reg_lo << REGION_SHIFT, n = (t.reg_hi - t.reg_lo) << REGION_SHIFT;     // the allocated slots
    uint32_t n_hc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const Slot* s = t.slots + s0 + i;
        const uint64_t w0 = s->w0;
        if (w0 == 0) continue;
        const uint64_t h = slot_hash_at(t, s, w0), key = key_of_hash(h, t.k);
        const uint32_t m = (uint32_t)(key % map_count);
        if (m < lo || m >= hi) continue;
        atomicAdd(&cnt[(uint64_t)(m - lo) * DBI_SUBMAPS + dbi_submap(dbi_mix(key))], 1ull);
        n_hc += logical_of(t, h, w0, s->e8).cov > LOW_TIER_MAX;
    }
    const uint64_t a = block_sum(n_hc);
    if (threadIdx.x == 0 && a) atomicAdd(&cnt[(uint64_t)(hi - lo) * DBI_SUBMAPS], (unsigned long long)a);
}

__global__ __launch_bounds__(256) void k_dbi_records(const kq_entry* __restrict__ e, uint64_t n, uint32_t map_count, uint32_t lo,
                                                      uint64_t* __restrict__ recs, kq_entry* __restrict__ hc_out, uint64_t hc_cap,
                                                      unsigned long long* __restrict__ hc_n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = e[i].key;
        const uint32_t b = ((uint32_t)(key % map_count) - lo) * DBI_SUBMAPS + dbi_submap(dbi_mix(key));
        recs[i] = ((uint64_t)b << 32) | i;
        if (e[i].hc) {
            const unsigned long long o = atomicAdd(hc_n, 1ull);       // few; the host puts them in key order
            if (o < hc_cap) hc_out[o] = e[i];
        }
    }
}

// Stable split of `n` records by digit = (rec >> shift) & 255 over G workgroups, workgroup g owning the records
// [g * chunk, (g + 1) * chunk).  mat[digit * G + g]: first the count (k_dbi_split_hist), then the output position of the
// first such record (k_dbi_split_scan: exclusive prefix in digit-major order).
__global__ __launch_bounds__(256) void k_dbi_split_hist(const uint64_t* __restrict__ recs, uint64_t n, uint64_t chunk, uint32_t shift,
                                                         unsigned long long* __restrict__ mat) {
    __shared__ uint32_t s_hist[256];
    const uint32_t tid = threadIdx.x;
    s_hist[tid] = 0;
    __syncthreads();
    const uint64_t a = (uint64_t)blockIdx.x * chunk, b = a + chunk < n ? a + chunk : n;
    for (uint64_t i = a + tid; i < b; i += 256) atomicAdd(&s_hist[(uint32_t)(recs[i] >> shift) & 255u], 1u);
    __syncthreads();
    mat[(uint64_t)tid * gridDim.x + blockIdx.x] = s_hist[tid];
}
__global__ __launch_bounds__(256) void k_dbi_split_scan(unsigned long long* __restrict__ mat, uint32_t G) {
    __shared__ unsigned long long s_tot[256];
    const uint32_t tid = threadIdx.x;
    unsigned long long tot = 0;
    for (uint32_t g = 0; g < G; ++g) tot += mat[(uint64_t)tid * G + g];
    s_tot[tid] = tot;
    __syncthreads();
    unsigned long long run = 0;
    for (uint32_t d = 0; d < tid; ++d) run += s_tot[d];
    for (uint32_t g = 0; g < G; ++g) { const unsigned long long v = mat[(uint64_t)tid * G + g]; mat[(uint64_t)tid * G + g] = run; run += v; }
}
__global__ __launch_bounds__(256) void k_dbi_split_scatter(const uint64_t* __restrict__ recs, uint64_t n, uint64_t chunk, uint32_t shift,
                                                            const unsigned long long* __restrict__ mat, uint64_t* __restrict__ out) {
    __shared__ unsigned long long s_cur[256];      // next output position of every digit
    __shared__ uint32_t s_wave[4][256];            // records of every digit in each wave of the current round
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_cur[tid] = mat[(uint64_t)tid * gridDim.x + blockIdx.x];
    for (int w = 0; w < 4; ++w) s_wave[w][tid] = 0;
    __syncthreads();
    const uint64_t a = (uint64_t)blockIdx.x * chunk, b = a + chunk < n ? a + chunk : n;
    for (uint64_t base = a; base < b; base += 256) {
        const uint64_t i = base + tid;
        const bool valid = i < b;
        const uint64_t rec = valid ? recs[i] : 0;
        const uint32_t d = (uint32_t)(rec >> shift) & 255u;
        uint64_t peers = __ballot(valid);          // lanes of this wave with the same digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const uint64_t m = __ballot(one);
            peers &= one ? m : ~m;
        }
        const uint32_t rank = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) s_wave[wave][d] = __popcll(peers);
        __syncthreads();
        if (valid) {
            unsigned long long o = s_cur[d] + rank;
            for (uint32_t w = 0; w < wave; ++w) o += s_wave[w][d];
            out[o] = rec;
        }
        __syncthreads();
        uint32_t sum = 0;
        for (int w = 0; w < 4; ++w) { sum += s_wave[w][tid]; s_wave[w][tid] = 0; }
        s_cur[tid] += sum;
        __syncthreads();
    }
}

// lanes first .. first + 7 write the little-endian bytes of v (the image has no alignment: a submap's size is odd or even)
__device__ __forceinline__ void dbi_put64(uint8_t* p, uint64_t v, uint32_t lane, uint32_t first) {
    if (lane - first < 8u) p[lane - first] = (uint8_t)(v >> (8 * (lane - first)));
}

// sub[s] = (byte offset of submap s's header in img, index of its first record); sub[n_sub].y = n.  img is zero-filled.
// The control bytes a wave probes were written by the same wave: a fence between an insertion's stores and the next
// one's loads makes them visible (the loads are ordinary ones and would hit stale lines of the vector cache otherwise).
__global__ __launch_bounds__(256) void k_dbi_build(const kq_entry* __restrict__ ents, const uint64_t* __restrict__ recs,
                                                    const ulonglong2* __restrict__ sub, uint32_t n_sub, uint8_t* img) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n_waves = gridDim.x * 4;
    for (uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6); s < n_sub; s += n_waves) {
        const uint64_t e0 = sub[s].y, size = sub[s + 1].y - e0, cap = dbi_capacity(size);
        uint8_t* p = img + sub[s].x;
        if ((s & (DBI_SUBMAPS - 1)) == 0) dbi_put64(p - 8, DBI_SUBMAPS, lane, 32);      // the file starts with its submap count
        dbi_put64(p, DBI_VERSION, lane, 0);
        dbi_put64(p + 8, size, lane, 8);
        dbi_put64(p + 16, cap, lane, 16);
        if (!size) continue;
        uint8_t* ctrl = p + 24;
        uint8_t* slots = ctrl + cap + DBI_GROUP + 1;
        for (uint64_t j = lane; j < cap + DBI_GROUP + 1; j += 64) ctrl[j] = j == cap ? 0xFF : 0x80;     // empty, sentinel, (empty) clones
        dbi_put64(slots + cap * DBI_SLOT, dbi_growth(cap) - size, lane, 0);
        __threadfence();
        for (uint64_t j = 0; j < size; ++j) {
            const kq_entry* e = ents + (uint32_t)recs[e0 + j];
            const uint64_t key = e->key, h = dbi_mix(key);
            uint64_t offset = (h >> 7) & cap, index = 0, pos = ~0ull;
            for (uint64_t probe = 0; probe <= cap; ++probe) {                // find_first_non_full: a table below its growth limit has an empty byte
                const uint8_t c = lane < DBI_GROUP ? ctrl[offset + lane] : 0;   // the group load may run into the cloned bytes
                const uint64_t hit = __ballot(lane < DBI_GROUP && c == 0x80);
                if (hit) { pos = (offset + (uint64_t)(__ffsll((unsigned long long)hit) - 1)) & cap; break; }
                index += DBI_GROUP;
                offset = (offset + index) & cap;
            }
            if (pos == ~0ull) break;
            uint64_t edges = 0, cov = 255;                                   // high-copy: the tombstone "look in the 32-bit map"
            if (!e->hc) {
#pragma unroll
                for (int w = 0; w < 4; ++w) edges |= (uint64_t)(e->fw[w] & 0xFF) << (8 * w) | (uint64_t)(e->bw[w] & 0xFF) << (8 * (4 + w));
                cov = e->cov & 0xFF;
            }
            uint8_t* slot = slots + pos * DBI_SLOT;
            dbi_put64(slot, key, lane, 0);
            dbi_put64(slot + 8, edges, lane, 8);
            dbi_put64(slot + 16, cov, lane, 16);
            if (lane == 32) ctrl[pos] = (uint8_t)(h & 0x7F);                                                          // set_ctrl ...
            if (lane == 33) ctrl[((pos - DBI_GROUP) & cap) + 1 + ((DBI_GROUP - 1) & cap)] = (uint8_t)(h & 0x7F);      // ... and its mirrored byte
            __threadfence();
        }
    }
}

// ---- reader ------------------------------------------------------------------------------------------------------------
struct DbiCheck { unsigned long long n_entries, n_tombstones, instances, bad_size, bad_entry, bad_map; };
struct DbiSlot { uint64_t key; uint32_t e[8]; uint32_t cov; };
__device__ __forceinline__ DbiSlot dbi_read_slot(const uint8_t* p) {        // 24 bytes at any alignment
    DbiSlot s;
    s.key = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { s.key |= (uint64_t)p[i] << (8 * i); s.e[i] = p[8 + i]; }
    s.cov = p[16];
    return s;
}
// one workgroup per submap
__global__ __launch_bounds__(256) void k_dbi_check(const uint8_t* __restrict__ img, const DbiExtent* __restrict__ ext, uint32_t k, uint32_t map_count,
                                                    uint32_t map, DbiCheck* __restrict__ res) {
    const DbiExtent x = ext[blockIdx.x];
    uint64_t occupied = 0, n_ent = 0, n_tomb = 0, inst = 0, bad = 0, bad_map = 0;
    for (uint64_t i = threadIdx.x; i < x.cap; i += 256) {
        if (img[x.ctrl_off + i] & 0x80) continue;
        ++occupied;
        const DbiSlot s = dbi_read_slot(img + x.slot_off + i * DBI_SLOT);
        if (s.key % map_count != map) ++bad_map;
        bool ok = s.cov > 0 && s.key != EMPTY_KEY && (k >= 32 || (s.key >> (2 * k)) == 0);
#pragma unroll
        for (int w = 0; w < 8; ++w) ok = ok && s.e[w] <= s.cov;           // an edge is seen at most once per instance
        if (!ok) ++bad;
        if (s.cov == 255) ++n_tomb; else { ++n_ent; inst += s.cov; }
    }
    const uint64_t o = block_sum(occupied), a = block_sum(n_ent), b = block_sum(n_tomb), c = block_sum(inst), d = block_sum(bad), f = block_sum(bad_map);
    if (threadIdx.x == 0) {
        if (a) atomicAdd(&res->n_entries, (unsigned long long)a);
        if (b) atomicAdd(&res->n_tombstones, (unsigned long long)b);
        if (c) atomicAdd(&res->instances, (unsigned long long)c);
        if (d) atomicAdd(&res->bad_entry, (unsigned long long)d);
        if (f) atomicAdd(&res->bad_map, (unsigned long long)f);
        if (o != x.size) atomicAdd(&res->bad_size, 1ull);
    }
}
__global__ __launch_bounds__(256) void k_dbi_add(TableView t, const uint8_t* __restrict__ img, const DbiExtent* __restrict__ ext) {
    const DbiExtent x = ext[blockIdx.x];
    uint32_t n_new = 0;
    uint64_t n_cov = 0;
    for (uint64_t i = threadIdx.x; i < x.cap; i += 256) {
        if (img[x.ctrl_off + i] & 0x80) continue;
        const DbiSlot s = dbi_read_slot(img + x.slot_off + i * DBI_SLOT);
        if (s.cov == 255) continue;                                        // its counters are in .map.hc.bin
        add_logical(t, table_hash(s.key, t.k), s.e, s.cov, n_new, n_cov);
    }
    const uint64_t a = block_sum(n_new), b = block_sum(n_cov);
    if (threadIdx.x == 0) {
        if (a) atomicAdd(&t.st->slots_used, (unsigned long long)a);
        if (b) atomicAdd(&t.st->kmers_added, (unsigned long long)b);
    }
}

}  // namespace kq
