// kreeq_amd.hip -- host side of the C ABI (include/kreeq_amd.h) of the MI355X-native kreeq hot path: handle,
// table sizing, partition planning and kernel launches.  The kernels live in kq_kernels.h (+ kq_device.h,
// kq_partition.h).  gfx950 only; no CPU fallback anywhere in this library.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>       // device radix sort: only for the key order of kq_export (plumbing, not on the hot path)

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/kreeq_amd.h"
#include "kq_device.h"
#include "kq_partition.h"
#include "kq_mem_host.h"
#include "kq_export_host.h"
#include "kq_plan_host.h"
#include "kq_roff_host.h"
#include "kq_seg_gate_host.h"
#include "kq_select_host.h"
#include "kq_bgzf_host.h"

using namespace kq;

#include "kq_kernels.h"
#include "kq_fastx.h"
#include "kq_bgzf.h"
#include "kq_deflate.h"
#include "kq_dbimage.h"
#include "kq_subgraph.h"
#include "kq_gfa.h"
#include "kq_variants.h"
#include "kq_table.h"

// ================================================================================================
// host side
// ================================================================================================

static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}
#define HIPC(expr)                                                                                   \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail(e_ == hipErrorOutOfMemory ? KQ_ERR_NOMEM : KQ_ERR_HIP, "%s: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                  \
    } while (0)

// A device buffer that is contiguous in the virtual address space and SCRAMBLED in the physical one: 2 MiB chunks (hipMemCreate)
// mapped in a permuted order.  Measured: the split level that writes a few thousand sub-bucket streams into a
// multi-GB array runs 15-20 % faster into such a buffer than into one hipMalloc block that happens to be physically contiguous
// (1.97 -> 1.58 ms per slice at 3 Gbp), and a hipMalloc block is or is not contiguous depending on what the process freed before --
// the source of the 1.65 / 2.03 ms cases of that kernel from run to run.  Falls back to hipMalloc if the mapping calls fail.
struct Scrambled {
    void* p = nullptr; size_t bytes = 0, chunk = 0;
    std::vector<hipMemGenericAllocationHandle_t> hs;
    bool vmm = false;

    Scrambled() = default;
    Scrambled(const Scrambled&) = delete;
    Scrambled& operator=(const Scrambled&) = delete;
    Scrambled(Scrambled&& o) noexcept { swap(o); }
    Scrambled& operator=(Scrambled&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~Scrambled() { reset(); }
    void swap(Scrambled& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(chunk, o.chunk); hs.swap(o.hs); std::swap(vmm, o.vmm); }
    friend void swap(Scrambled& a, Scrambled& b) noexcept { a.swap(b); }

    void reset() {
        if (!p) return;
        (void)hipDeviceSynchronize();
        if (vmm) {
            (void)hipMemUnmap(p, hs.size() * chunk);
            for (auto& hnd : hs) (void)hipMemRelease(hnd);
            (void)hipMemAddressFree(p, hs.size() * chunk);
        } else (void)hipFree(p);
        p = nullptr; bytes = chunk = 0; hs.clear(); vmm = false;
    }
    // `n` bytes (what was held goes first): the mapped form where `try_vmm` allows and the mapping calls succeed, else one plain
    // block.  false, with the owner empty and the runtime's error cleared: no memory
    bool alloc(size_t n, int device, bool try_vmm) {
        reset();
        if (try_vmm && map_chunks(n, device)) return true;
        if (hipMalloc(&p, n) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
        bytes = n; vmm = false;
        return true;
    }
private:
    bool map_chunks(size_t n_bytes, int device) {
        static const size_t chunk_mb = getenv("KQ_SCRAMBLE_MB") ? (size_t)atoi(getenv("KQ_SCRAMBLE_MB")) : 2;      // 0: plain hipMalloc (A/B)
        if (!chunk_mb) return false;
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = device;
        size_t gran = 0;
        if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) != hipSuccess || !gran) { (void)hipGetLastError(); return false; }
        const size_t ck = ((chunk_mb << 20) + gran - 1) / gran * gran, n = (n_bytes + ck - 1) / ck;
        void* base = nullptr;
        if (hipMemAddressReserve(&base, n * ck, 0, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
        std::vector<hipMemGenericAllocationHandle_t> fresh;
        fresh.reserve(n);
        bool ok = true;
        for (size_t i = 0; i < n && ok; ++i) { hipMemGenericAllocationHandle_t hnd; ok = hipMemCreate(&hnd, ck, &prop, 0) == hipSuccess; if (ok) fresh.push_back(hnd); }
        size_t mapped = 0;
        if (ok) {
            size_t mul = 7919;                                             // chunk i of the virtual range = physical chunk (i * mul + 13) mod n
            while (std::gcd(mul, n) != 1) ++mul;
            for (; mapped < n && ok; ++mapped) ok = hipMemMap((char*)base + mapped * ck, ck, 0, fresh[(mapped * mul + 13) % n], 0) == hipSuccess;
            if (!ok) --mapped;
        }
        if (ok) {
            hipMemAccessDesc acc = {};
            acc.location = prop.location; acc.flags = hipMemAccessFlagsProtReadWrite;
            ok = hipMemSetAccess(base, n * ck, &acc, 1) == hipSuccess;
        }
        if (!ok) {
            (void)hipGetLastError();
            if (mapped) (void)hipMemUnmap(base, mapped * ck);
            for (auto& hnd : fresh) (void)hipMemRelease(hnd);
            (void)hipMemAddressFree(base, n * ck);
            return false;
        }
        p = base; bytes = n * ck; chunk = ck; hs.swap(fresh); vmm = true;
        return true;
    }
};
static int scr_ensure(Scrambled& b, size_t need, int device) {
    if (b.bytes >= need) return KQ_OK;
    b.reset();                                                     // (before the new size is taken: the peak is one buffer)
    const size_t sz = need + std::min<size_t>(need / 4, (size_t)256 << 20) + 4096;
    if (!b.alloc(sz, device, true)) return fail(KQ_ERR_NOMEM, "partition scratch allocation failed");
    return KQ_OK;
}

// the scratch of one partition plan (plan_alloc): record buffers + offsets, and the second record array of large plans (the
// middle level's output)
struct ScratchSet { DevMem part; Scrambled part2; };

// Every resource below is an owner (kq_mem_host.h, Scrambled): `delete h` frees it, kq_destroy sets the device and drains the
// streams first.  Members go in reverse order of declaration: the handle's own stream last.
struct kq_handle {
    int device = 0, k = 0, map_count = 0;
    Stream own_stream;
    hipStream_t stream = nullptr;
    int n_cu = 256;
    DevMem slots;                    // Slot[n_slots()]
    uint64_t n_regions = 0;          // of the table's geometry (the scale of the hash -> region map)
    // window (multi-GPU shards, KQ_OPT_BUCKET_WINDOW / KQ_OPT_SHARD_WINDOW): only the regions of the hash-prefix buckets [win_lo, win_hi) are
    // allocated; `slots` is the allocation, view().slots the address region 0 would have
    uint32_t win_lo = 0, win_hi = 256;
    bool windowed = false;
    DevMem hc;                       // HcSlot[hc_cap]
    uint64_t hc_cap = 0;
    DevMem rstart;                   // u32: first top-32 hash value of every region (n_regions + 1 entries)
    DevMem st;                       // DevState
    PinnedMem st_host;               // its pinned mirror
    // scratch (grown on demand)
    DevMem scratch;
    DevMem stage;                    // device staging for host-buffer entry points
    uint64_t kmers_bound = 0;        // upper bound of instances inserted (sizing the side table)
    uint64_t used_bound = 0;         // upper bound of occupied slots (skips the state read-back)
    uint64_t hc_check_at = 0;        // instance count from which the side table's fill is looked at again (reserve)
    bool table_empty = true;         // nothing inserted since kq_create / kq_clear
    uint32_t mid_rps = 2048;         // KQ_OPT_NARROW_MID: regions per hash-prefix bucket from which the split gets a middle level
    int merge_path = 0;              // KQ_OPT_MERGE_PATH (of the destination handle): 0 auto, 1 per-entry atomics, 2 region by region
    int lookup_path = 0;             // KQ_OPT_LOOKUP_PATH: 0 auto, 1 direct (k_lookup), 2 partitioned (k_lookup_regions)
    bool slots_dirty = false;        // the slot array is logically empty but its memory is not initialised yet (lazy clear)
    bool trust_capacity = false;     // KQ_OPT_TRUST_CAPACITY: capacity_hint bounds the distinct k-mers
    int count_path = 0;              // KQ_OPT_COUNT_PATH: 0 auto, 1 direct (global atomics), 2 partitioned
    uint64_t slice_kmers = 1ull << 28;   // KQ_OPT_SLICE_KMERS
    bool slice_user = false;             // set explicitly: no automatic enlargement
    uint32_t filt_lo = 0, filt_hi = 0;   // KQ_OPT_COUNT_MAP_RANGE (set to [0, map_count) at creation)
    bool profile = false;                // KQ_OPT_PROFILE: HIP events around the stages of the partitioned count
    std::vector<std::pair<const char*, Event>> marks;
    ScratchSet work, fork_work;                        // partitioned path: the scratch plans are carved from, and the fork's
    // Fork / join of the slices of ONE count call (see count_seq_dev): consecutive slices run their partition stages on two
    // internal streams with a scratch set each, so that slice j+1's P1 fills the issue slots slice j's levels leave idle.
    // `stream` is where launches go (a fork stream while a forked slice is being enqueued), `base` the handle's stream
    // (its own or the caller's): everything that reads the table or the device state runs there, behind a join.
    hipStream_t base = nullptr;
    Stream fork_stream[2];
    bool fork_busy[2] = {false, false};              // work enqueued on the fork stream that `base` has not been joined with
    static constexpr int EV_RING = 64;
    Event ev_ring[EV_RING];                          // fork / join / pass events, used round-robin: an event is re-recorded only
    uint64_t ev_next = 0;                            // after the host has seen its previous use complete (ev_get)
    int overlap = 1;                                 // KQ_OPT_OVERLAP
    int kernel_set = 0;                              // KQ_OPT_KERNEL_SET (measurement only)
    // KQ_OPT_COUNT_MAP_PASSES: count matrices of resident batches, made for all map ranges by the first pass that scans a slice
    struct HistKey { const void* ab; const void* pinv; uint64_t lead, len, er_lo, er_hi; uint32_t g1, n_rng; int k;
                     bool operator==(const HistKey& o) const { return ab == o.ab && pinv == o.pinv && lead == o.lead && len == o.len && er_lo == o.er_lo && er_hi == o.er_hi && g1 == o.g1 && n_rng == o.n_rng && k == o.k; } };
    struct HistEntry { HistKey key; DevMem m1_all; };
    std::vector<HistEntry> hist_cache;
    size_t hist_cache_bytes = 0;
    int map_passes = 1;
    // pending record sets (see "pending sets" below): region-sorted records of earlier slices / batches that have not
    // been applied to the table yet; one k_count_regions pass takes them all
    Scrambled arena;                     // (a scrambled buffer from 1 GiB up: KQ_SCRAMBLE_ARENA)
    size_t arena_bytes = 0, arena_used = 0;
    DevMem d_sets;                       // P3Set[P3_MAX_SETS]
    P3Set pend_sets[P3_MAX_SETS] = {};   // the same on the host: the record pointers travel in k_count_regions_q4r's argument block
    DevMem tot;                          // u64 [TOT_LINES][8] partial sums of a table pass (k_fold_totals), zero between passes
    DevMem roff;                         // region-major offset matrix of a table pass (k_p3_region_offsets): (allocated regions + 1) x P3_MAX_SETS u32
    int n_pend = 0, pend_fmt = -1, pend_aux_fmt = 0;
    uint64_t pend_records = 0;           // upper bound of the records in the pending sets
    int64_t pend_budget = -1;            // KQ_OPT_PENDING_BYTES: -1 auto, 0 = apply every slice at once
    uint64_t table_passes = 0;           // k_count_regions passes so far
    // pipelined host ingest (kq_count_batch_async): copies on their own stream into a ring of device staging buffers
    static constexpr int IN_SLOTS = 3, IN_TICKETS = 512;
    Stream copy_stream;
    DevMem in_buf[IN_SLOTS];
    Event in_consumed[IN_SLOTS];         // the count that read the slot has been enqueued and finished
    std::vector<Event> in_copied;        // ring of "copy of ticket t done" events
    uint64_t in_next = 0;
    std::mutex in_m;                     // kq_count_batch_async may be called from several threads: the calls take turns
    uint8_t in_bad[IN_TICKETS] = {};     // format (KQ_FASTX_*) whose rules the text of a ticket broke (kq_count_fastx_async), else 0
    // device FASTQ / FASTA parser (kq_fastx.h): unit summaries, the compact read batch of kq_count_fastx_dev and, per ring
    // slot, of kq_count_fastx_async (the slot's in_buf keeps the raw text), the chain's result and its page-locked mirror
    DevMem fx_units, fx_out, in_cmp[IN_SLOTS];
    DevMem fx_res;                       // FxResult
    PinnedMem fx_res_host;               // its pinned mirror
    int fx_bad = 0;                      // a counted text broke its format: reported by kq_sync until kq_clear
    // BGZF members on the device (kq_bgzf.h): the members' descriptors and their page-locked staging, the status record and its
    // mirror, the text of one call (carry + the call's members) and the carry of a kq_count_bgzf_dev stream between calls
    DevMem bz_desc, bz_stat, bz_text, bz_carry;
    PinnedMem bz_desc_host, bz_stat_host;
    // the BGZF writer (kq_deflate.h): a batch's member slots, their sizes and output offsets, the status record and its mirror,
    // and the staging of the host-buffer form
    DevMem df_slots, df_sizes, df_offs, df_stat, df_in, df_out;
    PinnedMem df_stat_host;
    uint64_t bz_carry_len = 0;
    bool bz_bad = false;                 // a counted BGZF member was corrupt: reported by kq_sync until kq_clear
    std::string bz_err;                  // its message
    bool hist_cache_off = false;         // the batch being counted lives in a library-owned buffer, which keeps its address and
                                         // changes its content: the address-keyed KQ_OPT_COUNT_MAP_PASSES cache must not see it
    bool test_fail_plan = false;         // KQ_OPT_TEST_FAIL_PLAN: the next partition plan fails with KQ_ERR_NOMEM (failure-path tests)
    int test_export = 0;                 // KQ_OPT_TEST_EXPORT: bit 0 = sort_entries_dev finds no memory, bit 1 = copy_out_bounced takes chunks of 4096 bytes at any size (tests)
    DevMem hot;                          // k_count_regions' list of skewed regions
    uint64_t var_batch = 0;              // KQ_OPT_VARIANT_BATCH: searches per batch of kq_search_variants, 0 = from the scratch budget
    uint64_t sg_batch = 0;               // KQ_OPT_SUBGRAPH_BATCH: searches per batch of kq_subgraph_best_first, 0 = from the scratch budget
    std::vector<DevMem> user_mem;        // kq_dev_alloc: blocks lent to a caller that does not link the runtime
    DevMem tab_segs;                     // kq_per_base_triples_dev: the segment lists of the last call (it returns before its kernel ends)

    TableView view() const {
        TableView v; v.slots = slots.as<Slot>() - (reg_lo() << REGION_SHIFT); v.n_regions = n_regions; v.hc = hc.as<HcSlot>(); v.hc_mask = hc_cap - 1; v.st = d_state(); v.k = (uint32_t)k;
        v.reg_lo = reg_lo(); v.reg_hi = reg_hi();
        v.rps = k >= HI_K ? (uint32_t)(n_regions >> 8) : 0u;
        v.rstart = rstart.as<uint32_t>();
        return v;
    }
    DevState* d_state() const { return st.as<DevState>(); }
    DevState* host_state() const { return st_host.as<DevState>(); }
    FxResult* fx_host() const { return fx_res_host.as<FxResult>(); }
    uint64_t reg_lo() const { return windowed ? (uint64_t)win_lo * (n_regions >> 8) : 0; }
    uint64_t reg_hi() const { return windowed ? (uint64_t)win_hi * (n_regions >> 8) : n_regions; }
    uint64_t n_alloc_regions() const { return reg_hi() - reg_lo(); }
    uint64_t n_slots() const { return n_alloc_regions() << REGION_SHIFT; }      // allocated slots
    uint64_t table_bytes() const { return n_slots() * sizeof(Slot); }
    TableShape shape() const { return TableShape{k, n_regions, map_count, mid_rps}; }      // what a partition plan depends on (kq_plan_host.h)
};

static void marks_reset(kq_handle* h);
static int flush_pending(kq_handle* h);

// ---- fork / join (count_seq_dev) ----------------------------------------------------------------------------------
// One event per use: the ring hands out an event whose previous record has completed (the host waits for it if it has
// not: that bounds how far the host runs ahead to EV_RING forks / joins).  Re-recording an event that a queued
// hipStreamWaitEvent still refers to is exactly what this avoids.
static int ev_get(kq_handle* h, hipEvent_t* out) {
    Event& e = h->ev_ring[h->ev_next++ % kq_handle::EV_RING];
    if (!e) HIPC(e.create(hipEventDisableTiming));
    else HIPC(hipEventSynchronize(e.get()));
    *out = e.get();
    return KQ_OK;
}
// `base` waits for everything the fork streams have been given
static int join_forks(kq_handle* h) {
    for (int w = 0; w < 2; ++w) {
        if (!h->fork_busy[w]) continue;
        hipEvent_t e; int rc = ev_get(h, &e); if (rc) return rc;
        HIPC(hipEventRecord(e, h->fork_stream[w].get()));
        HIPC(hipStreamWaitEvent(h->base, e, 0));
        h->fork_busy[w] = false;
    }
    return KQ_OK;
}

// grid-stride kernels: at most `per_cu` workgroups per CU.  8 = what is resident (kernels that flush per-workgroup
// state at the end); the tile scanners take 32: the dispatcher balances the surplus (-4 % on k_lookup / k_count_direct)
static int grid_for(const kq_handle* h, uint64_t work_items, int per_block, int per_cu = 8) {
    uint64_t blocks = (work_items + per_block - 1) / per_block;
    uint64_t cap = (uint64_t)h->n_cu * per_cu;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

static void clear_words(kq_handle* h, void* p, uint32_t words_per_slot, uint64_t n_slots) {
    const uint64_t n_pairs = n_slots * words_per_slot / 2;      // both table sizes make this exact
    hipLaunchKernelGGL(k_clear_slots, dim3(grid_for(h, n_pairs, 256)), dim3(256), 0, h->stream, (ulonglong2*)p, words_per_slot, n_pairs);
}
// an empty main table is all zero bytes (w0 == 0 <=> free slot)
static void clear_main(kq_handle* h, Slot* p, uint64_t n_slots) { (void)hipMemsetAsync(p, 0, (size_t)n_slots * sizeof(Slot), h->stream); }
// lazy kq_clear: give the slot array its empty image now (every table user except the partitioned count)
static void materialize(kq_handle* h) {
    if (!h->slots_dirty) return;
    clear_main(h, h->slots.as<Slot>(), h->n_slots());
    h->slots_dirty = false;
}
// `alloc_regions` of the n_regions of the geometry get memory (all of them unless the table is a window).  `slots` and `rstart`
// are the caller's (empty) owners: the handle's own at creation, locals where a table replaces one
static int alloc_main(kq_handle* h, uint64_t n_regions, uint64_t alloc_regions, DevMem& slots, DevMem& rstart) {
    HIPC(slots.alloc((size_t)(alloc_regions << REGION_SHIFT) * sizeof(Slot)));
    if (rstart.alloc((size_t)(n_regions + 1) * sizeof(uint32_t)) != hipSuccess) { slots.reset(); return fail(KQ_ERR_NOMEM, "region index allocation failed"); }
    clear_main(h, slots.as<Slot>(), alloc_regions << REGION_SHIFT);
    hipLaunchKernelGGL(k_region_starts, dim3(grid_for(h, n_regions + 1, 256)), dim3(256), 0, h->stream, rstart.as<uint32_t>(), n_regions);
    return KQ_OK;
}
static int alloc_hc(kq_handle* h, uint64_t cap, DevMem& hc) {
    HIPC(hc.alloc((size_t)cap * sizeof(HcSlot)));
    clear_words(h, hc.get(), sizeof(HcSlot) / 8, cap);
    return KQ_OK;
}

static int read_state_raw(kq_handle* h) {
    HIPC(hipMemcpyAsync(h->host_state(), h->d_state(), sizeof(DevState), hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    return KQ_OK;
}
static int read_state(kq_handle* h) {
    int frc = flush_pending(h);          // the device state speaks for everything counted so far
    if (frc) return frc;
    return read_state_raw(h);
}
static int check_errors(kq_handle* h) {
    int rc = read_state(h);
    if (rc) return rc;
    if (h->host_state()->err_table_full) return fail(KQ_ERR_TABLE_FULL, "k-mer table region overflow (slots %llu / %llu)",
                                                 (unsigned long long)h->host_state()->slots_used, (unsigned long long)h->n_slots());
    if (h->host_state()->err_hc_full) return fail(KQ_ERR_TABLE_FULL, "high-copy side table overflow (%llu / %llu)",
                                              (unsigned long long)h->host_state()->hc_used, (unsigned long long)h->hc_cap);
    return KQ_OK;
}

// grow (rehash) so that `extra` more distinct k-mers fit at load <= 0.85, and the side table can
// take every k-mer that may reach cov >= 255 after `extra_instances` more instances.
static int grow_main(kq_handle* h, uint64_t need_slots) {
    int frc = flush_pending(h);          // pending records are sorted by the regions of the current geometry
    if (frc) return frc;
    const GrowTarget grown = grow_target(h->n_slots(), h->n_regions, need_slots);
    const uint64_t want = grown.slots, new_regions = grown.regions;
    if (!grown.ok) return fail(KQ_ERR_TABLE_FULL, "cannot grow k-mer table to %llu slots: region index overflow", (unsigned long long)want);
    // the new table in local owners; after the swap they hold the old one, which goes at scope exit on every way out: behind
    // the stream synchronisation below (the rehash reads it), or, if that fails, through a free that waits for the device
    DevMem slots, rstart;
    int rc = alloc_main(h, new_regions, want >> REGION_SHIFT, slots, rstart);
    if (rc) return rc == KQ_ERR_NOMEM ? fail(KQ_ERR_TABLE_FULL, "cannot grow k-mer table to %llu slots: out of device memory",
                                             (unsigned long long)want) : rc;
    const uint64_t n_old = h->n_slots();
    const TableView old_view = h->view();
    slots.swap(h->slots); rstart.swap(h->rstart);
    h->n_regions = new_regions;
    if (h->slots_dirty) h->slots_dirty = false;     // lazily cleared table: nothing to move, and the fresh array is clean
    else hipLaunchKernelGGL(k_rehash, dim3(grid_for(h, n_old, 256)), dim3(256), 0, h->stream, h->view(), old_view);
    HIPC(hipStreamSynchronize(h->stream));
    return KQ_OK;
}
static int grow_hc(kq_handle* h, uint64_t need) {
    uint64_t want = h->hc_cap;
    while (want < need) want *= 2;
    DevMem hc;                                      // the new side table; the old one after the swap (see grow_main)
    int rc = alloc_hc(h, want, hc);
    if (rc) return rc;
    const uint64_t n_old = h->hc_cap;
    hc.swap(h->hc); h->hc_cap = want;
    HIPC(hipMemsetAsync(&h->d_state()->hc_used, 0, sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(k_rehash_hc, dim3(grid_for(h, n_old, 256)), dim3(256), 0, h->stream, h->view(), hc.as<HcSlot>(), n_old);
    HIPC(hipStreamSynchronize(h->stream));
    return KQ_OK;
}

// Make room for a batch that may add `extra` distinct k-mers and `extra_instances` instances.
//  main table : load <= 0.85 even if every k-mer of the batch is new (unless the caller vouched for
//               capacity_hint with KQ_OPT_TRUST_CAPACITY); host-side upper bounds avoid a device round trip.
//  side table : #k-mers with cov >= 255 <= instances / 255; kept at load <= 0.5 up to 2^23 entries
//               (1.2 GB); beyond that growth follows the observed fill.
static int reserve(kq_handle* h, uint64_t extra, uint64_t extra_instances) {
    int rc;
    bool state_read = false;
    if (!h->trust_capacity) {
        uint64_t need = main_need(h->used_bound, extra);
        if (need > h->n_slots()) {
            rc = read_state(h); if (rc) return rc;
            state_read = true;
            h->used_bound = h->host_state()->slots_used;
            need = main_need(h->used_bound, extra);
            if (need > h->n_slots()) { rc = grow_main(h, need); if (rc) return rc; }
        }
    }
    h->used_bound += extra;
    h->kmers_bound += extra_instances;
    // side table: provable sizing (one entry per 255 instances, load <= 0.5) up to 2^23 entries; beyond that it
    // follows the observed fill with room for an eightfold growth of the high-copy set (as coverage doubles, the copy
    // number that reaches cov 255 halves): looked at once per doubling of the instance count here, and before every
    // table pass over pending records (flush_pending).  A side table that fills up anyway is reported as
    // KQ_ERR_TABLE_FULL by the next synchronising call
    uint64_t need_hc = hc_need(h->kmers_bound);
    if (hc_follows_fill(h->kmers_bound) && h->kmers_bound >= h->hc_check_at && h->n_pend == 0) {
        if (!state_read) { rc = read_state_raw(h); if (rc) return rc; }
        need_hc = hc_need(h->kmers_bound, h->host_state()->hc_used);
        h->hc_check_at = 2 * h->kmers_bound;
    }
    if (need_hc > h->hc_cap) { rc = grow_hc(h, need_hc); if (rc) return rc; }
    return KQ_OK;
}

static int stage_in(kq_handle* h, const void* host, size_t bytes, void** dev) {
    HIPC(h->stage.ensure(bytes + 64));
    if (bytes) HIPC(hipMemcpyAsync(h->stage.get(), host, bytes, hipMemcpyHostToDevice, h->stream));
    *dev = h->stage.get();
    return KQ_OK;
}

// sort by key with a few host threads: chunk sorts, then pairwise merges
static void parallel_sort_entries(kq_entry* a, uint64_t n) {
    auto less = [](const kq_entry& x, const kq_entry& y) { return x.key < y.key; };
    unsigned hw = std::thread::hardware_concurrency();
    unsigned t = std::max(1u, std::min(16u, hw ? hw : 1u));
    while (t > 1 && n / t < (1u << 16)) t /= 2;
    if (t <= 1) { std::sort(a, a + n, less); return; }
    std::vector<uint64_t> cut(t + 1);
    for (unsigned i = 0; i <= t; ++i) cut[i] = n * i / t;
    {
        std::vector<std::thread> th;
        for (unsigned i = 0; i < t; ++i) th.emplace_back([&, i] { std::sort(a + cut[i], a + cut[i + 1], less); });
        for (auto& x : th) x.join();
    }
    for (unsigned width = 1; width < t; width *= 2) {
        std::vector<std::thread> th;
        for (unsigned i = 0; i + width < t; i += 2 * width) {
            const uint64_t lo = cut[i], mid = cut[i + width], hi = cut[std::min(i + 2 * width, t)];
            th.emplace_back([=] { std::inplace_merge(a + lo, a + mid, a + hi, less); });
        }
        for (auto& x : th) x.join();
    }
}

// ---- kernel rows: a row pairs a descriptor of the selector (kq_select_host.h) with the instantiation it names.  The launchers
// below list the rows of each family once; launch_row runs the row equal to `s`, and a descriptor that no row has is an error,
// never another kernel
template <class Fn> struct KernelRow { KernelSel sel; Fn fn; };
template <class Fn, size_t N, class... A>
static int launch_row(const KernelRow<Fn> (&rows)[N], const char* family, const KernelSel& s, kq_handle* h, dim3 grid, dim3 block, A... args) {
    for (const KernelRow<Fn>& r : rows) if (r.sel == s) { hipLaunchKernelGGL(r.fn, grid, block, 0, h->stream, args...); return KQ_OK; }
    return fail(KQ_ERR_INVALID, "%s has no instantiation <fmt %d, nbc %d, bin %d, kc %d, tpr %d, flag %d> (selector family %d)", family, s.fmt, s.nbc, s.bin, s.kc, s.tpr, (int)s.flag, (int)s.fam);
}
template <int B, int K> static KernelRow<decltype(&k_p1_hist<0, 0>)> p1h() { return {sel_of(K_P1_HIST, 0, 0, B, K), k_p1_hist<B, K>}; }
template <int W, int N, int B, int K> static KernelRow<decltype(&k_p1_scatter<0, 512, 0, 0>)> p1w() { return {sel_of(K_P1_SCATTER, W, N, B, K), k_p1_scatter<W, N, B, K>}; }
template <int B, int K, int T, bool TOP8 = false> static KernelRow<decltype(&k_p1_scatter_s<0, 0, 1>)> p1s() { return {sel_of(K_P1_SCATTER_S, 0, 0, B, K, T, TOP8), k_p1_scatter_s<B, K, T, TOP8>}; }
template <int K> static KernelRow<decltype(&k_p1_scatter_c<0>)> p1c() { return {sel_of(K_P1_SCATTER_C, 0, 0, 0, K), k_p1_scatter_c<K>}; }
template <int W> static KernelRow<decltype(&k_lv_hist<0>)> lvh() { return {sel_of(K_LV_HIST, W, 0, 0, 0), k_lv_hist<W>}; }
template <int W, int N> static KernelRow<decltype(&k_lv_scatter<0, 512>)> lvw() { return {sel_of(K_LV_SCATTER, W, N, 0, 0), k_lv_scatter<W, N>}; }
template <bool T> static KernelRow<decltype(&k_lv_scatter_s<false>)> lvs() { return {sel_of(K_LV_SCATTER_S, 0, 0, 0, 0, 0, T), k_lv_scatter_s<T>}; }
template <int W, bool HOT> static KernelRow<decltype(&k_count_regions<0, false>)> p3g() { return {sel_of(K_COUNT_REGIONS, W, 0, 0, 0, 0, HOT), k_count_regions<W, HOT>}; }
template <int K, bool T> static KernelRow<decltype(&k_count_regions_q4<0, false>)> p3q() { return {sel_of(K_COUNT_REGIONS_Q4, 0, 0, 0, K, 0, T), k_count_regions_q4<K, T>}; }
template <int K, bool T> static KernelRow<decltype(&k_count_regions_q4r<0, false>)> p3r() { return {sel_of(K_COUNT_REGIONS_Q4R, 0, 0, 0, K, 0, T), k_count_regions_q4r<K, T>}; }
template <int W> static KernelRow<decltype(&k_lookup_regions<0>)> lkr() { return {sel_of(K_LOOKUP_REGIONS, W, 0, 0, 0), k_lookup_regions<W>}; }

extern "C" {

const char* kq_last_error(void) { return g_err.c_str(); }
int kq_abi_version(void) { return KQ_ABI_VERSION; }

int kq_device_available(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return 0;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) return 0;
    return strncmp(p.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

int kq_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes) {
    if (!free_bytes || !total_bytes) return fail(KQ_ERR_INVALID, "null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(KQ_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= n) return fail(KQ_ERR_NO_DEVICE, "device %d out of range (%d visible)", device, n);
    HIPC(hipSetDevice(device));
    size_t f = 0, t = 0;
    HIPC(hipMemGetInfo(&f, &t));
    *free_bytes = f; *total_bytes = t;
    return KQ_OK;
}

// KQ_OPT_BUCKET_WINDOW: the (empty) table becomes the window [lo, hi) of the 256 hash-prefix buckets of a geometry that is
// 256 / (hi - lo) times larger: the memory stays what kq_create sized, the handle then holds -- and answers for -- only
// the k-mers of those buckets (a multi-GPU shard; kq_insert_sharded_dev / kq_insert_sharded8_dev bring them).
// `shard` (KQ_OPT_SHARD_WINDOW): also for k >= HI_K, whose tables have the bucket geometry at every size and whose slots take
// their top 8 hash bits from the region -- the VIRTUAL region (view().slots is the address region 0 would have), so a window
// changes nothing in slot_hash / slot_hash_at
static int set_window(kq_handle* h, uint32_t lo, uint32_t hi, bool shard = false) {
    if (lo >= hi || hi > 256) return fail(KQ_ERR_INVALID, "bucket window [%u, %u) is not a range of the 256 hash-prefix buckets", lo, hi);
    if (shard && h->k > (int)NARROW_MAX_K && h->k < HI_K)
        return fail(KQ_ERR_INVALID, "shard windows need k <= %u (5-byte records) or k >= %d (8-byte hash-remainder records); k = %u..%d shards own map ranges", NARROW_MAX_K, HI_K, NARROW_MAX_K + 1, HI_K - 1);
    if (!shard && h->k > (int)NARROW_MAX_K) return fail(KQ_ERR_INVALID, "bucket windows need k <= %u (5-byte records)", NARROW_MAX_K);
    if (!h->table_empty || h->n_pend || h->kmers_bound) return fail(KQ_ERR_INVALID, "the bucket window is chosen before anything is counted");
    // an empty windowed table moves to another window of the same width without a new allocation (bucket-range passes of one
    // GPU: count the buckets [0, 128), clear, count [128, 256) into the same memory)
    if (h->windowed && hi - lo == h->win_hi - h->win_lo && !(lo == 0 && hi == 256)) {
        HIPC(hipStreamSynchronize(h->stream));
        h->win_lo = lo; h->win_hi = hi;
        return KQ_OK;
    }
    const WindowGeom g = window_geometry(h->n_alloc_regions(), lo, hi, h->k);
    if (!g.ok) return fail(KQ_ERR_INVALID, "bucket window too narrow for a table of %llu regions", (unsigned long long)h->n_alloc_regions());
    HIPC(hipStreamSynchronize(h->stream));
    // the new table first: a failed allocation leaves the handle as it was
    DevMem slots, rstart;
    int rc = alloc_main(h, g.virt, g.alloc_new, slots, rstart);
    if (rc) return rc;
    HIPC(hipStreamSynchronize(h->stream));
    slots.swap(h->slots); rstart.swap(h->rstart);          // (the old table goes at scope exit)
    h->n_regions = g.virt; h->win_lo = lo; h->win_hi = hi; h->windowed = !(lo == 0 && hi == 256);
    h->slots_dirty = false;
    return KQ_OK;
}

int kq_create(kq_handle** out, int device, int k, int map_count, uint64_t capacity_hint) {
    if (!out) return fail(KQ_ERR_INVALID, "out is null");
    *out = nullptr;
    if (k < 2 || k > 32) return fail(KQ_ERR_INVALID, "k must be in 2..32 (got %d)", k);       // src/input.cpp:142
    if (map_count < 1 || map_count > 65535) return fail(KQ_ERR_INVALID, "map_count must be in 1..65535 (got %d)", map_count);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(KQ_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= n) return fail(KQ_ERR_NO_DEVICE, "device %d out of range (%d visible)", device, n);
    HIPC(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPC(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(KQ_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);
    kq_handle* h = new (std::nothrow) kq_handle();
    if (!h) return fail(KQ_ERR_NOMEM, "host allocation failed");
    h->device = device; h->k = k; h->map_count = map_count; h->n_cu = prop.multiProcessorCount;
    h->filt_hi = (uint32_t)map_count;
    hipError_t e = h->own_stream.create(hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(KQ_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    h->stream = h->base = h->own_stream.get();
    int rc = KQ_OK;
    do {
        if (h->st.alloc(sizeof(DevState)) != hipSuccess || h->st_host.alloc(sizeof(DevState)) != hipSuccess) {
            rc = fail(KQ_ERR_NOMEM, "state allocation failed"); break;
        }
        (void)hipMemsetAsync(h->d_state(), 0, sizeof(DevState), h->stream);
        const uint64_t regions = initial_regions(capacity_hint, k);
        rc = alloc_main(h, regions, regions, h->slots, h->rstart); if (rc) break;
        h->n_regions = regions;
        uint64_t hc = 1u << 16;
        rc = alloc_hc(h, hc, h->hc); if (rc) break;
        h->hc_cap = hc;
        if (hipStreamSynchronize(h->stream) != hipSuccess) { rc = fail(KQ_ERR_HIP, "table initialisation failed"); break; }
    } while (0);
    if (rc) { kq_destroy(h); return rc; }
    *out = h;
    return KQ_OK;
}

// set the device, drain the streams, delete: every member of the handle frees what it holds
void kq_destroy(kq_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& s : h->fork_stream) if (s) (void)hipStreamSynchronize(s.get());
    if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream.get());
    delete h;
}

int kq_clear(kq_handle* h) {
    if (!h) return fail(KQ_ERR_INVALID, "null handle");
    HIPC(hipSetDevice(h->device));
    h->slots_dirty = true;           // the 24 B/slot clear is folded into the next partitioned count (k_count_regions writes every region); anything else materialises it first
    clear_words(h, h->hc.get(), sizeof(HcSlot) / 8, h->hc_cap);
    HIPC(hipMemsetAsync(h->d_state(), 0, sizeof(DevState), h->stream));
    h->kmers_bound = 0;
    h->used_bound = 0;
    h->hc_check_at = 0;
    h->table_empty = true;
    h->n_pend = 0; h->arena_used = 0; h->pend_records = 0;      // records not applied yet are dropped with the rest
    h->fx_bad = 0;
    h->bz_bad = false; h->bz_carry_len = 0;      // an open kq_count_bgzf_dev stream is dropped
    return KQ_OK;
}

int kq_set_stream(kq_handle* h, void* s) {
    if (!h) return fail(KQ_ERR_INVALID, "null handle");
    HIPC(hipStreamSynchronize(h->stream));
    h->stream = h->base = s ? (hipStream_t)s : h->own_stream.get();
    return KQ_OK;
}
int kq_set_option(kq_handle* h, int option, int64_t value) {
    if (!h) return fail(KQ_ERR_INVALID, "null handle");
    switch (option) {
        case KQ_OPT_TRUST_CAPACITY: h->trust_capacity = value != 0; return KQ_OK;
        case KQ_OPT_COUNT_PATH:
            if (value < 0 || value > 2) return fail(KQ_ERR_INVALID, "KQ_OPT_COUNT_PATH must be 0, 1 or 2");
            h->count_path = (int)value; return KQ_OK;
        case KQ_OPT_COUNT_MAP_RANGE: {
            const int64_t lo = value & 0xFFFF, hi = (value >> 16) & 0xFFFF;
            if (lo >= hi || hi > h->map_count) return fail(KQ_ERR_INVALID, "map range [%lld,%lld) outside [0,%d]", (long long)lo, (long long)hi, h->map_count);
            h->filt_lo = (uint32_t)lo; h->filt_hi = (uint32_t)hi; return KQ_OK;
        }
        case KQ_OPT_NARROW_MID:
            if (value < 2 || value > (1 << 14)) return fail(KQ_ERR_INVALID, "KQ_OPT_NARROW_MID must be in [2, 16384]");
            h->mid_rps = (uint32_t)value; return KQ_OK;
        case KQ_OPT_MERGE_PATH:
            if (value < 0 || value > 2) return fail(KQ_ERR_INVALID, "KQ_OPT_MERGE_PATH must be 0, 1 or 2");
            h->merge_path = (int)value; return KQ_OK;
        case KQ_OPT_LOOKUP_PATH:
            if (value < 0 || value > 2) return fail(KQ_ERR_INVALID, "KQ_OPT_LOOKUP_PATH must be 0, 1 or 2");
            h->lookup_path = (int)value; return KQ_OK;
        case KQ_OPT_PROFILE: h->profile = value != 0; if (!h->profile) marks_reset(h); return KQ_OK;
        case KQ_OPT_TEST_FAIL_PLAN: h->test_fail_plan = value != 0; return KQ_OK;
        case KQ_OPT_TEST_EXPORT:
            if (value < 0 || value > 3) return fail(KQ_ERR_INVALID, "KQ_OPT_TEST_EXPORT must be in [0, 3]");
            h->test_export = (int)value; return KQ_OK;
        case KQ_OPT_COUNT_MAP_PASSES: {
            if (value != 1 && value != 2 && value != 4 && value != 8) return fail(KQ_ERR_INVALID, "KQ_OPT_COUNT_MAP_PASSES must be 1, 2, 4 or 8");
            if ((h->map_count & (h->map_count - 1)) != 0 || value > h->map_count) return fail(KQ_ERR_INVALID, "KQ_OPT_COUNT_MAP_PASSES needs a power-of-two map count");
            HIPC(hipStreamSynchronize(h->stream));
            h->hist_cache.clear(); h->hist_cache_bytes = 0;
            h->map_passes = (int)value; return KQ_OK;
        }
        case KQ_OPT_KERNEL_SET:
            if (value < 0 || (value & ~(int64_t)KS_ALL)) return fail(KQ_ERR_INVALID, "KQ_OPT_KERNEL_SET is a mask of bits 1, 2, 4, 16, 32, 64, 128");
            h->kernel_set = (int)value; return KQ_OK;
        case KQ_OPT_OVERLAP:
            if (value < 0 || value > 2) return fail(KQ_ERR_INVALID, "KQ_OPT_OVERLAP must be 0, 1 or 2");
            h->overlap = (int)value; return KQ_OK;
        case KQ_OPT_PENDING_BYTES: {
            if (value < -1) return fail(KQ_ERR_INVALID, "KQ_OPT_PENDING_BYTES must be -1 (auto), 0 (off) or a byte count");
            int rc = flush_pending(h);
            if (rc) return rc;
            if (h->arena.p && value != h->pend_budget) { HIPC(hipStreamSynchronize(h->stream)); h->arena.reset(); h->arena_bytes = 0; }
            h->pend_budget = value; return KQ_OK;
        }
        case KQ_OPT_BUCKET_WINDOW:
            HIPC(hipSetDevice(h->device));
            return set_window(h, (uint32_t)(value & 0xFFFF), (uint32_t)((value >> 16) & 0xFFFF));
        case KQ_OPT_SHARD_WINDOW:
            HIPC(hipSetDevice(h->device));
            return set_window(h, (uint32_t)(value & 0xFFFF), (uint32_t)((value >> 16) & 0xFFFF), true);
        case KQ_OPT_SLICE_KMERS:
            if (value < 1) return fail(KQ_ERR_INVALID, "KQ_OPT_SLICE_KMERS must be positive");
            h->slice_kmers = (uint64_t)value; h->slice_user = true; return KQ_OK;
        case KQ_OPT_SUBGRAPH_BATCH:
            if (value < 0) return fail(KQ_ERR_INVALID, "KQ_OPT_SUBGRAPH_BATCH must be 0 (automatic) or a number of searches");
            h->sg_batch = (uint64_t)value; return KQ_OK;
        case KQ_OPT_VARIANT_BATCH:
            if (value < 0) return fail(KQ_ERR_INVALID, "KQ_OPT_VARIANT_BATCH must be 0 (automatic) or a number of searches");
            h->var_batch = (uint64_t)value; return KQ_OK;
        default: return fail(KQ_ERR_INVALID, "unknown option %d", option);
    }
}
int kq_get_profile(kq_handle* h, char* buf, uint64_t cap) {
    if (!h || !buf || !cap) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    HIPC(hipStreamSynchronize(h->stream));
    std::string out;
    for (size_t i = 1; i < h->marks.size(); ++i) {
        float ms = 0;
        HIPC(hipEventElapsedTime(&ms, h->marks[i - 1].second.get(), h->marks[i].second.get()));
        char tmp[96];
        snprintf(tmp, sizeof tmp, "%s%s=%.4f", out.empty() ? "" : ";", h->marks[i].first, ms);
        out += tmp;
    }
    if (out.size() + 1 > cap) return fail(KQ_ERR_CAPACITY, "profile buffer too small: need %zu", out.size() + 1);
    memcpy(buf, out.c_str(), out.size() + 1);
    return KQ_OK;
}
void* kq_get_stream(kq_handle* h) { return h ? (void*)h->stream : nullptr; }
int kq_sync(kq_handle* h) {
    if (!h) return fail(KQ_ERR_INVALID, "null handle");
    HIPC(hipSetDevice(h->device));
    HIPC(hipStreamSynchronize(h->stream));
    const int rc = check_errors(h);
    if (h->bz_bad) return fail(KQ_ERR_INVALID, "%s: submitted for counting and skipped (kq_clear resets this)", h->bz_err.c_str());
    if (h->fx_bad) return fail(KQ_ERR_INVALID, "malformed %s text was submitted for counting and skipped (kq_clear resets this)", h->fx_bad == KQ_FASTX_FASTQ ? "FASTQ" : "FASTA");
    return rc;
}
int kq_flush(kq_handle* h) {
    if (!h) return fail(KQ_ERR_INVALID, "null handle");
    HIPC(hipSetDevice(h->device));
    return flush_pending(h);
}
int kq_get_info(kq_handle* h, kq_info* out) {
    if (!h || !out) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    int rc = read_state(h);
    if (rc) return rc;
    out->kmers_counted = h->host_state()->kmers_added;
    out->slots_used = h->host_state()->slots_used;
    out->slots_total = h->n_slots();
    out->hc_used = h->host_state()->hc_used;
    out->hc_total = h->hc_cap;
    out->table_bytes = h->n_slots() * sizeof(Slot) + h->hc_cap * sizeof(HcSlot);
    out->table_passes = h->table_passes;
    return KQ_OK;
}

// ---- count ---------------------------------------------------------------------------------
// ---- partitioned count: host orchestration -------------------------------------------------------
struct PartPlan : PlanSizes {   // the plan's numbers (kq_plan_host.h) ...
    bool even_buckets = false;   // the slice's bucket offsets were read back and passed kq::seg_gate_even (count_partitioned)
    // ... and its device pointers into h->work
    uint64_t *recs1, *recs2;
    uint8_t *aux1, *aux2;     // WIDE records: edge bytes travelling with recs1 / recs2
    unsigned long long *m1, *seg_off, *unit_base, *group_base, *sums, *total, *hot;
    uint32_t* m2;
    // the lockstep bytes of recs1 / recs2; null for the formats that have none
    uint8_t* a1() const { return fmt == FMT_WIDE || fmt == FMT_NARROW ? aux1 : nullptr; }
    uint8_t* a2() const { return fmt == FMT_WIDE || fmt == FMT_NARROW ? aux2 : nullptr; }
};
// carve the scratch buffer for a batch of at most n_max records (plan_sizes / plan_layout: kq_plan_host.h); n_tiles = 0 when
// the input is records
static int plan_alloc(kq_handle* h, PartPlan* p, uint64_t n_max, uint64_t n_tiles, uint32_t p1_bins, bool allow_narrow = false,
                      uint64_t min_segs = 0 /*segments / output groups an exchange level needs beyond the table's own*/) {
    if (h->test_fail_plan) { h->test_fail_plan = false; return fail(KQ_ERR_NOMEM, "partition scratch allocation failed (injected by KQ_OPT_TEST_FAIL_PLAN)"); }
    if (n_max >= (1ull << 32) - 16) return fail(KQ_ERR_INVALID, "a partition pass handles fewer than 2^32 records (got %llu): slice the input", (unsigned long long)n_max);
    static_cast<PlanSizes&>(*p) = plan_sizes(h->shape(), h->n_cu, n_max, n_tiles, p1_bins, allow_narrow, min_segs);
    const PlanLayout at = plan_layout(*p);
    // the second record array of a large plan lives in a physically scrambled buffer of its own (struct Scrambled)
    if (p->split2) { int rc2 = scr_ensure(h->work.part2, at.part2_bytes, h->device); if (rc2) return rc2; }
    HIPC(h->work.part.ensure((size_t)at.words * 8));
    uint64_t* const base = h->work.part.as<uint64_t>();
    uint64_t* const base2 = p->split2 ? (uint64_t*)h->work.part2.p : base;
    p->recs1 = base + at.recs1; p->aux1 = (uint8_t*)(base + at.aux1);
    p->recs2 = base2 + at.recs2; p->aux2 = (uint8_t*)(base2 + at.aux2);
    p->m1 = (unsigned long long*)(base + at.m1);
    p->seg_off = (unsigned long long*)(base + at.seg_off);
    p->unit_base = (unsigned long long*)(base + at.unit_base);
    p->group_base = (unsigned long long*)(base + at.group_base);
    p->sums = (unsigned long long*)(base + at.sums);
    p->total = (unsigned long long*)(base + at.total);
    p->hot = (unsigned long long*)(base + at.hot);
    p->m2 = (uint32_t*)(base + at.m2);
    return KQ_OK;
}
// exclusive scan of n u64 on the device (in place); *total (device) receives the sum
static void scan_u64(kq_handle* h, unsigned long long* a, uint64_t n, unsigned long long* sums_scratch, unsigned long long* total) {
    if (n <= 2 * SCAN_CHUNK) {                     // one workgroup: up to 32 elements per thread
        hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(1024), 0, h->stream, a, n, total);
        return;
    }
    const uint64_t chunks = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
    hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)chunks), dim3(1024), 0, h->stream, a, n, sums_scratch);
    hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(1024), 0, h->stream, sums_scratch, chunks, total);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)chunks), dim3(1024), 0, h->stream, a, n, sums_scratch);
}
// P1 on bases with the given bin function; afterwards p->seg_off[0..bins] are the bucket offsets
// (seg_off[bins] = number of records) and `out` holds the records grouped by bin
// stage marker of the last partitioned count (KQ_OPT_PROFILE): one HIP event per call, on the handle's stream
static void mark(kq_handle* h, const char* name) {
    if (!h->profile) return;
    Event e;
    if (e.create(hipEventDefault) != hipSuccess) return;
    (void)hipEventRecord(e.get(), h->stream);
    h->marks.emplace_back(name, std::move(e));
}
static void marks_reset(kq_handle* h) { h->marks.clear(); }

// the scanned sequence of a P1 pass; pinv != nullptr: packed input, ab = the code words (tile_fetch)
struct P1Scan { const uint8_t* ab; uint64_t lead, len; EmitRange er; const uint16_t* pinv; };
static int launch_p1_hist(kq_handle* h, const KernelSel& s, uint32_t grid, const P1Scan& in, const PartCfg& cfg, uint32_t g1, unsigned long long* m1) {
    static const KernelRow<decltype(&k_p1_hist<0, 0>)> rows[] = {p1h<6, 21>(), p1h<6, 31>(), p1h<6, 0>(), p1h<2, 21>(), p1h<2, 0>(), p1h<1, 31>(), p1h<1, 0>(),
                                                                  p1h<3, 21>(), p1h<3, 0>(), p1h<4, 21>(), p1h<4, 0>(), p1h<0, 0>(), p1h<5, 21>(), p1h<5, 0>()};
    return launch_row(rows, "k_p1_hist", s, h, dim3(grid), dim3(TILE_THREADS), in.ab, in.lead, in.len, h->k, cfg, in.er, g1, m1, in.pinv);
}
static int launch_p1_scatter(kq_handle* h, const KernelSel& s, uint32_t grid, const P1Scan& in, const PartCfg& cfg, const unsigned long long* m1, uint64_t* out, uint8_t* out_aux, int aux_fmt) {
    static const KernelRow<decltype(&k_p1_scatter<0, 512, 0, 0>)> wide[] = {
        p1w<FMT_TOP8, 512, 6, 31>(), p1w<FMT_TOP8, 512, 6, 0>(), p1w<FMT_TOP8, 512, 2, 31>(), p1w<FMT_TOP8, 512, 2, 0>(), p1w<FMT_TOP8, 512, 0, 0>(),
        p1w<FMT_NARROW, 512, 4, 21>(), p1w<FMT_NARROW, 512, 4, 0>(), p1w<FMT_NARROW, 512, 6, 21>(), p1w<FMT_NARROW, 512, 6, 0>(), p1w<FMT_NARROW, 512, 2, 21>(), p1w<FMT_NARROW, 512, 2, 0>(), p1w<FMT_NARROW, 512, 0, 0>(),
        p1w<FMT_WIDE, 512, 1, 31>(), p1w<FMT_WIDE, NB_MAX, 1, 31>(), p1w<FMT_WIDE, 512, 0, 0>(), p1w<FMT_WIDE, NB_MAX, 0, 0>(),
        p1w<FMT_PACK8, 512, 3, 21>(), p1w<FMT_PACK8, 512, 3, 0>(), p1w<FMT_PACK8, 512, 1, 0>(), p1w<FMT_PACK8, NB_MAX, 1, 0>(), p1w<FMT_PACK8, 512, 0, 0>(), p1w<FMT_PACK8, NB_MAX, 0, 0>()};
    // the streamed scatter of 5-byte records (TPR tiles per round) and of hash-remainder records (TOP8)
    static const KernelRow<decltype(&k_p1_scatter_s<0, 0, 1>)> streamed[] = {
        p1s<4, 21, 1>(), p1s<4, 0, 1>(), p1s<6, 21, 1>(), p1s<6, 0, 1>(), p1s<2, 21, KQ_P1S_TPR>(), p1s<2, 0, KQ_P1S_TPR>(), p1s<0, 0, 1>(),
        p1s<6, 31, 1, true>(), p1s<6, 0, 1, true>(), p1s<2, 31, 1, true>(), p1s<2, 0, 1, true>(), p1s<0, 0, 1, true>()};
    static const KernelRow<decltype(&k_p1_scatter_c<0>)> compact[] = {p1c<21>(), p1c<0>()};
    if (s.fam == K_P1_SCATTER_S) return launch_row(streamed, "k_p1_scatter_s", s, h, dim3(grid), dim3(TILE_THREADS * s.tpr), in.ab, in.lead, in.len, h->k, cfg, in.er, m1, (uint32_t*)out, out_aux, in.pinv);
    if (s.fam == K_P1_SCATTER_C) return launch_row(compact, "k_p1_scatter_c", s, h, dim3(grid), dim3(TILE_THREADS), in.ab, in.lead, in.len, h->k, cfg, in.er, m1, (uint32_t*)out, out_aux, in.pinv);
    return launch_row(wide, "k_p1_scatter", s, h, dim3(grid), dim3(TILE_THREADS), in.ab, in.lead, in.len, h->k, cfg, in.er, m1, out, out_aux, aux_fmt, in.pinv);
}

static int run_p1(kq_handle* h, PartPlan* p, const PartCfg& cfg, const uint8_t* ab, uint64_t lead, uint64_t len, EmitRange er, uint64_t* out,
                  uint8_t* out_aux, int aux_fmt, const uint16_t* pinv = nullptr /*packed input: ab = the code words (tile_fetch)*/) {
    const P1Scan in{ab, lead, len, er, pinv};
    const bool full_range = cfg.filt_lo == 0 && cfg.filt_hi == cfg.map_count, windowed = cfg.win_lo != 0 || cfg.win_hi != (1u << NARROW_CBITS);
    const KernelSel hist = select_p1_hist(h->k, cfg.mode, cfg.narrow, cfg.map_mask, full_range, windowed);
    const bool narrow_filt = hist.bin == 4, narrow_win = hist.bin == 6;      // map-range pass on a bucketed table; windowed table
    // KQ_OPT_COUNT_MAP_PASSES = n: this map-range pass is one of n over RESIDENT batches (the caller vouches that a batch keeps
    // its address and content between the passes).  The first pass that scans a slice counts for all n ranges in one histogram
    // launch (bin = range * 256 + bucket: the block of a range is contiguous in the bin-major matrix) and keeps the raw counts;
    // every pass takes its block from there -- (n - 1) of the n histogram scans of a slice are never run.
    // the cached count matrix of `key`, or a fresh one of `bytes` bytes that a histogram over `all` fills; null: no room (4 GiB
    // cap, hipMalloc) or, with rc set, no such kernel
    int rc = KQ_OK;
    auto cached_hist = [&](const kq_handle::HistKey& key, size_t bytes, const PartCfg& all) -> kq_handle::HistEntry* {
        for (auto& e : h->hist_cache) if (e.key == key) return &e;
        if (h->hist_cache_bytes + bytes > ((size_t)4 << 30)) return nullptr;
        DevMem buf;
        if (buf.alloc(bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        rc = launch_p1_hist(h, select_p1_hist_cached(h->k, hist.bin), p->g1, in, all, p->g1, buf.as<unsigned long long>());
        if (rc) return nullptr;
        h->hist_cache.push_back(kq_handle::HistEntry{key, std::move(buf)});
        h->hist_cache_bytes += bytes;
        return &h->hist_cache.back();
    };
    bool have_hist = false;
    const size_t row = (size_t)p->g1 * sizeof(unsigned long long), block = row << NARROW_CBITS;       // one bucket's counts; the matrix of one range
    if (narrow_filt && h->map_passes > 1 && P1_F == 1 && !h->hist_cache_off) {
        const uint32_t n = (uint32_t)h->map_passes, per = cfg.map_count / n, rr = cfg.filt_lo / per;
        if (cfg.filt_lo == rr * per && cfg.filt_hi == (rr + 1) * per) {
            PartCfg all = cfg;
            all.n_rng = n; all.n_coarse = n << NARROW_CBITS;
            if (const auto* ent = cached_hist({ab, pinv, lead, len, er.lo, er.hi, p->g1, n, h->k}, n * block, all)) {
                (void)hipMemcpyAsync(p->m1, ent->m1_all.as<char>() + rr * block, block, hipMemcpyDeviceToDevice, h->stream);
                have_hist = true;
            }
        }
    }
    // the same for bucket-range passes (windowed table): the unfiltered bucket matrix (any k: hash-remainder records too) serves
    // every window -- the rows of the other buckets are zeroed before the scan
    if (narrow_win && h->map_passes > 1 && P1_F == 1 && !h->hist_cache_off) {
        PartCfg all = cfg;
        all.win_lo = 0; all.win_hi = 1u << NARROW_CBITS;
        if (const auto* ent = cached_hist({ab, pinv, lead, len, er.lo, er.hi, p->g1, 0xB0C4E7u, h->k}, block, all)) {
            (void)hipMemcpyAsync(p->m1, ent->m1_all.get(), block, hipMemcpyDeviceToDevice, h->stream);
            if (cfg.win_lo) (void)hipMemsetAsync(p->m1, 0, (size_t)cfg.win_lo * row, h->stream);
            if (cfg.win_hi < (1u << NARROW_CBITS)) (void)hipMemsetAsync((char*)p->m1 + (size_t)cfg.win_hi * row, 0, (size_t)((1u << NARROW_CBITS) - cfg.win_hi) * row, h->stream);
            have_hist = true;
        }
    }
    if (!rc && !have_hist) rc = launch_p1_hist(h, hist, p->g1 * P1_F, in, cfg, p->g1, p->m1);
    if (rc) return rc;
    scan_u64(h, p->m1, (uint64_t)cfg.n_coarse * p->g1 * P1_F, p->sums, p->total);
    hipLaunchKernelGGL(k_p1_offsets, dim3((cfg.n_coarse + 256) / 256), dim3(256), 0, h->stream, p->m1, p->total, cfg, p->g1, p->seg_off);
    mark(h, "k_p1_hist+scan");
    rc = launch_p1_scatter(h, select_p1_scatter(h->k, cfg.mode, cfg.narrow, cfg.map_mask, full_range, windowed, out_aux != nullptr, cfg.n_coarse, KQ_P1S_TPR, h->kernel_set), p->g1, in, cfg, p->m1, out, out_aux, aux_fmt);
    mark(h, "k_p1_scatter");
    return rc;
}
// The input of a split level: records (+ lockstep bytes) grouped in segments [seg_lo[i], seg_hi[i]).  n_seg / spb (segments per
// hash-prefix bucket) matter to sort_to_regions only, whose first level may read runs that are not the plan's own
struct LevelIn { const uint64_t* recs; const uint8_t* aux; const unsigned long long *seg_lo, *seg_hi; uint32_t n_seg, spb; };
// records grouped by the plan's own segment table p.seg_off[0..n_seg]: every segment ends where the next one starts
static LevelIn own_segments(const PartPlan& p, const uint64_t* recs, const uint8_t* aux, uint32_t n_seg) { return LevelIn{recs, aux, p.seg_off, p.seg_off + 1, n_seg, 1}; }
// what the unit kernels of a level read: the input records and segments, the level and the unit table
struct LevelUnits { const uint64_t* in; const uint8_t* in_aux; LevelCfg lv; const unsigned long long *seg_lo, *seg_hi, *unit_base; uint32_t* m2; unsigned grid; };
static int launch_level_hist(kq_handle* h, const KernelSel& s, const LevelUnits& u) {
    static const KernelRow<decltype(&k_lv_hist<0>)> rows[] = {lvh<FMT_TOP8>(), lvh<FMT_NARROW>(), lvh<FMT_WIDE>(), lvh<FMT_PACK8>()};
    return launch_row(rows, "k_lv_hist", s, h, dim3(u.grid), dim3(MS_THREADS), u.in, u.in_aux, u.lv, u.seg_lo, u.seg_hi, u.unit_base, u.m2);
}
static int launch_level_scatter(kq_handle* h, const KernelSel& s, const LevelUnits& u, const unsigned long long* gb, uint64_t* out, uint8_t* out_aux) {
    static const KernelRow<decltype(&k_lv_scatter<0, 512>)> rows[] = {
        lvw<FMT_PACK8_TO_NARROW, 512>(), lvw<FMT_TOP8, 512>(), lvw<FMT_TOP8, NB_MAX>(), lvw<FMT_NARROW_TO_TIGHT, 512>(), lvw<FMT_NARROW_TO_TIGHT, NB_MAX>(),
        lvw<FMT_NARROW, 512>(), lvw<FMT_NARROW, NB_MAX>(), lvw<FMT_WIDE, 512>(), lvw<FMT_WIDE, NB_MAX>(), lvw<FMT_PACK8, 512>(), lvw<FMT_PACK8, NB_MAX>()};
    static const KernelRow<decltype(&k_lv_scatter_s<false>)> streamed[] = {lvs<true>(), lvs<false>()};
    if (s.fam == K_LV_SCATTER_S) return launch_row(streamed, "k_lv_scatter_s", s, h, dim3(u.grid), dim3(LV_THREADS), (const uint32_t*)u.in, u.in_aux, u.lv, u.seg_lo, u.seg_hi, u.unit_base, u.m2, gb, (uint32_t*)out, out_aux);
    return launch_row(rows, "k_lv_scatter", s, h, dim3(u.grid), dim3(LV_THREADS), u.in, u.in_aux, u.lv, u.seg_lo, u.seg_hi, u.unit_base, u.m2, gb, out, out_aux);
}
// one generic split level: src -> out grouped by (segment, bin); afterwards gb[0..n_seg*nb] are the output offsets
static int run_level(kq_handle* h, PartPlan* p, const LevelCfg& lv, const LevelIn& src, uint64_t* out, uint8_t* out_aux,
                     unsigned long long* gb = nullptr /*where the output offsets go (default p->group_base)*/) {
    if (!gb) gb = p->group_base;
    const LevelCfg lv_ = with_rep_shift(lv);
    const uint64_t groups = (uint64_t)(lv.n_seg / lv.spb) * lv.nb;
    hipLaunchKernelGGL(k_lv_units, dim3(1), dim3(1024), 0, h->stream, src.seg_lo, src.seg_hi, lv_, p->unit_base);
    // one workgroup per work unit (upper bound of the unit count; surplus workgroups exit at once):
    // the hardware dispatcher balances them, a fixed grid looping over units left a 30 % tail
    const LevelUnits u{src.recs, src.aux, lv_, src.seg_lo, src.seg_hi, p->unit_base, p->m2, (unsigned)std::min<uint64_t>(p->n_max / P2_UNIT + lv.n_seg + 1, 1u << 30)};
    int rc = launch_level_hist(h, select_level_hist(lv.narrow, src.aux != nullptr), u);
    if (rc) return rc;
    // few units per segment (many segments): one thread per group; else one wave per group (a segment of thousands of units)
    if (p->n_max / P2_UNIT + 1 <= 8 * (uint64_t)(lv.n_seg / lv.spb))
        hipLaunchKernelGGL(k_lv_offsets_thread, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, h->stream, p->m2, lv_, p->unit_base, gb);
    else
        hipLaunchKernelGGL(k_lv_offsets, dim3((unsigned)((groups * 64 + 255) / 256)), dim3(256), 0, h->stream, p->m2, lv_, p->unit_base, gb);
    (void)hipMemsetAsync(gb + groups, 0, 8, h->stream);   // failure surfaces at the caller's hipGetLastError
    scan_u64(h, gb, groups + 1, p->sums, p->total + 1);
    mark(h, "k_lv_hist+offsets+scan");
    rc = launch_level_scatter(h, select_level_scatter(lv.narrow, src.aux != nullptr, lv.top8 != 0, lv.nb, lv.rstart != nullptr, h->kernel_set), u, gb, out, out_aux);
    mark(h, "k_lv_scatter");
    return rc;
}
// The last level of a plan with a middle level, narrow records in and tight records out, fewer than 512 regions per segment: one
// workgroup per segment counts, offsets and splits it (k_lv_segment_s).  Same output and same gb as run_level.
static void run_segment_level(kq_handle* h, PartPlan* p, const LevelCfg& lv, const uint64_t* in, const uint8_t* in_aux, uint64_t* out, unsigned long long* gb) {
    mark(h, "segment_level");                                     // (zero-length: tells a reader of the stage list which form ran)
    mark(h, "k_lv_hist+offsets+scan");                            // (no such stage here: the name stays so that stage_ms adds up)
    hipLaunchKernelGGL(k_lv_segment_s, dim3(lv.n_seg), dim3(LV_THREADS), 0, h->stream, (const uint32_t*)in, in_aux, with_rep_shift(lv), p->seg_off, gb, (uint32_t*)out);
    mark(h, "k_lv_scatter");
}
// ---- pending sets ---------------------------------------------------------------------------------
// A k_count_regions pass streams every region image of the table in and out once, whatever the number of records it
// applies.  So the region-sorted record set that P1 + the split levels make of a slice is not applied at once: it is
// kept in an arena (5 bytes per record for the default k) and one pass takes all pending sets together -- when the
// arena is full, before the table geometry changes, and before anything reads the table or the device state
// (kq_sync, summary, lookup, export, merge ...).  Counting is commutative, so results do not depend on when a set is
// applied.  This is what lets a human-scale table (tens of GB) be streamed once per ~10^10 records instead of once
// per slice; KQ_OPT_PENDING_BYTES bounds the arena (0 = apply every slice at once, the round-1 behaviour).
__global__ void k_p3set(P3Set* sets, int i, P3Set v) { sets[i] = v; }

// Where the last split level writes records, lockstep bytes and region offsets: a pending set in the arena (recs != nullptr) or
// the plan's scratch, whose set is applied at once (the scratch is reused by the next slice).  fmt / aux_fmt: of the finished
// set; `tight`: the last level writes FMT_TIGHT records (count path only: the lookup kernels read 5-byte records)
struct Dest {
    int fmt, aux_fmt;
    bool tight = false;
    uint64_t* recs = nullptr; uint8_t* aux = nullptr; unsigned long long* base = nullptr; uint64_t n_max = 0;      // the arena set
    bool in_arena() const { return recs != nullptr; }
};
// room for one more set of format d->fmt in the arena (flushes / allocates as needed); d stays in the scratch: no deferral for this slice
static int arena_take(kq_handle* h, uint64_t n_max, uint64_t R, Dest* d) {
    if (h->pend_budget == 0) return KQ_OK;
    const int fmt = d->fmt;
    const SetLayout lay = set_bytes(n_max, fmt, R);
    const size_t need = lay.total;
    bool was_full = false;
    if (h->n_pend && (h->n_pend >= P3_MAX_SETS || h->pend_fmt != fmt || h->arena_used + need > h->arena_bytes)) {
        was_full = h->pend_fmt == fmt && h->n_pend < P3_MAX_SETS;
        int rc = flush_pending(h);
        if (rc) return rc;
    }
    // the arena grows as arena_want / arena_budget say (kq_plan_host.h)
    const size_t want = arena_want(need, h->arena_bytes, was_full, h->pend_budget);
    if (want > h->arena_bytes) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return KQ_OK;
        const size_t budget = arena_budget(want, need, h->arena_bytes, h->pend_budget, free_b, total_b, (size_t)h->table_bytes());
        if (budget == ARENA_STAY) return KQ_OK;
        if (budget) {
            if (h->arena.p) { HIPC(hipStreamSynchronize(h->stream)); HIPC(hipStreamSynchronize(h->base)); h->arena.reset(); h->arena_bytes = 0; }
            static const bool scramble_arena = !getenv("KQ_SCRAMBLE_ARENA") || atoi(getenv("KQ_SCRAMBLE_ARENA")) != 0;      // (0: plain hipMalloc, for A/B)
            if (!h->arena.alloc(budget, h->device, scramble_arena && budget >= ((size_t)1 << 30))) return KQ_OK;      // no memory is no error: the slice stays in the scratch
            h->arena_bytes = budget; h->arena_used = 0;
        }
    }
    uint8_t* set = (uint8_t*)h->arena.p + h->arena_used;
    d->recs = (uint64_t*)set;
    d->aux = lay.has_aux ? set + lay.aux_off : nullptr;
    d->base = (unsigned long long*)(set + lay.base_off);
    d->n_max = n_max;
    h->arena_used += need;
    return KQ_OK;
}
// make `set` (records of format fmt, sorted by region of the CURRENT geometry) part of the next table pass
static int pend_add(kq_handle* h, const P3Set& set, int fmt, int aux_fmt) {
    if (h->n_pend && (h->n_pend >= P3_MAX_SETS || h->pend_fmt != fmt || h->pend_aux_fmt != aux_fmt)) {
        int rc = flush_pending(h);
        if (rc) return rc;
    }
    if (!h->d_sets) HIPC(h->d_sets.alloc(sizeof(P3Set) * P3_MAX_SETS));
    hipLaunchKernelGGL(k_p3set, dim3(1), dim3(1), 0, h->stream, h->d_sets.as<P3Set>(), h->n_pend, set);
    h->pend_sets[h->n_pend] = set;
    h->pend_fmt = fmt; h->pend_aux_fmt = aux_fmt;
    ++h->n_pend;
    h->pend_records += set.n_max;
    return KQ_OK;
}
// P3 over all pending sets.  Always on the handle's own stream (`base`), behind a join with the fork streams that wrote the
// sets; the fork streams in turn wait for the pass before they go on (their next sets reuse the arena it reads).
static int flush_pending_base(kq_handle* h);
static int flush_pending(kq_handle* h) {
    if (!h->n_pend) return KQ_OK;
    hipStream_t work = h->stream;
    h->stream = h->base;
    int rc = join_forks(h);
    if (!rc) rc = flush_pending_base(h);
    if (!rc && h->fork_stream[0]) {
        hipEvent_t e; rc = ev_get(h, &e);
        if (!rc && hipEventRecord(e, h->base) != hipSuccess) rc = fail(KQ_ERR_HIP, "hipEventRecord failed");
        for (int w = 0; w < 2 && !rc; ++w) if (hipStreamWaitEvent(h->fork_stream[w].get(), e, 0) != hipSuccess) rc = fail(KQ_ERR_HIP, "hipStreamWaitEvent failed");
    }
    h->stream = work;
    return rc;
}
static_assert(ROFF_MAX_SETS == (uint32_t)P3_MAX_SETS, "the offset matrix has a column for every set of a pass");
// The region-major offset matrix (geometry: kq_roff_host.h) for this pass, or nullptr: the pass then reads the sets' own offset
// arrays, as it always could.  The buffer is taken at the first pass from what the arena's sizing leaves free, and again only
// when the table has grown; a failed allocation is not an error.
static uint32_t* roff_take(kq_handle* h) {
    for (int i = 0; i < h->n_pend; ++i) if (h->pend_sets[i].n_max >> 32) return nullptr;      // offsets are stored in 32 bits
    const size_t need = roff_bytes(h->n_alloc_regions());
    if (!need || !roff_pitch((uint32_t)h->n_pend)) return nullptr;
    if (h->roff.bytes() < need && h->roff.alloc(need) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return h->roff.as<uint32_t>();
}
// one kernel of the table pass over the pending sets; `rows`: the region-major offset matrix (k_count_regions_q4r only)
static int launch_table_pass(kq_handle* h, const KernelSel& s, dim3 grid, const Q4SetsRow& rows, int empty, unsigned long long* hot, uint32_t rps) {
    static const KernelRow<decltype(&k_count_regions<0, false>)> generic[] = {p3g<FMT_TOP8, false>(), p3g<FMT_WIDE, false>(), p3g<FMT_PACK8, false>(), p3g<FMT_NARROW, true>(), p3g<FMT_TOP8, true>(), p3g<FMT_WIDE, true>(), p3g<FMT_PACK8, true>()};
    static const KernelRow<decltype(&k_count_regions_q4<0, false>)> compact[] = {p3q<21, true>(), p3q<0, true>(), p3q<21, false>(), p3q<0, false>()};
    static const KernelRow<decltype(&k_count_regions_q4r<0, false>)> matrix[] = {p3r<21, true>(), p3r<0, true>(), p3r<21, false>(), p3r<0, false>()};
    const P3Set* sets = h->d_sets.as<P3Set>();
    if (s.fam == K_COUNT_REGIONS_Q4R) return launch_row(matrix, "k_count_regions_q4r", s, h, grid, dim3(Q4_THREADS), h->view(), rows, empty, hot, rps);
    if (s.fam == K_COUNT_REGIONS_Q4) return launch_row(compact, "k_count_regions_q4", s, h, grid, dim3(Q4_THREADS), h->view(), sets, (uint32_t)h->n_pend, empty, hot, rps);
    return launch_row(generic, "k_count_regions", s, h, grid, dim3(P3_THREADS), h->view(), sets, (uint32_t)h->n_pend, h->pend_aux_fmt, empty, hot, rps);
}
static int flush_pending_base(kq_handle* h) {
    const uint64_t R = h->n_regions;
    HIPC(h->hot.ensure((size_t)(R + 2) * 8));
    int rc;
    if (hc_follows_fill(h->kmers_bound)) {       // large jobs: the side table follows its observed fill (see reserve)
        rc = read_state_raw(h); if (rc) return rc;
        const uint64_t need_hc = hc_need(h->kmers_bound, h->host_state()->hc_used);
        if (need_hc > h->hc_cap) { rc = grow_hc(h, need_hc); if (rc) return rc; }
    }
    unsigned long long* hot = h->hot.as<unsigned long long>();     // [0] = count, then up to R region ids
    HIPC(hipMemsetAsync(hot, 0, 8, h->stream));
    const dim3 grid((unsigned)std::min<uint64_t>(h->n_alloc_regions(), 1u << 30)), grid_hot(h->n_cu);   // one workgroup per (allocated) region: dispatcher-balanced
    // 1: the slot array holds the empty image (skip reading it); 2: logically empty but not initialised (lazy kq_clear):
    // also write the image of regions without records.  A dirty array is never read, whatever table_empty says
    const int empty = h->slots_dirty ? 2 : h->table_empty ? 1 : 0;
    const int fmt = h->pend_fmt;
    const uint32_t rps = (fmt == FMT_NARROW || fmt == FMT_TIGHT || fmt == FMT_TOP8) ? (uint32_t)(R >> NARROW_CBITS) : 1u;
    // 4- and 5-byte records: the sets' region offsets are transposed first, the pass reads one row pair per region and adds the
    // regions' totals to TOT_LINES lines, which k_fold_totals adds to the table state behind it (KQ_OPT_KERNEL_SET bit 16, or no
    // memory for the matrix: the previous pass -- the sets' own offset arrays, two atomics per region on the table state)
    Q4SetsRow rows = {};
    if (table_pass_wants_matrix(fmt, h->kernel_set)) {
        if (uint32_t* roff = roff_take(h)) {
            rows.pitch = roff_pitch((uint32_t)h->n_pend);
            if (!h->tot) {
                const size_t tb = (size_t)TOT_LINES * 64;
                if (h->tot.alloc(tb) != hipSuccess) (void)hipGetLastError();
                else HIPC(hipMemsetAsync(h->tot.get(), 0, tb, h->stream));
            }
            rows.tot = h->tot.as<unsigned long long>();
            rows.roff = roff - h->reg_lo() * rows.pitch;                 // row r of the geometry (a window allocates its own rows only)
            for (int i = 0; i < h->n_pend; ++i) { rows.d[i].recs = (const uint32_t*)h->pend_sets[i].recs; rows.d[i].aux = h->pend_sets[i].aux; }
            const uint64_t n_rows = roff_rows(h->n_alloc_regions());
            hipLaunchKernelGGL(k_p3_region_offsets, dim3(grid_for(h, n_rows, ROFF_ROWS, 32)), dim3(ROFF_THREADS), 0, h->stream,
                               roff, h->d_sets.as<P3Set>(), (uint32_t)h->n_pend, rows.pitch, h->reg_lo(), n_rows);
        }
    }
    // ordinary regions, then the skewed ones the pass listed
    rc = launch_table_pass(h, select_table_pass(fmt, h->k, rows.roff != nullptr), grid, rows, empty, hot, rps);
    if (!rc) rc = launch_table_pass(h, select_hot_pass(fmt), grid_hot, rows, empty, hot, rps);
    if (rc) return rc;
    if (rows.roff && rows.tot) hipLaunchKernelGGL(k_fold_totals, dim3(1), dim3(256), 0, h->stream, rows.tot, h->d_state());
    h->n_pend = 0; h->arena_used = 0; h->pend_records = 0;
    ++h->table_passes;
    // only now (every failure path of the partition stages lies before this point): the table has content, and a lazily
    // cleared slot array has been written in full
    h->slots_dirty = false;
    h->table_empty = false;
    mark(h, "k_count_regions");
    HIPC(hipGetLastError());
    return KQ_OK;
}

// the destination of the set the plan's levels make of at most n_max records: in the arena if it has (or gets) room, else the
// scratch.  (A map-range pass calls this after P1, with the record count P1 found: see count_partitioned)
static int dest_take(kq_handle* h, const PartPlan& p, uint64_t n_max, Dest* d) {
    d->tight = tight_ok(p.fmt, p.R, (bool)h->rstart);
    if (d->tight) { d->fmt = FMT_TIGHT; d->aux_fmt = AUX_TIGHT; }
    return arena_take(h, n_max, p.R, d);
}
// Region-sorted set of records that the first split left grouped as `in`: whatever levels the plan needs, the last one
// writing to `d`.
//   5-byte / hash-remainder records (FMT_NARROW / FMT_TOP8): bucket -> regions (bucket b owns regions [b * nb, (b + 1) * nb)),
//     in one level or, for plans with sub_bits, bucket -> sub-bucket -> regions
//   packed / wide records: coarse bucket -> regions, or nothing at all when the bins were the regions themselves
static int sort_to_regions(kq_handle* h, PartPlan* p, const LevelIn& in, const Dest& d, P3Set* set) {
    const bool arena = d.in_arena();
    int rc = KQ_OK;
    uint64_t* fin = arena ? d.recs : p->recs2;
    uint8_t* fin_aux = arena ? d.aux : p->a2();
    unsigned long long* fin_base = arena ? d.base : p->group_base;
    if (p->fmt == FMT_NARROW || p->fmt == FMT_TOP8) {
        const uint32_t sb = p->cfg.sub_bits;
        const bool t8 = p->fmt == FMT_TOP8;
        // a middle level reads `in` and writes the scratch array that is not its input; the last level then takes the other one
        const bool mid_to_2 = sb != 0 && in.recs == p->recs1;
        if (!arena && mid_to_2) { fin = p->recs1; fin_aux = p->a1(); }
        if (d.tight) fin_aux = nullptr;
        LevelCfg last = level_narrow(p->cfg, sb, false, t8);
        if (d.tight) last.rstart = h->rstart.as<uint32_t>();
        if (sb == 0) {
            last.n_seg = in.n_seg; last.spb = in.spb;
            rc = run_level(h, p, last, in, fin, fin_aux, fin_base);
        } else {
            LevelCfg mid = level_narrow(p->cfg, sb, true, t8);
            mid.n_seg = in.n_seg; mid.spb = in.spb;
            uint64_t* m = mid_to_2 ? p->recs2 : p->recs1;
            uint8_t* m_aux = mid_to_2 ? p->a2() : p->a1();
            rc = run_level(h, p, mid, in, m, m_aux);
            if (rc) return rc;
            (void)hipMemcpyAsync(p->seg_off, p->group_base, (size_t)(((1u << NARROW_CBITS) << sb) + 1) * 8, hipMemcpyDeviceToDevice, h->stream);
            if (select_last_level(p->fmt, last.narrow, last.rstart != nullptr, last.nr_shift, last.nb, last.spb, p->even_buckets, h->kernel_set).fam == K_LV_SEGMENT_S)
                run_segment_level(h, p, last, m, m_aux, fin, fin_base);
            else
                rc = run_level(h, p, last, own_segments(*p, m, m_aux, last.n_seg), fin, fin_aux, fin_base);
        }
    } else if (p->two_level) {
        rc = run_level(h, p, level_coarse_to_regions(p->cfg), in, fin, fin_aux, fin_base);
    } else {
        *set = P3Set{in.recs, in.aux, in.seg_lo, p->n_max};          // bins were the regions themselves
        return KQ_OK;
    }
    *set = P3Set{fin, fin_aux, fin_base, arena ? d.n_max : p->n_max};
    return rc;
}

// make `set` part of the next table pass; a set in the scratch buffers is applied at once (the scratch is reused by the next slice)
static int submit(kq_handle* h, const P3Set& set, const Dest& d) {
    HIPC(hipGetLastError());
    int rc = pend_add(h, set, d.fmt, d.aux_fmt);
    if (rc) return rc;
    return d.in_arena() ? KQ_OK : flush_pending(h);
}
static int sort_and_submit(kq_handle* h, PartPlan* p, const LevelIn& in, const Dest& d) {
    P3Set set; int rc = sort_to_regions(h, p, in, d, &set);
    return rc ? rc : submit(h, set, d);
}

// the plan of a scanned sequence (count, region-wise lookup), in the record format sequence_fmt gives it
static int plan_sequence(kq_handle* h, PartPlan* p, uint64_t lead, uint64_t len) {
    int rc = plan_alloc(h, p, len, n_tiles_of(lead, len), plan_cfg(h->shape(), true).n_coarse, true);
    if (rc) return rc;
    p->fmt = sequence_fmt(p->fmt, h->k);
    return KQ_OK;
}

// partitioned count of one batch of bases: P1 (coarse split) -> P2 (region split) -> a pending set for P3 (LDS regions)
static int count_partitioned(kq_handle* h, const uint8_t* ab, uint64_t lead, uint64_t len, EmitRange er, const uint16_t* pinv = nullptr) {
    PartPlan p;
    int rc = plan_sequence(h, &p, lead, len);
    if (rc) return rc;
    p.cfg.filt_lo = h->filt_lo; p.cfg.filt_hi = h->filt_hi;      // KQ_OPT_COUNT_MAP_RANGE
    if (h->windowed) { p.cfg.win_lo = h->win_lo; p.cfg.win_hi = h->win_hi; }      // a window drops foreign buckets in P1
    const bool leveled = p.fmt == FMT_NARROW || p.fmt == FMT_TOP8 || p.two_level;
    Dest dst{p.fmt, AUX_IDX6};
    // A map-range pass (KQ_OPT_COUNT_MAP_RANGE: the reference's memory-bounded mode, src/kreeq.cpp:59-74) keeps a fraction of
    // the k-mers it scans: its pending set is sized by the record count P1 found, not by the starts of the slice, so that the
    // arena holds as many RECORDS per table pass as it would without the filter (one small read-back per slice)
    const bool filtered = p.cfg.filt_lo != 0 || p.cfg.filt_hi != p.cfg.map_count || h->windowed;      // (a window keeps its own buckets only)
    if (leveled && !filtered) { rc = dest_take(h, p, p.n_max, &dst); if (rc) return rc; }
    marks_reset(h);
    mark(h, "start");
    rc = run_p1(h, &p, p.cfg, ab, lead, len, er, p.recs1, p.a1(), AUX_IDX6, pinv);
    if (rc) return rc;
    if (leveled && filtered) {
        // (5-byte records with a middle level: the 257 bucket offsets come with the count, p.seg_off[256] = *p.total -- the
        // last level's kernel depends on how even the buckets are, kq_seg_gate_host.h)
        constexpr uint32_t NBK = 1u << NARROW_CBITS;
        const bool with_offsets = p.fmt == FMT_NARROW && p.cfg.sub_bits != 0 && p.cfg.n_coarse == NBK;
        unsigned long long offs[NBK + 1];
        unsigned long long n_recs = 0;
        if (with_offsets) HIPC(hipMemcpyAsync(offs, p.seg_off, sizeof offs, hipMemcpyDeviceToHost, h->stream));
        else HIPC(hipMemcpyAsync(&n_recs, p.total, sizeof n_recs, hipMemcpyDeviceToHost, h->stream));
        HIPC(hipStreamSynchronize(h->stream));
        if (with_offsets) { n_recs = offs[NBK]; p.even_buckets = kq::seg_gate_even(offs, NBK); }
        rc = dest_take(h, p, std::min<uint64_t>(p.n_max, ((uint64_t)n_recs + 15) & ~7ull), &dst); if (rc) return rc;
    }
    return sort_and_submit(h, &p, own_segments(p, p.recs1, p.a1(), p.cfg.n_coarse), dst);
}
// partitioned count of n records already on the device (multi-GPU receive side, kq_insert_records_dev).
// d_aux == nullptr: packed 8-byte records; else WIDE records with d_aux in `aux_fmt`.
// `raw`: d_recs holds raw keys (kq_insert_records); otherwise the records of kq_emit_packed_dev (table hashes)
static int count_partitioned_records(kq_handle* h, const uint64_t* d_recs, const uint8_t* d_aux, int aux_fmt, uint64_t n, bool raw) {
    PartPlan p;
    int rc = plan_alloc(h, &p, n, 0, 1, /*allow_narrow=*/!d_aux && !raw);
    if (rc) return rc;
    if (d_aux) p.fmt = FMT_WIDE;
    Dest dst{p.fmt, aux_fmt};
    LevelCfg first = level_flat_to_coarse(p.cfg);
    if (p.fmt == FMT_NARROW) {
        // packed records of kq_emit_packed_dev on a narrow-eligible table: the first level splits on the top 8 hash
        // bits and writes 5-byte records, the rest is the narrow path of count_partitioned
        rc = dest_take(h, p, p.n_max, &dst); if (rc) return rc;
        first.top8 = 1;
    } else {
        first.in_raw = raw ? 1 : 0; first.k = (uint32_t)h->k;
    }
    hipLaunchKernelGGL(k_set2, dim3(1), dim3(1), 0, h->stream, p.seg_off, 0ull, (unsigned long long)n);
    rc = run_level(h, &p, first, own_segments(p, d_recs, d_aux, 1), p.recs1, p.a1());        // group_base = coarse offsets
    if (rc) return rc;
    LevelIn coarse{p.recs1, p.a1(), p.group_base, p.group_base + 1, p.cfg.n_coarse, 1};
    if (p.two_level) {
        // the coarse offsets become the segment table of the next level
        HIPC(hipMemcpyAsync(p.seg_off, p.group_base, (size_t)(p.cfg.n_coarse + 1) * 8, hipMemcpyDeviceToDevice, h->stream));
        coarse = own_segments(p, p.recs1, p.a1(), p.cfg.n_coarse);
    }
    return sort_and_submit(h, &p, coarse, dst);
}

// count a resident sequence: ASCII bytes (d_inv == nullptr) or the packed form (d_bases = the code words, d_inv = the masks)
static int count_seq_dev(kq_handle* h, const char* d_bases, const uint16_t* d_inv, uint64_t len) {
    if (!h || (!d_bases && len)) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    if (len < (uint64_t)h->k) return KQ_OK;                                  // src/graph-builder.cpp:60
    const uint64_t kmers = len - h->k + 1;
    // slices (choose_slice, kq_plan_host.h); the device is asked for its free memory only where the choice depends on it
    size_t free_b = 0, total_b = 0;
    const bool have_mem_info = slice_reads_free(kmers, h->slice_kmers, h->slice_user, h->pend_budget, h->n_slots()) && hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    const uint64_t slice = choose_slice(kmers, h->slice_kmers, h->slice_user, h->pend_budget, h->n_slots(), free_b, h->work.part.bytes(), have_mem_info);
    // Fork / join: with two or more slices in this call, consecutive slices alternate between two internal streams (and two
    // scratch sets), both behind the caller's position on `base` (the input is ready there), and `base` is joined with them
    // before the call returns -- the caller's stream-ordered view of the handle does not change, and no fork outlives a call.
    struct ForkGuard {
        kq_handle* h; bool swapped = false;
        void leave() { if (swapped) { std::swap(h->work, h->fork_work); swapped = false; } h->stream = h->base; }
        ~ForkGuard() { leave(); (void)join_forks(h); }
    } guard{h};
    const bool forked = slices_fork(h->overlap, h->profile, h->count_path, kmers, slice, h->filt_lo == 0 && h->filt_hi == (uint32_t)h->map_count && !h->windowed);
    if (forked) {
        for (int w = 0; w < 2; ++w) if (!h->fork_stream[w]) HIPC(h->fork_stream[w].create(hipStreamNonBlocking));
        hipEvent_t e_in; int erc = ev_get(h, &e_in); if (erc) return erc;
        HIPC(hipEventRecord(e_in, h->base));
        for (int w = 0; w < 2; ++w) HIPC(hipStreamWaitEvent(h->fork_stream[w].get(), e_in, 0));
    }
    uint64_t slice_no = 0;
    for (uint64_t a = 0; a < kmers; a += slice, ++slice_no) {
        const uint64_t b = std::min(kmers, a + slice);
        int rc = reserve(h, b - a, b - a);
        if (rc) return rc;
        const SliceView v = slice_view(d_bases, d_inv, len, h->k, a, b);
        const bool table_ok = part_table_ok(h->shape(), true);
        bool part = slice_partitions(b - a, table_ok, h->table_bytes(), h->n_regions, h->pend_budget, h->pend_records, h->arena.p != nullptr, h->arena_bytes);
        if (h->count_path == 1) part = false;
        if (h->count_path == 2) {
            if (!table_ok) return fail(KQ_ERR_INVALID, "table too large for the partitioned path");
            part = true;
        }
        if (part) {
            if (forked) {
                const int w = (int)(slice_no & 1);
                if (w == 1) { std::swap(h->work, h->fork_work); guard.swapped = true; }
                h->stream = h->fork_stream[w].get();
                h->fork_busy[w] = true;
            }
            rc = count_partitioned(h, v.ab, v.lead, v.len, v.er, v.pinv);
            if (forked) h->fork_busy[slice_no & 1] = true;            // (a table pass inside joined the stream; what followed has not been joined)
            guard.leave();
            if (rc) return rc;
            continue;
        }
        if (forked) { rc = join_forks(h); if (rc) return rc; }       // the direct kernel updates the table: behind everything in flight
        PartCfg filt = plan_cfg(h->shape());
        filt.filt_lo = h->filt_lo; filt.filt_hi = h->filt_hi;
        materialize(h);
        h->table_empty = false;
        hipLaunchKernelGGL(k_count_direct, dim3(grid_for(h, n_tiles_of(v.lead, v.len), 1, 32)), dim3(TILE_THREADS), 0, h->stream,
                           h->view(), v.ab, v.lead, v.len, h->k, v.er, filt, v.pinv);
        HIPC(hipGetLastError());
    }
    return KQ_OK;
}
int kq_count_batch_dev(kq_handle* h, const char* d_bases, uint64_t len) { return count_seq_dev(h, d_bases, nullptr, len); }
int kq_count_packed_dev(kq_handle* h, const uint32_t* d_codes, const uint16_t* d_inv, uint64_t n_bases) {
    if (!d_inv && n_bases) return fail(KQ_ERR_INVALID, "null argument");
    return count_seq_dev(h, (const char*)d_codes, d_inv, n_bases);
}
// 16 bases -> one u32 of 2-bit codes (base i at bits 2i: A C G T = 0 1 2 3, case-blind) + one u16 of invalid-base bits
// (anything but ACGT/acgt, and the positions behind `len` in the last unit): the tile scanner's own LDS format
void kq_pack_bases(const char* bases, uint64_t len, uint32_t* codes, uint16_t* inv) {
    static const struct Lut { uint8_t v[256]; Lut() { for (int i = 0; i < 256; ++i) v[i] = 4; v['A'] = v['a'] = 0; v['C'] = v['c'] = 1; v['G'] = v['g'] = 2; v['T'] = v['t'] = 3; } } lut;
    const uint64_t full = len / 16;
    const uint8_t* b = (const uint8_t*)bases;
    for (uint64_t u = 0; u < full; ++u, b += 16) {
        uint32_t c = 0, m = 0;
        for (int i = 0; i < 16; ++i) { const uint32_t x = lut.v[b[i]]; c |= (x & 3u) << (2 * i); m |= (x >> 2) << i; }
        codes[u] = c; inv[u] = (uint16_t)m;
    }
    if (len % 16) {
        uint32_t c = 0, m = 0xFFFFu;
        for (uint64_t i = 0; i < len % 16; ++i) { const uint32_t x = lut.v[b[i]]; c |= (x & 3u) << (2 * i); if (!(x >> 2)) m &= ~(1u << i); }
        codes[full] = c; inv[full] = (uint16_t)m;
    }
}
int kq_count_batch(kq_handle* h, const char* bases, uint64_t len) {
    if (!h || (!bases && len)) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    void* d = nullptr;
    int rc = stage_in(h, bases, len, &d);
    if (rc) return rc;
    rc = kq_count_batch_dev(h, (const char*)d, len);
    if (rc) return rc;
    // the staging buffer is free again once the stream has drained; records may stay pending (errors of a pending
    // pass surface at the next kq_sync / read of the table)
    HIPC(hipStreamSynchronize(h->stream));
    return KQ_OK;
}

// page-locked host memory = ordinary pages registered with the runtime: measured on this box, hipHostRegister of 32 MiB
// takes 0.2-0.5 ms and the copies then run at the same 50+ GB/s as from hipHostMalloc memory, whose allocation costs
// 0.14 ms per MiB (and its release half of that again)
void* kq_host_alloc(uint64_t bytes) {
    const size_t n = ((size_t)(bytes ? bytes : 1) + 4095) & ~(size_t)4095;
    void* p = aligned_alloc(4096, n);
    if (!p) return nullptr;
    if (hipHostRegister(p, n, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); free(p); return nullptr; }
    return p;
}
void kq_host_free(void* p) { if (p) { (void)hipHostUnregister(p); free(p); } }

// A ticket and its staging slot (under h->in_m): the copy stream waits for the slot's previous reader, the slot holds `bytes`
static int ingest_begin(kq_handle* h, size_t bytes, uint64_t* ticket, int* slot, hipEvent_t* copied) {
    if (!h->copy_stream) {
        // events first, the stream last: a failure on the way leaves no stream, and the next call starts over
        for (auto& e : h->in_consumed) HIPC(e.create(hipEventDisableTiming));
        h->in_copied.resize(kq_handle::IN_TICKETS);
        for (auto& e : h->in_copied) HIPC(e.create(hipEventDisableTiming));
        HIPC(h->copy_stream.create(hipStreamNonBlocking));
    }
    const uint64_t t = h->in_next++;
    const int s = (int)(t % kq_handle::IN_SLOTS);
    *copied = h->in_copied[t % kq_handle::IN_TICKETS].get();
    *ticket = t; *slot = s;
    h->in_bad[t % kq_handle::IN_TICKETS] = 0;
    // the slot's previous reader must be done before it is overwritten (copy stream waits; the host does not)
    if (t >= (uint64_t)kq_handle::IN_SLOTS) HIPC(hipStreamWaitEvent(h->copy_stream.get(), h->in_consumed[s].get(), 0));
    if (h->in_buf[s].bytes() < bytes + 64) {
        // growing a slot: nothing may still read the old buffer
        if (h->in_buf[s]) { HIPC(hipStreamSynchronize(h->copy_stream.get())); HIPC(hipStreamSynchronize(h->stream)); }
        HIPC(h->in_buf[s].alloc(bytes + bytes / 4 + 4096));
    }
    return KQ_OK;
}
// shared by the ASCII and the packed entry point: copy (a [+ b]) into a staging slot, count behind the copy
static int ingest_async(kq_handle* h, const void* a, size_t a_bytes, const void* b, size_t b_bytes, uint64_t n_bases, uint64_t* ticket) {
    HIPC(hipSetDevice(h->device));
    // One caller at a time, copy included: concurrent copies from pageable memory on several streams were measured and are
    // 3 x SLOWER than one after the other (HIP stages them through per-stream buffers it first has to set up)
    std::lock_guard<std::mutex> lock(h->in_m);
    const size_t b_off = (a_bytes + 63) & ~(size_t)63, bytes = b_off + b_bytes;
    int s = 0; hipEvent_t copied;
    int rc = ingest_begin(h, bytes, ticket, &s, &copied);
    if (rc) return rc;
    char* d = h->in_buf[s].as<char>();
    if (a_bytes) HIPC(hipMemcpyAsync(d, a, a_bytes, hipMemcpyHostToDevice, h->copy_stream.get()));
    if (b_bytes) HIPC(hipMemcpyAsync(d + b_off, b, b_bytes, hipMemcpyHostToDevice, h->copy_stream.get()));
    HIPC(hipEventRecord(copied, h->copy_stream.get()));
    HIPC(hipStreamWaitEvent(h->stream, copied, 0));
    rc = count_seq_dev(h, d, b ? (const uint16_t*)(d + b_off) : nullptr, n_bases);
    HIPC(hipEventRecord(h->in_consumed[s].get(), h->stream));
    return rc;
}
int kq_count_batch_async(kq_handle* h, const char* bases, uint64_t len, uint64_t* ticket) {
    if (!h || !ticket || (!bases && len)) return fail(KQ_ERR_INVALID, "null argument");
    return ingest_async(h, bases, len, nullptr, 0, len, ticket);
}
int kq_count_packed_async(kq_handle* h, const uint32_t* codes, const uint16_t* inv, uint64_t n_bases, uint64_t* ticket) {
    if (!h || !ticket || ((!codes || !inv) && n_bases)) return fail(KQ_ERR_INVALID, "null argument");
    const uint64_t units = (n_bases + 15) / 16;
    if (!n_bases) return ingest_async(h, nullptr, 0, nullptr, 0, 0, ticket);
    return ingest_async(h, codes, units * 4, inv, units * 2, n_bases, ticket);
}
int kq_host_wait(kq_handle* h, uint64_t ticket) {
    if (!h) return fail(KQ_ERR_INVALID, "null handle");
    if (ticket >= h->in_next) return fail(KQ_ERR_INVALID, "unknown ticket %llu", (unsigned long long)ticket);
    if (h->in_next - ticket >= (uint64_t)kq_handle::IN_TICKETS) return KQ_OK;      // long recycled: that copy finished many batches ago
    HIPC(hipEventSynchronize(h->in_copied[ticket % kq_handle::IN_TICKETS].get()));
    if (const int bad = h->in_bad[ticket % kq_handle::IN_TICKETS])
        return fail(KQ_ERR_INVALID, "malformed %s text (ticket %llu): not counted", bad == KQ_FASTX_FASTQ ? "FASTQ" : "FASTA", (unsigned long long)ticket);
    return KQ_OK;
}

// ---- FASTQ / FASTA text and 2-bit packing on the device (kq_fastx.h) --------------------------------------------------

int kq_pack_bases_dev(kq_handle* h, const char* d_bases, uint64_t len, uint32_t* d_codes, uint16_t* d_inv) {
    if (!h || ((!d_bases || !d_codes || !d_inv) && len)) return fail(KQ_ERR_INVALID, "null argument");
    if (!len) return KQ_OK;
    HIPC(hipSetDevice(h->device));
    const uint8_t* ab; uint64_t lead;
    aligned_view(d_bases, &ab, &lead);
    hipLaunchKernelGGL(k_pack_bases, dim3(grid_for(h, (len + 15) / 16, 256, 16)), dim3(256), 0, h->stream, ab, (uint32_t)lead, len, d_codes, d_inv);
    HIPC(hipGetLastError());
    return KQ_OK;
}

static int fx_args(kq_handle* h, const char* text, uint64_t len, int format) {
    if (!h || (!text && len)) return fail(KQ_ERR_INVALID, "null argument");
    if (format != KQ_FASTX_FASTQ && format != KQ_FASTX_FASTA) return fail(KQ_ERR_INVALID, "format must be KQ_FASTX_FASTQ or KQ_FASTX_FASTA, not %d", format);
    return KQ_OK;
}
static uint64_t fx_units_of(const char* d_text, uint64_t len) { return (((uintptr_t)d_text & 15) + len + FX_UNIT - 1) / FX_UNIT; }
static int fx_prepare(kq_handle* h, uint64_t n_units) {
    if (!h->fx_res) HIPC(h->fx_res.alloc(sizeof(FxResult)));
    if (!h->fx_res_host) HIPC(h->fx_res_host.alloc(sizeof(FxResult)));
    HIPC(h->fx_units.ensure((size_t)n_units * sizeof(FxUnit)));
    return KQ_OK;
}
// summaries + scan on `st` (len > 0): the units hold every unit's output offset and incoming state, fx_res the total
static void fx_scan(kq_handle* h, hipStream_t st, const char* d_text, uint64_t len, int format) {
    const uint8_t* ab; uint64_t lead;
    aligned_view(d_text, &ab, &lead);
    const uint64_t n_units = fx_units_of(d_text, len);
    const dim3 grid((unsigned)((n_units + FX_THREADS / 64 - 1) / (FX_THREADS / 64)));
    FxUnit* units = h->fx_units.as<FxUnit>();
    if (format == KQ_FASTX_FASTQ) {
        hipLaunchKernelGGL((k_fx_summary<FX_FASTQ>), grid, dim3(FX_THREADS), 0, st, ab, lead, lead + len, n_units, units);
        hipLaunchKernelGGL((k_fx_scan<FX_FASTQ>), dim3(1), dim3(FX_SCAN_THREADS), 0, st, ab, lead, units, n_units, h->fx_res.as<FxResult>());
    } else {
        hipLaunchKernelGGL((k_fx_summary<FX_FASTA>), grid, dim3(FX_THREADS), 0, st, ab, lead, lead + len, n_units, units);
        hipLaunchKernelGGL((k_fx_scan<FX_FASTA>), dim3(1), dim3(FX_SCAN_THREADS), 0, st, ab, lead, units, n_units, h->fx_res.as<FxResult>());
    }
}
// kept bytes -> d_out (nullptr: the record checks only)
static void fx_apply(kq_handle* h, hipStream_t st, const char* d_text, uint64_t len, int format, char* d_out) {
    const uint8_t* ab; uint64_t lead;
    aligned_view(d_text, &ab, &lead);
    const uint64_t n_units = fx_units_of(d_text, len);
    const dim3 grid((unsigned)((n_units + FX_THREADS / 64 - 1) / (FX_THREADS / 64)));
    if (format == KQ_FASTX_FASTQ) hipLaunchKernelGGL((k_fx_apply<FX_FASTQ>), grid, dim3(FX_THREADS), 0, st, ab, lead, lead + len, n_units, h->fx_units.as<const FxUnit>(), (uint8_t*)d_out, h->fx_res.as<FxResult>());
    else hipLaunchKernelGGL((k_fx_apply<FX_FASTA>), grid, dim3(FX_THREADS), 0, st, ab, lead, lead + len, n_units, h->fx_units.as<const FxUnit>(), (uint8_t*)d_out, h->fx_res.as<FxResult>());
}
static int fx_read_result(kq_handle* h, hipStream_t st) {
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(h->fx_res_host.get(), h->fx_res.get(), sizeof(FxResult), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return KQ_OK;
}
static const char* fx_name(int format) { return format == KQ_FASTX_FASTQ ? "FASTQ" : "FASTA"; }
static const char* fx_rule(int format) {
    return format == KQ_FASTX_FASTQ ? "four-line records expected: every first line starts with '@', every third with '+'" : "the text must start with '>'";
}

int kq_parse_fastx_dev(kq_handle* h, const char* d_text, uint64_t len, int format, char* d_bases, uint64_t cap, uint64_t* n_bases) {
    int rc = fx_args(h, d_text, len, format);
    if (rc) return rc;
    if (!n_bases) return fail(KQ_ERR_INVALID, "null argument");
    *n_bases = 0;
    if (!len) return KQ_OK;
    HIPC(hipSetDevice(h->device));
    rc = fx_prepare(h, fx_units_of(d_text, len)); if (rc) return rc;
    fx_scan(h, h->stream, d_text, len, format);
    rc = fx_read_result(h, h->stream); if (rc) return rc;
    const uint64_t n = h->fx_host()->n_bases;
    *n_bases = n;
    const bool fits = d_bases && n <= cap;
    fx_apply(h, h->stream, d_text, len, format, fits ? d_bases : nullptr);
    rc = fx_read_result(h, h->stream); if (rc) return rc;
    if (h->fx_host()->bad) return fail(KQ_ERR_INVALID, "malformed %s text (%s)", fx_name(format), fx_rule(format));
    if (d_bases && !fits) return fail(KQ_ERR_CAPACITY, "output buffer too small: %llu bases, room for %llu", (unsigned long long)n, (unsigned long long)cap);
    return KQ_OK;
}

// counts out of a library-owned buffer: no KQ_OPT_COUNT_MAP_PASSES cache entry may be made for or taken from its address
struct HistCacheOff { kq_handle* h; explicit HistCacheOff(kq_handle* x) : h(x) { h->hist_cache_off = true; } ~HistCacheOff() { h->hist_cache_off = false; } };

int kq_count_fastx_dev(kq_handle* h, const char* d_text, uint64_t len, int format) {
    int rc = fx_args(h, d_text, len, format);
    if (rc) return rc;
    if (!len) return KQ_OK;
    HIPC(hipSetDevice(h->device));
    rc = fx_prepare(h, fx_units_of(d_text, len)); if (rc) return rc;
    if (h->fx_out.bytes() < len + 64) {
        HIPC(hipStreamSynchronize(h->stream));             // (an earlier count may still read the old buffer)
        HIPC(h->fx_out.ensure(len + 64));
    }
    fx_scan(h, h->stream, d_text, len, format);
    fx_apply(h, h->stream, d_text, len, format, h->fx_out.as<char>());
    // the count path plans its slices and scratch from the batch size on the host: one 16-byte read per call
    rc = fx_read_result(h, h->stream); if (rc) return rc;
    if (h->fx_host()->bad) { h->fx_bad = format; return KQ_OK; }       // not counted; kq_sync reports it
    HistCacheOff guard(h);
    return count_seq_dev(h, h->fx_out.as<const char>(), nullptr, h->fx_host()->n_bases);
}

int kq_count_fastx_async(kq_handle* h, const char* text, uint64_t len, int format, uint64_t* ticket) {
    int rc = fx_args(h, text, len, format);
    if (rc) return rc;
    if (!ticket) return fail(KQ_ERR_INVALID, "null argument");
    if (!len) return ingest_async(h, nullptr, 0, nullptr, 0, 0, ticket);
    HIPC(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lock(h->in_m);
    int s = 0; hipEvent_t copied;
    rc = ingest_begin(h, len, ticket, &s, &copied); if (rc) return rc;
    if (h->in_cmp[s].bytes() < len + 64) {
        if (h->in_cmp[s]) { HIPC(hipStreamSynchronize(h->copy_stream.get())); HIPC(hipStreamSynchronize(h->stream)); }
        HIPC(h->in_cmp[s].ensure(len + 64));
    }
    rc = fx_prepare(h, fx_units_of(h->in_buf[s].as<const char>(), len)); if (rc) return rc;
    // copy and parse on the copy stream: beside the counting of earlier batches.  The call waits for ITS OWN copy and parse
    // (the batch size plans the count on the host), never for the counting of earlier batches unless the ring is full
    char* d = h->in_buf[s].as<char>();
    HIPC(hipMemcpyAsync(d, text, len, hipMemcpyHostToDevice, h->copy_stream.get()));
    HIPC(hipEventRecord(copied, h->copy_stream.get()));
    fx_scan(h, h->copy_stream.get(), d, len, format);
    fx_apply(h, h->copy_stream.get(), d, len, format, h->in_cmp[s].as<char>());
    rc = fx_read_result(h, h->copy_stream.get()); if (rc) return rc;
    if (h->fx_host()->bad) {
        h->in_bad[*ticket % kq_handle::IN_TICKETS] = (uint8_t)format;
        h->fx_bad = format;
        rc = KQ_OK;
    } else {
        HistCacheOff guard(h);
        rc = count_seq_dev(h, h->in_cmp[s].as<const char>(), nullptr, h->fx_host()->n_bases);
    }
    HIPC(hipEventRecord(h->in_consumed[s].get(), h->stream));
    return rc;
}

// ---- BGZF members on the device (kq_bgzf.h, kq_bgzf_host.h, kq_inflate_core.h) --------------------------------------------

static_assert(sizeof(kq_bgzf_block) == sizeof(kqbgzf::Block) && offsetof(kq_bgzf_block, isize) == offsetof(kqbgzf::Block, isize), "kq_bgzf_block is kqbgzf::Block");

int kq_bgzf_scan(const void* data, uint64_t len, kq_bgzf_block* blocks, uint64_t cap, uint64_t* n_blocks, uint64_t* consumed) {
    if ((!data && len) || (!blocks && cap) || !n_blocks || !consumed) return fail(KQ_ERR_INVALID, "null argument");
    const int rc = kqbgzf::scan(data, len, reinterpret_cast<kqbgzf::Block*>(blocks), cap, n_blocks, consumed);
    if (rc == KQ_ERR_INVALID) return fail(rc, "the gzip member at byte %llu is not a BGZF block", (unsigned long long)*consumed);
    if (rc == KQ_ERR_CAPACITY) return fail(rc, "block array too small: %llu blocks, room for %llu", (unsigned long long)*n_blocks, (unsigned long long)cap);
    return rc;
}

// the list lies inside comp_len and every size is one a member can have -> *n_text = the sum of ISIZE
static int bz_check(const kq_bgzf_block* blocks, uint64_t n_blocks, uint64_t comp_len, uint64_t* n_text) {
    if (n_blocks >= (1ull << 31)) return fail(KQ_ERR_INVALID, "2^31 BGZF blocks or more in one call");
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_blocks; ++i) {
        const kq_bgzf_block& b = blocks[i];
        const bool inside = b.off <= comp_len && b.size <= comp_len - b.off;
        const bool shaped = b.size <= 65536 && (uint64_t)b.data_off + b.data_len + 8 <= b.size && b.isize <= kqbgzf::MAX_ISIZE;
        if (!inside || !shaped)
            return fail(KQ_ERR_INVALID, "BGZF block %llu (offset %llu, %u bytes) %s", (unsigned long long)i, (unsigned long long)b.off, b.size,
                        inside ? "has impossible sizes" : "does not lie inside the compressed buffer");
        total += b.isize;
    }
    *n_text = total;
    return KQ_OK;
}
static int bz_prepare(kq_handle* h, uint64_t n_blocks) {
    if (!h->bz_stat) HIPC(h->bz_stat.alloc(sizeof(BzStatus)));
    if (!h->bz_stat_host) HIPC(h->bz_stat_host.alloc(sizeof(BzStatus)));
    HIPC(h->bz_desc.ensure((size_t)n_blocks * sizeof(BzBlock)));
    HIPC(h->bz_desc_host.ensure((size_t)n_blocks * sizeof(BzBlock)));
    return KQ_OK;
}
// status record: no bad block, no newline, no cut
static int bz_reset_status(kq_handle* h, hipStream_t st) {
    HIPC(hipMemsetAsync(h->bz_stat.get(), 0xFF, sizeof(unsigned long long), st));
    HIPC(hipMemsetAsync(h->bz_stat.as<char>() + sizeof(unsigned long long), 0, sizeof(BzStatus) - sizeof(unsigned long long), st));
    return KQ_OK;
}
// inflate the members into d_text + base, on `st` (which the host has synchronised with since the previous use of the staging).
// The descriptor staging and the status record belong to the handle: like every entry point that works on the handle's stream,
// the BGZF entries take one caller at a time
static int bz_launch(kq_handle* h, hipStream_t st, const void* d_comp, const kq_bgzf_block* blocks, uint64_t n_blocks, char* d_text, uint64_t base) {
    BzBlock* desc = h->bz_desc_host.as<BzBlock>();
    uint64_t out = base;
    for (uint64_t i = 0; i < n_blocks; ++i) {
        BzBlock d;
        d.in_off = blocks[i].off + blocks[i].data_off; d.out_off = out; d.data_len = blocks[i].data_len; d.crc = blocks[i].crc32; d.isize = blocks[i].isize; d.pad = 0;
        desc[i] = d;
        out += blocks[i].isize;
    }
    HIPC(hipMemcpyAsync(h->bz_desc.get(), desc, (size_t)n_blocks * sizeof(BzBlock), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)n_blocks), dim3(64), 0, st, (const uint8_t*)d_comp, h->bz_desc.as<const BzBlock>(), (uint32_t)n_blocks,
                       (uint8_t*)d_text, h->bz_stat.as<BzStatus>());
    HIPC(hipGetLastError());
    return KQ_OK;
}
static int bz_read_status(kq_handle* h, hipStream_t st) {
    HIPC(hipMemcpyAsync(h->bz_stat_host.get(), h->bz_stat.get(), sizeof(BzStatus), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return KQ_OK;
}
static std::string bz_describe(const BzStatus* s) {
    char buf[160];
    snprintf(buf, sizeof buf, "BGZF block %llu is corrupt (%s)", s->first_bad >> 8, kqinf::err_name((int)(s->first_bad & 0xFF)));
    return buf;
}

int kq_inflate_bgzf_dev(kq_handle* h, const void* d_comp, uint64_t comp_len, const kq_bgzf_block* blocks, uint64_t n_blocks, char* d_text, uint64_t cap,
                        uint64_t* n_text) {
    if (!h || !n_text || ((!d_comp || !blocks) && n_blocks)) return fail(KQ_ERR_INVALID, "null argument");
    *n_text = 0;
    if (!n_blocks) return KQ_OK;
    uint64_t total = 0;
    int rc = bz_check(blocks, n_blocks, comp_len, &total); if (rc) return rc;
    *n_text = total;
    if (!d_text) return KQ_OK;
    if (total > cap) return fail(KQ_ERR_CAPACITY, "output buffer too small: %llu bytes of text, room for %llu", (unsigned long long)total, (unsigned long long)cap);
    HIPC(hipSetDevice(h->device));
    rc = bz_prepare(h, n_blocks); if (rc) return rc;
    rc = bz_reset_status(h, h->stream); if (rc) return rc;
    rc = bz_launch(h, h->stream, d_comp, blocks, n_blocks, d_text, 0); if (rc) return rc;
    rc = bz_read_status(h, h->stream); if (rc) return rc;
    const BzStatus* s = h->bz_stat_host.as<BzStatus>();
    if (s->first_bad != ~0ull) return fail(KQ_ERR_INVALID, "%s", bz_describe(s).c_str());
    return KQ_OK;
}

// ---- text -> BGZF members on the device (kq_deflate.h, kq_deflate_core.h) ---------------------------------------------------

constexpr uint64_t DF_BATCH = 4096;      // members per launch: 256 MiB of slots at the most

uint64_t kq_bgzf_bound(uint64_t n_text, uint32_t flags) {
    const uint64_t members = (n_text + kqdef::MEMBER_TEXT - 1) / kqdef::MEMBER_TEXT;
    return n_text + members * (kqdef::HEADER_BYTES + kqdef::STORED_BYTES + kqdef::TRAILER_BYTES) + ((flags & KQ_BGZF_EOF) ? kqdef::EOF_BYTES : 0);
}

int kq_deflate_bgzf_dev(kq_handle* h, const char* d_text, uint64_t n_text, void* d_out, uint64_t cap, uint64_t* n_out, uint32_t flags) {
    if (!h || !n_out || (!d_text && n_text) || (!d_out && cap)) return fail(KQ_ERR_INVALID, "null argument");
    *n_out = 0;
    if (flags & ~(uint32_t)KQ_BGZF_EOF) return fail(KQ_ERR_INVALID, "unknown flag bits %#x", flags);
    const uint64_t bound = kq_bgzf_bound(n_text, flags);
    if (cap < bound) { *n_out = bound; return fail(KQ_ERR_CAPACITY, "output buffer too small: up to %llu bytes of BGZF, room for %llu", (unsigned long long)bound, (unsigned long long)cap); }
    if (!bound) return KQ_OK;
    HIPC(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const uint64_t members = (n_text + kqdef::MEMBER_TEXT - 1) / kqdef::MEMBER_TEXT, batch = std::min(members, DF_BATCH);
    uint64_t total = 0;
    if (members) {
        if (!h->df_stat) HIPC(h->df_stat.alloc(sizeof(DfStatus)));
        if (!h->df_stat_host) HIPC(h->df_stat_host.alloc(sizeof(DfStatus)));
        HIPC(h->df_slots.ensure((size_t)batch * DF_SLOT));
        HIPC(h->df_sizes.ensure((size_t)batch * sizeof(uint32_t)));
        HIPC(h->df_offs.ensure((size_t)batch * sizeof(unsigned long long)));
        HIPC(hipMemsetAsync(h->df_stat.get(), 0xFF, sizeof(unsigned long long), st));                                  // no bad member
        HIPC(hipMemsetAsync(h->df_stat.as<char>() + sizeof(unsigned long long), 0, sizeof(unsigned long long), st));   // nothing written
        for (uint64_t m0 = 0; m0 < members; m0 += batch) {
            const uint32_t nm = (uint32_t)std::min(batch, members - m0);
            hipLaunchKernelGGL(k_bgzf_deflate, dim3(nm), dim3(64), 0, st, (const uint8_t*)d_text, n_text, m0, nm, h->df_slots.as<uint8_t>(), h->df_sizes.as<uint32_t>(),
                               h->df_stat.as<DfStatus>());
            hipLaunchKernelGGL(k_bgzf_sizes_scan, dim3(1), dim3(64), 0, st, h->df_sizes.as<const uint32_t>(), nm, h->df_offs.as<unsigned long long>(), h->df_stat.as<DfStatus>());
            hipLaunchKernelGGL(k_bgzf_gather, dim3(nm), dim3(DF_GATHER_THREADS), 0, st, h->df_slots.as<const uint8_t>(), h->df_sizes.as<const uint32_t>(),
                               h->df_offs.as<const unsigned long long>(), nm, (uint8_t*)d_out);
            HIPC(hipGetLastError());
        }
        HIPC(hipMemcpyAsync(h->df_stat_host.get(), h->df_stat.get(), sizeof(DfStatus), hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        const DfStatus* s = h->df_stat_host.as<DfStatus>();
        if (s->first_bad != ~0ull)
            return fail(KQ_ERR_INVALID, "BGZF member %llu could not be written (%s)", s->first_bad >> 8, kqdef::err_name((int)(s->first_bad & 0xFF)));
        total = s->total;
        if (total + ((flags & KQ_BGZF_EOF) ? kqdef::EOF_BYTES : 0) > bound) return fail(KQ_ERR_INVALID, "the BGZF writer produced %llu bytes, above its bound %llu", (unsigned long long)total, (unsigned long long)bound);
    }
    if (flags & KQ_BGZF_EOF) {
        static uint8_t eof[kqdef::EOF_BYTES];
        for (uint32_t i = 0; i < kqdef::EOF_BYTES; ++i) eof[i] = (uint8_t)kqdef::eof_byte(i);
        HIPC(hipMemcpyAsync((uint8_t*)d_out + total, eof, kqdef::EOF_BYTES, hipMemcpyHostToDevice, st));
        HIPC(hipStreamSynchronize(st));
        total += kqdef::EOF_BYTES;
    }
    *n_out = total;
    return KQ_OK;
}

int kq_deflate_bgzf(kq_handle* h, const char* text, uint64_t n_text, void* out, uint64_t cap, uint64_t* n_out, uint32_t flags) {
    if (!h || !n_out || (!text && n_text) || (!out && cap)) return fail(KQ_ERR_INVALID, "null argument");
    *n_out = 0;
    if (flags & ~(uint32_t)KQ_BGZF_EOF) return fail(KQ_ERR_INVALID, "unknown flag bits %#x", flags);
    const uint64_t bound = kq_bgzf_bound(n_text, flags);
    if (cap < bound) { *n_out = bound; return fail(KQ_ERR_CAPACITY, "output buffer too small: up to %llu bytes of BGZF, room for %llu", (unsigned long long)bound, (unsigned long long)cap); }
    if (!bound) return KQ_OK;
    HIPC(hipSetDevice(h->device));
    HIPC(h->df_in.ensure((size_t)n_text + 16));
    HIPC(h->df_out.ensure((size_t)bound));
    if (n_text) HIPC(hipMemcpyAsync(h->df_in.get(), text, (size_t)n_text, hipMemcpyHostToDevice, h->stream));
    const int rc = kq_deflate_bgzf_dev(h, h->df_in.as<const char>(), n_text, h->df_out.get(), bound, n_out, flags);
    if (rc) return rc;
    HIPC(hipMemcpyAsync(out, h->df_out.get(), (size_t)*n_out, hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    return KQ_OK;
}

static int bz_args(kq_handle* h, const void* comp, const kq_bgzf_block* blocks, uint64_t n_blocks, int format, uint32_t flags) {
    if (!h || ((!comp || !blocks) && n_blocks)) return fail(KQ_ERR_INVALID, "null argument");
    if (format != KQ_FASTX_FASTQ && format != KQ_FASTX_FASTA) return fail(KQ_ERR_INVALID, "format must be KQ_FASTX_FASTQ or KQ_FASTX_FASTA, not %d", format);
    if (flags & ~(uint32_t)KQ_BGZF_END) return fail(KQ_ERR_INVALID, "unknown flag bits %#x", flags);
    return KQ_OK;
}
// One step of a BGZF stream, on the handle's stream: carry + the members' text -> cut -> parse [0, cut) into fx_out -> count it;
// [cut, end) is the next carry.  Two small read-backs: the status record (bad member, cut), then the parser's batch size.
static int bz_count_step(kq_handle* h, const void* d_comp, const kq_bgzf_block* blocks, uint64_t n_blocks, uint64_t n_new, int format, uint32_t flags) {
    const hipStream_t st = h->stream;
    DevMem& parsed = h->fx_out;
    const uint64_t carry = h->bz_carry_len, total = carry + n_new;
    const bool end = (flags & KQ_BGZF_END) != 0;
    if (!total) return KQ_OK;
    int rc = bz_prepare(h, n_blocks); if (rc) return rc;
    if (h->bz_text.bytes() < total + 64) {
        HIPC(hipStreamSynchronize(st));                    // (nothing may still read the old buffer)
        HIPC(h->bz_text.ensure(total + 64));
    }
    char* text = h->bz_text.as<char>();
    if (carry) HIPC(hipMemcpyAsync(text, h->bz_carry.get(), carry, hipMemcpyDeviceToDevice, st));
    rc = bz_reset_status(h, st); if (rc) return rc;
    if (n_blocks) { rc = bz_launch(h, st, d_comp, blocks, n_blocks, text, carry); if (rc) return rc; }
    if (!end) {
        if (format == KQ_FASTX_FASTQ) {
            hipLaunchKernelGGL(k_bgzf_count_nl, dim3(grid_for(h, (total + 15) / 16, 256)), dim3(256), 0, st, (const uint8_t*)text, total, h->bz_stat.as<BzStatus>());
            hipLaunchKernelGGL((k_bgzf_cut<FX_FASTQ>), dim3(1), dim3(BZ_CUT_THREADS), 0, st, (const uint8_t*)text, total, h->bz_stat.as<BzStatus>());
        } else hipLaunchKernelGGL((k_bgzf_cut<FX_FASTA>), dim3(1), dim3(BZ_CUT_THREADS), 0, st, (const uint8_t*)text, total, h->bz_stat.as<BzStatus>());
        HIPC(hipGetLastError());
    }
    rc = bz_read_status(h, st); if (rc) return rc;
    const BzStatus* s = h->bz_stat_host.as<BzStatus>();
    if (s->first_bad != ~0ull) {
        // not counted, and the stream ends here: kq_sync reports it up to kq_clear
        h->bz_bad = true; h->bz_err = bz_describe(s); h->bz_carry_len = 0;
        return KQ_OK;
    }
    const uint64_t cut = end ? total : std::min<uint64_t>(s->cut, total);
    h->bz_carry_len = total - cut;
    if (total > cut) {
        // the carry was copied into the text above and `st` has been synchronised since: its buffer may be replaced
        HIPC(h->bz_carry.ensure(total - cut));
        HIPC(hipMemcpyAsync(h->bz_carry.get(), text + cut, total - cut, hipMemcpyDeviceToDevice, st));
    }
    if (!cut) { HIPC(hipStreamSynchronize(st)); return KQ_OK; }
    rc = fx_prepare(h, fx_units_of(text, cut)); if (rc) return rc;
    if (parsed.bytes() < cut + 64) {
        if (parsed) HIPC(hipStreamSynchronize(st));        // (an earlier count may still read the old buffer)
        HIPC(parsed.ensure(cut + 64));
    }
    fx_scan(h, st, text, cut, format);
    fx_apply(h, st, text, cut, format, parsed.as<char>());
    rc = fx_read_result(h, st); if (rc) return rc;             // (the carry has been copied by now, too)
    if (h->fx_host()->bad) { h->fx_bad = format; return KQ_OK; }       // not counted; kq_sync reports it
    HistCacheOff guard(h);
    return count_seq_dev(h, parsed.as<const char>(), nullptr, h->fx_host()->n_bases);
}

int kq_count_bgzf_dev(kq_handle* h, const void* d_comp, uint64_t comp_len, const kq_bgzf_block* blocks, uint64_t n_blocks, int format, uint32_t flags) {
    int rc = bz_args(h, d_comp, blocks, n_blocks, format, flags); if (rc) return rc;
    uint64_t n_new = 0;
    rc = bz_check(blocks, n_blocks, comp_len, &n_new); if (rc) return rc;
    HIPC(hipSetDevice(h->device));
    return bz_count_step(h, d_comp, blocks, n_blocks, n_new, format, flags);
}

static int emit_ordered(kq_handle* h, const char* d_bases, uint64_t len, uint64_t* d_keys, uint8_t* d_edges, uint64_t cap,
                        uint64_t* n_out) {
    const uint8_t* ab; uint64_t lead;
    aligned_view(d_bases, &ab, &lead);
    const uint64_t nt = n_tiles_of(lead, len);
    HIPC(h->scratch.ensure((nt + 2) * sizeof(unsigned long long)));
    unsigned long long* tile_counts = h->scratch.as<unsigned long long>();
    unsigned long long* total = tile_counts + nt;
    int grid = grid_for(h, nt, 1);
    hipLaunchKernelGGL(k_emit_count, dim3(grid), dim3(TILE_THREADS), 0, h->stream, ab, lead, len, h->k, tile_counts);
    hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(1024), 0, h->stream, tile_counts, nt, total);
    unsigned long long n = 0;
    HIPC(hipMemcpyAsync(&n, total, sizeof n, hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    *n_out = n;
    if (!d_keys || !d_edges) return KQ_OK;
    if (n > cap) return fail(KQ_ERR_CAPACITY, "record buffer too small: need %llu, have %llu", n, (unsigned long long)cap);
    hipLaunchKernelGGL(k_emit_write, dim3(grid), dim3(TILE_THREADS), 0, h->stream, ab, lead, len, h->k, tile_counts, d_keys, d_edges, cap);
    HIPC(hipGetLastError());
    return KQ_OK;
}

int kq_emit_records(kq_handle* h, const char* bases, uint64_t len, uint64_t* keys, uint8_t* edges, uint64_t cap, uint64_t* n_out) {
    if (!h || !n_out || (!bases && len)) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    *n_out = 0;
    if (len < (uint64_t)h->k) return KQ_OK;
    void* d = nullptr;
    int rc = stage_in(h, bases, len, &d);
    if (rc) return rc;
    if (!keys || !edges) return emit_ordered(h, (const char*)d, len, nullptr, nullptr, 0, n_out);
    rc = emit_ordered(h, (const char*)d, len, nullptr, nullptr, 0, n_out);
    if (rc) return rc;
    if (*n_out > cap) return fail(KQ_ERR_CAPACITY, "record buffer too small: need %llu, have %llu", (unsigned long long)*n_out, (unsigned long long)cap);
    uint64_t n = *n_out;
    DevScope mem;
    uint64_t* dk = nullptr; uint8_t* de = nullptr;
    if (n) {
        HIPC(mem.alloc((void**)&dk, n * sizeof(uint64_t)));
        if (mem.alloc((void**)&de, n) != hipSuccess) return fail(KQ_ERR_NOMEM, "record buffer allocation failed");
        rc = emit_ordered(h, (const char*)d, len, dk, de, n, n_out);
        if (!rc) {
            hipError_t e1 = hipMemcpyAsync(keys, dk, n * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream);
            hipError_t e2 = hipMemcpyAsync(edges, de, n, hipMemcpyDeviceToHost, h->stream);
            hipError_t e3 = hipStreamSynchronize(h->stream);
            if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) rc = fail(KQ_ERR_HIP, "copying records back failed");
        }
    }
    return rc;
}

// owner split of a resident batch (multi-GPU staging): records grouped by owner part in d_recs.  `packed`: packed 8-byte records
// (kq_emit_packed_dev), else WIDE records (raw key + reference edge byte in d_edges, kq_emit_partitioned_dev)
static int owner_split(kq_handle* h, const char* d_bases, uint64_t len, int n_parts, uint64_t* d_recs, uint8_t* d_edges, bool packed, uint64_t cap, uint64_t* part_counts) {
    if (!h || !part_counts || n_parts < 1 || n_parts > h->map_count || n_parts >= NB_MAX || (!d_bases && len)) return fail(KQ_ERR_INVALID, "bad argument");
    if (packed && h->k > PART_MAX_K) return fail(KQ_ERR_INVALID, "packed 8-byte records need k <= %d (use kq_emit_partitioned_dev)", PART_MAX_K);
    HIPC(hipSetDevice(h->device));
    for (int i = 0; i < n_parts; ++i) part_counts[i] = 0;
    if (len < (uint64_t)h->k) return KQ_OK;
    if (len - h->k + 1 >= (1ull << 32) - 16) return fail(KQ_ERR_INVALID, "an owner split handles fewer than 2^32 k-mer starts per call (got %llu): cut the batch", (unsigned long long)(len - h->k + 1));
    if (cap < len - h->k + 1 || !d_recs || (!packed && !d_edges)) return fail(KQ_ERR_CAPACITY, "record buffer too small: need room for %llu records", (unsigned long long)(len - h->k + 1));
    const uint8_t* ab; uint64_t lead;
    aligned_view(d_bases, &ab, &lead);
    PartPlan p;
    const uint32_t sb = owner_sub_bits(n_parts);
    const uint32_t bins = (uint32_t)n_parts << sb;
    int rc = plan_alloc(h, &p, 0, n_tiles_of(lead, len), bins);
    if (rc) return rc;
    PartCfg cfg = p.cfg;
    cfg.mode = 1; cfg.n_coarse = bins; cfg.owner_sub = sb;
    if (!packed) cfg.raw_out = 1;
    rc = run_p1(h, &p, cfg, ab, lead, len, EmitRange{0, ~0ull}, d_recs, packed ? nullptr : d_edges, packed ? AUX_IDX6 : AUX_EDGE_BYTE);
    if (rc) return rc;
    std::vector<unsigned long long> off((size_t)bins + 1);
    HIPC(hipMemcpyAsync(off.data(), p.seg_off, off.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n_parts; ++i) part_counts[i] = off[((size_t)i + 1) << sb] - off[(size_t)i << sb];
    return KQ_OK;
}

int kq_emit_partitioned_dev(kq_handle* h, const char* d_bases, uint64_t len, int n_parts, uint64_t* d_keys, uint8_t* d_edges, uint64_t cap, uint64_t* part_counts) {
    return owner_split(h, d_bases, len, n_parts, d_keys, d_edges, false, cap, part_counts);
}
int kq_emit_packed_dev(kq_handle* h, const char* d_bases, uint64_t len, int n_parts, uint64_t* d_recs, uint64_t cap, uint64_t* part_counts) {
    return owner_split(h, d_bases, len, n_parts, d_recs, nullptr, true, cap, part_counts);
}

// ---- multi-GPU exchange of 5-byte records (k <= 21) -------------------------------------------------
// Ownership is by hash-prefix bucket range, so the sender's work is the first split of the single-GPU count and nothing
// else: P1 writes the bucket-sorted 5-byte records straight into the send buffers, the part of every destination rank is
// one contiguous run.  Receiver (a table that is the window of its buckets, KQ_OPT_BUCKET_WINDOW): the runs of all peers
// are (peer, bucket) segments of its bucket -> region levels, so the received records enter the ordinary narrow path.
// 5 bytes per record cross xGMI.  kq_emit_packed_dev / kq_insert_packed_dev remain for k = 22..28 and small tables.
// (peer q, bucket b) run j = q * 256 + b of the received array -> input segment b * n_peers + q of the receive levels
__global__ void k_sharded_segments(const unsigned long long* __restrict__ start /*exclusive scan of the counts, peer-major*/,
                                   const unsigned long long* __restrict__ counts, uint32_t n_peers,
                                   unsigned long long* __restrict__ seg_lo, unsigned long long* __restrict__ seg_hi) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_peers << NARROW_CBITS) return;
    const uint32_t q = j >> NARROW_CBITS, b = j & ((1u << NARROW_CBITS) - 1u);
    seg_lo[b * n_peers + q] = start[j];
    seg_hi[b * n_peers + q] = start[j] + counts[j];
}

// (the parts are contiguous ranges of the 256 hash-prefix buckets: part_first_bucket, kq_plan_host.h)
__global__ void k_bucket_meta(const unsigned long long* __restrict__ seg_off, uint32_t n_parts, unsigned long long* __restrict__ counts) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_parts << NARROW_CBITS) return;
    const uint32_t p = j >> NARROW_CBITS, b = j & ((1u << NARROW_CBITS) - 1u);
    const uint32_t lo = (uint32_t)(((uint64_t)p * 256 + n_parts - 1) / n_parts), hi = (uint32_t)(((uint64_t)(p + 1) * 256 + n_parts - 1) / n_parts);
    counts[j] = (b >= lo && b < hi) ? seg_off[b + 1] - seg_off[b] : 0ull;
}
// `five`: 5-byte records (u32 + lockstep byte in d_aux), else 8-byte hash-remainder records (see below; d_aux = nullptr)
static int emit_buckets(kq_handle* h, const char* d_bases, uint64_t len, int n_parts, uint64_t* d_recs, uint8_t* d_aux, bool five, uint64_t cap,
                        uint64_t* d_bucket_counts, uint64_t* part_counts) {
    if (!h || !d_bucket_counts || n_parts < 1 || n_parts > 256 || (!d_bases && len)) return fail(KQ_ERR_INVALID, "bad argument");
    if (five && h->k > (int)NARROW_MAX_K) return fail(KQ_ERR_INVALID, "5-byte records need k <= %u (use kq_emit_packed_dev)", NARROW_MAX_K);
    if (!five && h->k <= PART_MAX_K) return fail(KQ_ERR_INVALID, "8-byte hash-remainder records need k >= %d (use kq_emit_sharded_dev or kq_emit_packed_dev)", HI_K);
    HIPC(hipSetDevice(h->device));
    for (int i = 0; part_counts && i < n_parts; ++i) part_counts[i] = 0;
    const uint64_t n_groups = (uint64_t)n_parts << NARROW_CBITS;
    HIPC(hipMemsetAsync(d_bucket_counts, 0, n_groups * 8, h->stream));
    if (len < (uint64_t)h->k) { if (part_counts) HIPC(hipStreamSynchronize(h->stream)); return KQ_OK; }
    if (len - h->k + 1 >= (1ull << 32) - 16) return fail(KQ_ERR_INVALID, "a bucket split handles fewer than 2^32 k-mer starts per call (got %llu): cut the batch", (unsigned long long)(len - h->k + 1));
    if (cap < len - h->k + 1 || !d_recs || (five && !d_aux)) return fail(KQ_ERR_CAPACITY, "record buffer%s too small: need room for %llu records", five ? "s" : "", (unsigned long long)(len - h->k + 1));
    const uint8_t* ab; uint64_t lead;
    aligned_view(d_bases, &ab, &lead);
    PartPlan p;
    // (P1 writes into the caller's buffers: the 8-byte form asks for no record scratch, the 5-byte form for its historical `len` records)
    int rc = plan_alloc(h, &p, five ? len : 0, n_tiles_of(lead, len), 1u << NARROW_CBITS, true, n_groups);
    if (rc) return rc;
    // the bucket split of the single-GPU count IS the owner split: bucket = top 8 hash bits, whatever this rank's table
    // looks like (plan_cfg leaves the window of the sending handle out: every bucket is emitted), and every part is a range
    // of buckets -- P1 writes straight into the send buffers
    PartCfg cfg = p.cfg;
    cfg.mode = 0; cfg.narrow = 1; cfg.n_coarse = 1u << NARROW_CBITS; cfg.sub_bits = 0; if (cfg.g_shift == 0) cfg.g_shift = 1;
    cfg.filt_lo = 0; cfg.filt_hi = cfg.map_count;
    rc = run_p1(h, &p, cfg, ab, lead, len, EmitRange{0, ~0ull}, d_recs, five ? d_aux : nullptr, AUX_IDX6);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bucket_meta, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, h->stream, p.seg_off, (uint32_t)n_parts, (unsigned long long*)d_bucket_counts);
    HIPC(hipGetLastError());
    if (!part_counts) return KQ_OK;               // asynchronous: the caller takes the part sizes from the rows of d_bucket_counts
    std::vector<unsigned long long> off((size_t)(1u << NARROW_CBITS) + 1);
    HIPC(hipMemcpyAsync(off.data(), p.seg_off, off.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n_parts; ++i) part_counts[i] = off[part_first_bucket(i + 1, n_parts)] - off[part_first_bucket(i, n_parts)];
    return KQ_OK;
}
// receive side: the (peer, bucket) runs of all peers enter the table's bucket -> region levels
static int insert_buckets(kq_handle* h, const uint64_t* d_recs, const uint8_t* d_aux, bool five, uint64_t n, int n_peers, const uint64_t* d_bucket_counts) {
    if (!h || ((!d_recs || (five && !d_aux)) && n) || !d_bucket_counts || n_peers < 1 || n_peers > 256) return fail(KQ_ERR_INVALID, "bad argument");
    if (five && h->k > (int)NARROW_MAX_K) return fail(KQ_ERR_INVALID, "5-byte records need k <= %u (use kq_insert_packed_dev)", NARROW_MAX_K);
    if (!five && h->k <= PART_MAX_K) return fail(KQ_ERR_INVALID, "8-byte hash-remainder records need k >= %d (use kq_insert_sharded_dev or kq_insert_packed_dev)", HI_K);
    HIPC(hipSetDevice(h->device));
    if (!n) return KQ_OK;
    if (n >= (1ull << 32) - 16) return fail(KQ_ERR_INVALID, "a partition pass handles fewer than 2^32 records (got %llu)", (unsigned long long)n);
    if (!five) {   // the format of the plan the table allows, before anything is reserved or grown for records it cannot take
        if (!plan_cfg(h->shape(), true).narrow) return fail(KQ_ERR_INVALID, "the table has no hash-prefix bucket split for 8-byte hash-remainder records (fewer than 2048 regions): use kq_insert_records_dev");
    }
    int rc = reserve(h, n, n);
    if (rc) return rc;
    const uint32_t n_in = (uint32_t)n_peers << NARROW_CBITS;      // input segments: one run per (bucket, peer)
    PartPlan p;
    rc = plan_alloc(h, &p, n, 0, 1, true, n_in);
    if (rc) return rc;
    if (five && p.fmt != FMT_NARROW) return fail(KQ_ERR_INVALID, "the table is too small for 5-byte records (fewer than 2048 regions): use kq_insert_packed_dev");
    if (!five && p.fmt != FMT_TOP8) return fail(KQ_ERR_INVALID, "the table has no hash-prefix bucket split for 8-byte hash-remainder records: use kq_insert_records_dev");
    // segment table of the received array (peer-major runs) in logical order (bucket-major)
    HIPC(h->scratch.ensure((size_t)(3 * (n_in + 2)) * 8));
    unsigned long long* start = h->scratch.as<unsigned long long>();
    unsigned long long* seg_lo = start + n_in + 2;
    unsigned long long* seg_hi = seg_lo + n_in + 2;
    HIPC(hipMemcpyAsync(start, d_bucket_counts, (size_t)n_in * 8, hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(1024), 0, h->stream, start, (uint64_t)n_in, start + n_in);
    hipLaunchKernelGGL(k_sharded_segments, dim3((n_in + 255) / 256), dim3(256), 0, h->stream, start, (const unsigned long long*)d_bucket_counts, (uint32_t)n_peers, seg_lo, seg_hi);
    Dest dst{p.fmt, AUX_IDX6};
    rc = dest_take(h, p, p.n_max, &dst); if (rc) return rc;
    // the first level reads the received runs; the table pass visits the window's regions only, so records of foreign buckets
    // are sorted and never applied
    const LevelIn runs{d_recs, five ? d_aux : nullptr, seg_lo, seg_hi, n_in, (uint32_t)n_peers};
    return sort_and_submit(h, &p, runs, dst);
}
int kq_emit_sharded_dev(kq_handle* h, const char* d_bases, uint64_t len, int n_parts, uint32_t* d_recs, uint8_t* d_aux, uint64_t cap, uint64_t* d_bucket_counts, uint64_t* part_counts) {
    return emit_buckets(h, d_bases, len, n_parts, (uint64_t*)d_recs, d_aux, true, cap, d_bucket_counts, part_counts);
}
int kq_insert_sharded_dev(kq_handle* h, const uint32_t* d_recs, const uint8_t* d_aux, uint64_t n, int n_peers, const uint64_t* d_bucket_counts) {
    return insert_buckets(h, (const uint64_t*)d_recs, d_aux, true, n, n_peers, d_bucket_counts);
}

// ---- multi-GPU exchange of 8-byte hash-remainder records (k = 29..32) -------------------------------
// The same glue for FMT_TOP8: a record plus its bucket is the whole k-mer (top8_hash), tables of k >= HI_K have the bucket
// geometry at every size, so ownership by bucket range makes P1 the owner split here too.  One u64 array crosses the link
// (the 9-byte path: u64 key + edge byte in two arrays, hashed again by the receiver), and the receiver's levels start from
// the (peer, bucket) runs.  kq_emit_partitioned_dev / kq_insert_records_dev remain for tables below 2048 regions.
int kq_emit_sharded8_dev(kq_handle* h, const char* d_bases, uint64_t len, int n_parts, uint64_t* d_recs, uint64_t cap, uint64_t* d_bucket_counts, uint64_t* part_counts) {
    return emit_buckets(h, d_bases, len, n_parts, d_recs, nullptr, false, cap, d_bucket_counts, part_counts);
}
int kq_insert_sharded8_dev(kq_handle* h, const uint64_t* d_recs, uint64_t n, int n_peers, const uint64_t* d_bucket_counts) {
    return insert_buckets(h, d_recs, nullptr, false, n, n_peers, d_bucket_counts);
}

int kq_insert_packed_dev(kq_handle* h, const uint64_t* d_recs, uint64_t n) {
    if (!h || (!d_recs && n)) return fail(KQ_ERR_INVALID, "null argument");
    if (h->k > PART_MAX_K) return fail(KQ_ERR_INVALID, "packed 8-byte records need k <= %d (use kq_insert_records_dev)", PART_MAX_K);
    HIPC(hipSetDevice(h->device));
    if (!n) return KQ_OK;
    int rc = reserve(h, n, n);
    if (rc) return rc;
    if (!part_table_ok(h->shape(), true)) return fail(KQ_ERR_INVALID, "table too large for the partitioned path");
    return count_partitioned_records(h, d_recs, nullptr, AUX_IDX6, n, false);
}

int kq_insert_records_dev(kq_handle* h, const uint64_t* d_keys, const uint8_t* d_edges, uint64_t n) {
    if (!h || ((!d_keys || !d_edges) && n)) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    if (!n) return KQ_OK;
    int rc = reserve(h, n, n);
    if (rc) return rc;
    if ((h->count_path == 2 || (h->count_path == 0 && n >= (1u << 20))) && h->n_regions <= (1ull << 20)) {   // WIDE records: key + reference edge byte
        return count_partitioned_records(h, d_keys, d_edges, AUX_EDGE_BYTE, n, true);
    }
    materialize(h);
    h->table_empty = false;
    hipLaunchKernelGGL(k_insert_records, dim3(grid_for(h, n, 256)), dim3(256), 0, h->stream, h->view(), d_keys, d_edges, n);
    HIPC(hipGetLastError());
    return KQ_OK;
}
int kq_insert_records(kq_handle* h, const uint64_t* keys, const uint8_t* edges, uint64_t n) {
    if (!h || ((!keys || !edges) && n)) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    if (!n) return KQ_OK;
    HIPC(h->stage.ensure(n * 9 + 64));
    uint64_t* dk = h->stage.as<uint64_t>();
    uint8_t* de = h->stage.as<uint8_t>() + n * 8;
    HIPC(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, h->stream));
    HIPC(hipMemcpyAsync(de, edges, n, hipMemcpyHostToDevice, h->stream));
    int rc = kq_insert_records_dev(h, dk, de, n);
    if (rc) return rc;
    return kq_sync(h);
}

// ---- summary ---------------------------------------------------------------------------------
struct SummaryHost { SummaryOut so; std::vector<unsigned long long> small; std::vector<uint32_t> big; };
static int run_summary(kq_handle* h, SummaryHost* r) {
    const uint64_t big_cap = h->hc_cap;     // cov >= 4096 implies a high-copy k-mer
    size_t need = sizeof(SummaryOut) + HIST_SMALL * sizeof(unsigned long long) + big_cap * sizeof(uint32_t);
    HIPC(h->scratch.ensure(need));
    SummaryOut* d_so = h->scratch.as<SummaryOut>();
    unsigned long long* d_small = (unsigned long long*)(d_so + 1);
    uint32_t* d_big = (uint32_t*)(d_small + HIST_SMALL);
    HIPC(hipMemsetAsync(h->scratch.get(), 0, sizeof(SummaryOut) + HIST_SMALL * sizeof(unsigned long long), h->stream));
    SummaryOut init; memset(&init, 0, sizeof init); init.big_cap = big_cap;
    HIPC(hipMemcpyAsync(d_so, &init, sizeof init, hipMemcpyHostToDevice, h->stream));
    materialize(h);
    hipLaunchKernelGGL(k_summary, dim3(grid_for(h, h->n_slots(), 1024)), dim3(256), 0, h->stream, h->view(), d_so, d_small, d_big);
    r->small.resize(HIST_SMALL);
    HIPC(hipMemcpyAsync(&r->so, d_so, sizeof(SummaryOut), hipMemcpyDeviceToHost, h->stream));
    HIPC(hipMemcpyAsync(r->small.data(), d_small, HIST_SMALL * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    if (r->so.n_big > big_cap) return fail(KQ_ERR_HIP, "summary: high-coverage list overflow");
    r->big.resize(r->so.n_big);
    if (r->so.n_big) {
        HIPC(hipMemcpyAsync(r->big.data(), d_big, r->so.n_big * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPC(hipStreamSynchronize(h->stream));
    }
    return KQ_OK;
}
int kq_summary(kq_handle* h, kq_stats* out) {
    if (!h || !out) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    int rc = check_errors(h);
    if (rc) return rc;
    SummaryHost r;
    rc = run_summary(h, &r);
    if (rc) return rc;
    out->total = r.so.total; out->unique = r.so.uniq; out->distinct = r.so.distinct; out->edges = r.so.edges;
    const uint64_t space = h->k < 32 ? (1ull << (2 * h->k)) : 0ull;          // src/graph-builder.cpp:286
    out->missing = space - out->distinct;
    return KQ_OK;
}
int kq_histogram(kq_handle* h, uint64_t* cov, uint64_t* cnt, uint64_t cap, uint64_t* n_out) {
    if (!h || !n_out) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    int rc = check_errors(h);
    if (rc) return rc;
    SummaryHost r;
    rc = run_summary(h, &r);
    if (rc) return rc;
    std::vector<std::pair<uint64_t, uint64_t>> hist;
    for (uint32_t c = 0; c < HIST_SMALL; ++c) if (r.small[c]) hist.emplace_back(c, r.small[c]);
    std::sort(r.big.begin(), r.big.end());
    for (size_t i = 0; i < r.big.size();) {
        size_t j = i; while (j < r.big.size() && r.big[j] == r.big[i]) ++j;
        hist.emplace_back(r.big[i], j - i);
        i = j;
    }
    *n_out = hist.size();
    if (!cov || !cnt) return KQ_OK;
    if (hist.size() > cap) return fail(KQ_ERR_CAPACITY, "histogram buffer too small: need %zu", hist.size());
    for (size_t i = 0; i < hist.size(); ++i) { cov[i] = hist[i].first; cnt[i] = hist[i].second; }
    return KQ_OK;
}

// ---- lookup ----------------------------------------------------------------------------------
// K3 through the partition machinery (counters only): P1 -> (level) -> k_lookup_regions
static int lookup_partitioned(kq_handle* h, const uint8_t* ab, uint64_t lead, uint64_t len, EmitRange er, uint32_t cov_cutoff,
                              uint32_t map_lo, uint32_t map_hi, unsigned long long* d_counters) {
    PartPlan p;
    int rc = plan_sequence(h, &p, lead, len);
    if (rc) return rc;
    p.cfg.filt_lo = map_lo; p.cfg.filt_hi = map_hi;               // the reference's range filter, src/kreeq.cpp:150
    rc = run_p1(h, &p, p.cfg, ab, lead, len, er, p.recs1, p.a1(), AUX_IDX6);
    if (rc) return rc;
    P3Set set;
    rc = sort_to_regions(h, &p, own_segments(p, p.recs1, p.a1(), p.cfg.n_coarse), Dest{p.fmt, AUX_IDX6}, &set);      // in the scratch, never tight
    if (rc) return rc;
    const uint32_t rps = (p.fmt == FMT_NARROW || p.fmt == FMT_TOP8) ? (uint32_t)(p.R >> NARROW_CBITS) : 1u;
    static const KernelRow<decltype(&k_lookup_regions<0>)> rows[] = {lkr<FMT_NARROW>(), lkr<FMT_TOP8>(), lkr<FMT_WIDE>(), lkr<FMT_PACK8>()};
    rc = launch_row(rows, "k_lookup_regions", select_lookup(p.fmt), h, dim3((unsigned)std::min<uint64_t>(p.R, 1u << 30)), dim3(P3_THREADS), h->view(), set.recs, set.aux, set.base, rps, cov_cutoff, d_counters);
    if (rc) return rc;
    HIPC(hipGetLastError());
    return KQ_OK;
}

int kq_lookup_sequence_dev(kq_handle* h, const char* d_bases, uint64_t len, uint32_t cov_cutoff, uint16_t map_lo, uint16_t map_hi,
                           kq_dbgbase* d_per_base, uint64_t* d_counters) {
    if (!h || !d_counters || (!d_bases && len)) return fail(KQ_ERR_INVALID, "null argument");
    if (map_lo > map_hi || map_hi > h->map_count) return fail(KQ_ERR_INVALID, "map range [%u,%u) outside [0,%d]", map_lo, map_hi, h->map_count);
    HIPC(hipSetDevice(h->device));
    if (len < (uint64_t)h->k) return KQ_OK;                                  // src/kreeq.cpp:123
    const uint8_t* ab; uint64_t lead;
    aligned_view(d_bases, &ab, &lead);
    const uint32_t map_mask = (h->map_count & (h->map_count - 1)) == 0 ? (uint32_t)h->map_count - 1 : 0;
    { int frc = flush_pending(h); if (frc) return frc; }
    materialize(h);
    // the partitioned path (lookup_partitions): regions staged in LDS instead of one random sector per k-mer
    const uint64_t kmers = len - h->k + 1;
    if (lookup_partitions(d_per_base != nullptr, h->lookup_path, part_table_ok(h->shape(), true), kmers, h->slice_kmers, h->table_bytes())) {
        for (uint64_t a = 0; a < kmers; a += h->slice_kmers) {
            const uint64_t b = std::min(kmers, a + h->slice_kmers);
            const SliceView v = slice_view(d_bases, nullptr, len, h->k, a, b);
            int rc = lookup_partitioned(h, v.ab, v.lead, v.len, v.er, cov_cutoff, map_lo, map_hi, (unsigned long long*)d_counters);
            if (rc) return rc;
        }
        return KQ_OK;
    }
    const dim3 grid(grid_for(h, n_tiles_of(lead, len), 1, 32));
    if (d_per_base) hipLaunchKernelGGL(k_lookup<true>, grid, dim3(TILE_THREADS), 0, h->stream, h->view(), ab, lead, len, h->k, (uint32_t)h->map_count,
                                       map_mask, (uint32_t)map_lo, (uint32_t)map_hi, cov_cutoff, d_per_base, (unsigned long long*)d_counters);
    else hipLaunchKernelGGL(k_lookup<false>, grid, dim3(TILE_THREADS), 0, h->stream, h->view(), ab, lead, len, h->k, (uint32_t)h->map_count,
                            map_mask, (uint32_t)map_lo, (uint32_t)map_hi, cov_cutoff, d_per_base, (unsigned long long*)d_counters);
    HIPC(hipGetLastError());
    return KQ_OK;
}
int kq_lookup_sequence(kq_handle* h, const char* bases, uint64_t len, uint32_t cov_cutoff, uint16_t map_lo, uint16_t map_hi,
                       kq_dbgbase* per_base, uint64_t counters[3]) {
    if (!h || !counters || (!bases && len)) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    int rc = check_errors(h);
    if (rc) return rc;
    void* d = nullptr;
    rc = stage_in(h, bases, len, &d);
    if (rc) return rc;
    DevScope mem;
    unsigned long long* d_ctr = nullptr;
    kq_dbgbase* d_pb = nullptr;
    HIPC(mem.alloc((void**)&d_ctr, 3 * sizeof(unsigned long long)));
    (void)hipMemsetAsync(d_ctr, 0, 3 * sizeof(unsigned long long), h->stream);
    if (per_base && len) {
        if (mem.alloc((void**)&d_pb, len * sizeof(kq_dbgbase)) != hipSuccess) return fail(KQ_ERR_NOMEM, "per-base buffer allocation failed");
        (void)hipMemcpyAsync(d_pb, per_base, len * sizeof(kq_dbgbase), hipMemcpyHostToDevice, h->stream);
    }
    rc = kq_lookup_sequence_dev(h, (const char*)d, len, cov_cutoff, map_lo, map_hi, d_pb, (uint64_t*)d_ctr);
    unsigned long long c[3] = {0, 0, 0};
    if (!rc) {
        hipError_t e1 = hipMemcpyAsync(c, d_ctr, sizeof c, hipMemcpyDeviceToHost, h->stream);
        hipError_t e2 = d_pb ? hipMemcpyAsync(per_base, d_pb, len * sizeof(kq_dbgbase), hipMemcpyDeviceToHost, h->stream) : hipSuccess;
        hipError_t e3 = hipStreamSynchronize(h->stream);
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) rc = fail(KQ_ERR_HIP, "lookup failed: %s", hipGetErrorString(e3));
    }
    if (!rc) for (int i = 0; i < 3; ++i) counters[i] += c[i];
    return rc;
}

// ---- per-base tables: device memory for the CLI, triples, text ---------------------------------------------------------
void* kq_dev_alloc(kq_handle* h, uint64_t bytes) {
    if (!h || hipSetDevice(h->device) != hipSuccess) return nullptr;
    DevMem m;
    if (m.alloc(bytes ? (size_t)bytes : 8) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipMemsetAsync(m.get(), 0, m.bytes(), h->stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }      // (what kq_lookup_sequence_dev asks of a per-base array)
    h->user_mem.push_back(std::move(m));
    return h->user_mem.back().get();
}
void kq_dev_free(kq_handle* h, void* p) {
    if (!h || !p) return;
    (void)hipSetDevice(h->device);
    for (size_t i = 0; i < h->user_mem.size(); ++i)
        if (h->user_mem[i].get() == p) { h->user_mem.erase(h->user_mem.begin() + (ptrdiff_t)i); return; }
}
int kq_copy_async(kq_handle* h, void* dst, const void* src, uint64_t bytes, int kind) {
    if (!h || ((!dst || !src) && bytes)) return fail(KQ_ERR_INVALID, "null argument");
    if (kind != KQ_COPY_TO_DEVICE && kind != KQ_COPY_TO_HOST) return fail(KQ_ERR_INVALID, "unknown copy kind %d", kind);
    HIPC(hipSetDevice(h->device));
    if (bytes) HIPC(hipMemcpyAsync(dst, src, (size_t)bytes, kind == KQ_COPY_TO_DEVICE ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, h->stream));
    return KQ_OK;
}

int kq_per_base_triples_dev(kq_handle* h, const kq_dbgbase* d_per_base, const uint64_t* seg_start, const uint64_t* seg_len, uint64_t n_segs, uint32_t* d_triples) {
    if (!h || ((!seg_start || !seg_len) && n_segs)) return fail(KQ_ERR_INVALID, "null argument");
    if (n_segs >= 0xFFFFFFFFull) return fail(KQ_ERR_INVALID, "%llu segments: fewer than 2^32 - 1 per call", (unsigned long long)n_segs);
    std::vector<unsigned long long> lists(2 * (size_t)n_segs + 1);          // seg_start[n_segs], out_start[n_segs + 1]
    unsigned long long total = 0;
    for (uint64_t s = 0; s < n_segs; ++s) { lists[s] = seg_start[s]; lists[n_segs + s] = total; total += seg_len[s]; }
    lists[2 * n_segs] = total;
    if (!total) return KQ_OK;
    if (!d_per_base || !d_triples) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    HIPC(h->tab_segs.ensure(lists.size() * 8));                          // (frees the previous lists only after the device has finished with them)
    unsigned long long* d_lists = h->tab_segs.as<unsigned long long>();
    HIPC(hipMemcpyAsync(d_lists, lists.data(), lists.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIPC(hipStreamSynchronize(h->stream));                                // `lists` is pageable and leaves scope
    hipLaunchKernelGGL(k_tab_triples, dim3(grid_for(h, total, 256)), dim3(256), 0, h->stream, d_per_base, (const unsigned long long*)d_lists,
                       (const unsigned long long*)(d_lists + n_segs), (uint32_t)n_segs, (uint64_t)total, d_triples);
    HIPC(hipGetLastError());
    return KQ_OK;
}

int kq_per_base_merge_dev(kq_handle* h, kq_dbgbase* d_per_base, const uint64_t* seg_start, const uint64_t* seg_len, uint64_t n_segs, uint32_t* d_triples) {
    if (!h || ((!seg_start || !seg_len) && n_segs)) return fail(KQ_ERR_INVALID, "null argument");
    if (n_segs >= 0xFFFFFFFFull) return fail(KQ_ERR_INVALID, "%llu segments: fewer than 2^32 - 1 per call", (unsigned long long)n_segs);
    std::vector<unsigned long long> lists(2 * (size_t)n_segs + 1);          // seg_start[n_segs], out_start[n_segs + 1]
    unsigned long long total = 0, end = 0;                                  // end: behind the entries of the segments so far
    for (uint64_t s = 0; s < n_segs; ++s) {
        if (seg_start[s] < end || seg_len[s] > ~0ull - seg_start[s])         // (two threads would consume one entry)
            return fail(KQ_ERR_INVALID, "segment %llu (%llu + %llu) is not behind the one before it", (unsigned long long)s, (unsigned long long)seg_start[s], (unsigned long long)seg_len[s]);
        end = seg_start[s] + seg_len[s];
        lists[s] = seg_start[s]; lists[n_segs + s] = total; total += seg_len[s];
    }
    lists[2 * n_segs] = total;
    if (!total) return KQ_OK;
    if (!d_per_base || !d_triples) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    HIPC(h->tab_segs.ensure(lists.size() * 8));                          // (frees the previous lists only after the device has finished with them)
    unsigned long long* d_lists = h->tab_segs.as<unsigned long long>();
    HIPC(hipMemcpyAsync(d_lists, lists.data(), lists.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIPC(hipStreamSynchronize(h->stream));                                // `lists` is pageable and leaves scope
    hipLaunchKernelGGL(k_tab_merge, dim3(grid_for(h, total, 256)), dim3(256), 0, h->stream, d_per_base, (const unsigned long long*)d_lists,
                       (const unsigned long long*)(d_lists + n_segs), (uint32_t)n_segs, (uint64_t)total, d_triples);
    HIPC(hipGetLastError());
    return KQ_OK;
}

// the checks of kq_format_table*, and the lines before every piece
static int tab_check(kq_handle* h, int format, const void* triples, uint64_t n_triples, const kq_table_seg* segs, uint64_t n_segs, const char* names, uint64_t names_len,
                     uint64_t* n_out, std::vector<unsigned long long>* line_start) {
    if (!h || !n_out || (!segs && n_segs) || (!triples && n_triples) || (!names && names_len)) return fail(KQ_ERR_INVALID, "null argument");
    if (format != KQ_TABLE_KWIG && format != KQ_TABLE_BED && format != KQ_TABLE_CSV) return fail(KQ_ERR_INVALID, "unknown table format %d", format);
    if (n_segs >= 0xFFFFFFFFull) return fail(KQ_ERR_INVALID, "%llu pieces: format fewer than 2^32 lines per call", (unsigned long long)n_segs);
    line_start->assign((size_t)n_segs + 1, 0);
    unsigned long long lines = 0;
    for (uint64_t p = 0; p < n_segs; ++p) {
        const kq_table_seg& s = segs[p];
        if (s.n_ctx > (uint32_t)(h->k - 1) || s.n_ctx > s.first) return fail(KQ_ERR_INVALID, "piece %llu: n_ctx %u exceeds k - 1 = %d or its first triple %llu", (unsigned long long)p, s.n_ctx, h->k - 1, (unsigned long long)s.first);
        if (s.first > n_triples || s.n > n_triples - s.first) return fail(KQ_ERR_INVALID, "piece %llu runs past the %llu triples", (unsigned long long)p, (unsigned long long)n_triples);
        if (s.name_len > TAB_MAX_NAME || s.name_off > names_len || s.name_len > names_len - s.name_off) return fail(KQ_ERR_INVALID, "piece %llu: its name lies outside the names (or is longer than %u bytes)", (unsigned long long)p, TAB_MAX_NAME);
        (*line_start)[p] = lines;
        lines += s.n + ((format == KQ_TABLE_KWIG && (s.flags & KQ_TABLE_SEG_HEADER)) ? 1 : 0);
        if (lines >= (1ull << 32)) return fail(KQ_ERR_INVALID, "2^32 lines or more in one call: format in smaller calls");
    }
    (*line_start)[n_segs] = lines;
    return KQ_OK;
}
// d_triples on the device; `out` on the device (out_on_host false) or on the host
static int tab_format(kq_handle* h, int format, const uint32_t* d_triples, const kq_table_seg* segs, uint64_t n_segs, const char* names, uint64_t names_len,
                      const std::vector<unsigned long long>& line_start, char* out, bool out_on_host, uint64_t cap, uint64_t* n_out) {
    *n_out = 0;
    const uint64_t n_lines = line_start[n_segs];
    if (!n_lines) return KQ_OK;
    hipStream_t st = h->stream;
    const uint64_t n_tiles = (n_lines + TAB_TILE - 1) / TAB_TILE, n_chunks = (n_tiles + SCAN_CHUNK - 1) / SCAN_CHUNK;
    DevScope mem;
    kq_table_seg* d_segs = nullptr;
    unsigned long long *d_ls = nullptr, *d_tile = nullptr, *d_sums = nullptr;
    char* d_names = nullptr;
    if (mem.alloc((void**)&d_segs, n_segs * sizeof(kq_table_seg)) != hipSuccess || mem.alloc((void**)&d_ls, (n_segs + 1) * 8) != hipSuccess ||
        mem.alloc((void**)&d_names, names_len) != hipSuccess || mem.alloc((void**)&d_tile, n_tiles * 8) != hipSuccess || mem.alloc((void**)&d_sums, (n_chunks + 2) * 8) != hipSuccess)
        return fail(KQ_ERR_NOMEM, "no device memory for the placement of %llu lines", (unsigned long long)n_lines);
    unsigned long long* d_total = d_sums + n_chunks + 1;
    HIPC(hipMemcpyAsync(d_segs, segs, n_segs * sizeof(kq_table_seg), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_ls, line_start.data(), (n_segs + 1) * 8, hipMemcpyHostToDevice, st));
    if (names_len) HIPC(hipMemcpyAsync(d_names, names, names_len, hipMemcpyHostToDevice, st));
    const TabArgs a{d_triples, d_segs, d_ls, d_names, n_lines, (uint32_t)n_segs, format, h->k};
    const dim3 grid(grid_for(h, n_tiles, 1, 8));
    // 1. line lengths -> bytes per tile, 2. tile offsets and the size
    hipLaunchKernelGGL(k_tab_len, grid, dim3(TAB_THREADS), 0, st, a, d_tile);
    scan_u64(h, d_tile, n_tiles, d_sums, d_total);
    HIPC(hipGetLastError());
    unsigned long long total = 0;
    HIPC(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    *n_out = total;
    if (!out) return KQ_OK;
    if (total > cap) return fail(KQ_ERR_CAPACITY, "the table text takes %llu bytes: the buffer holds %llu", total, (unsigned long long)cap);
    // 3. the text
    char* d_out = out;
    if (out_on_host && mem.alloc((void**)&d_out, total) != hipSuccess) return fail(KQ_ERR_NOMEM, "no device memory for %llu bytes of table text", total);
    hipLaunchKernelGGL(k_tab_write, grid, dim3(TAB_THREADS), 0, st, a, (const unsigned long long*)d_tile, (uint64_t)total, d_out);
    HIPC(hipGetLastError());
    if (out_on_host) HIPC(hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return KQ_OK;
}
int kq_format_table_dev(kq_handle* h, int format, const uint32_t* d_triples, uint64_t n_triples, const kq_table_seg* segs, uint64_t n_segs, const char* names,
                        uint64_t names_len, char* d_out, uint64_t cap, uint64_t* n_out) {
    std::vector<unsigned long long> line_start;
    int rc = tab_check(h, format, d_triples, n_triples, segs, n_segs, names, names_len, n_out, &line_start);
    if (rc) return rc;
    HIPC(hipSetDevice(h->device));
    return tab_format(h, format, d_triples, segs, n_segs, names, names_len, line_start, d_out, false, cap, n_out);
}
int kq_format_table(kq_handle* h, int format, const uint32_t* triples, uint64_t n_triples, const kq_table_seg* segs, uint64_t n_segs, const char* names,
                    uint64_t names_len, char* out, uint64_t cap, uint64_t* n_out) {
    std::vector<unsigned long long> line_start;
    int rc = tab_check(h, format, triples, n_triples, segs, n_segs, names, names_len, n_out, &line_start);
    if (rc) return rc;
    HIPC(hipSetDevice(h->device));
    void* d = nullptr;
    rc = stage_in(h, triples, (size_t)n_triples * 12, &d);
    if (rc) return rc;
    return tab_format(h, format, (const uint32_t*)d, segs, n_segs, names, names_len, line_start, out, true, cap, n_out);
}

// ---- candidate-error search support ---------------------------------------------------------------
int kq_lookup_keys(kq_handle* h, const uint64_t* keys, uint64_t n, kq_entry* out) {
    if (!h || ((!keys || !out) && n)) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    if (!n) return KQ_OK;
    int rc = flush_pending(h);
    if (rc) return rc;
    materialize(h);
    // keys in, entries out: one scratch buffer (8 + 48 bytes per key)
    HIPC(h->stage.ensure((size_t)n * (sizeof(uint64_t) + sizeof(kq_entry)) + 64));
    uint64_t* d_keys = h->stage.as<uint64_t>();
    kq_entry* d_out = (kq_entry*)(d_keys + ((n + 1) & ~1ull));
    HIPC(hipMemcpyAsync(d_keys, keys, n * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_lookup_keys, dim3(grid_for(h, n, 256)), dim3(256), 0, h->stream, h->view(), d_keys, n, d_out);
    HIPC(hipMemcpyAsync(out, d_out, n * sizeof(kq_entry), hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    return KQ_OK;
}
int kq_branch_scan(kq_handle* h, const char* bases, uint64_t len, uint32_t cov_cutoff, uint8_t* flags) {
    if (!h || ((!bases || !flags) && len)) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    if (len) memset(flags, 0, len);
    if (len < (uint64_t)h->k) return KQ_OK;
    int rc = flush_pending(h);
    if (rc) return rc;
    materialize(h);
    void* d = nullptr;
    rc = stage_in(h, bases, len, &d);
    if (rc) return rc;
    DevScope mem;
    uint8_t* d_flags = nullptr;
    HIPC(mem.alloc((void**)&d_flags, len));
    (void)hipMemsetAsync(d_flags, 0, len, h->stream);
    const uint8_t* ab; uint64_t lead;
    aligned_view((const char*)d, &ab, &lead);
    hipLaunchKernelGGL(k_branch_scan, dim3(grid_for(h, n_tiles_of(lead, len), 1, 32)), dim3(TILE_THREADS), 0, h->stream, h->view(), ab, lead, len, h->k,
                       cov_cutoff, d_flags);
    hipError_t e1 = hipMemcpyAsync(flags, d_flags, len, hipMemcpyDeviceToHost, h->stream);
    hipError_t e2 = hipStreamSynchronize(h->stream);
    if (e1 != hipSuccess || e2 != hipSuccess) return fail(KQ_ERR_HIP, "branch scan failed: %s", hipGetErrorString(e2 != hipSuccess ? e2 : e1));
    return KQ_OK;
}


// Scratch budget of the candidate-error searches: every search of a batch owns one state block of kqvar::block_bytes(depth,
// max_span) bytes (2.8 KB at depth 15 / span 32, 7.8 KB at depth 60 / span 20, 34.7 KB at the limits), so a batch is
// VAR_ARENA_BYTES / block bytes searches (at least one, at most the flagged positions there are).  KQ_OPT_VARIANT_BATCH fixes
// the number instead (tests).
constexpr uint64_t VAR_ARENA_BYTES = 1ull << 30;

// the ascending list of the i < len with word[i] != 0, through an exclusive prefix sum into rank -> *out (mem owns it), *n_out
static int var_compact(kq_handle* h, DevScope& mem, const uint32_t* d_word, uint32_t* d_rank, uint64_t len, void* d_tmp, size_t tmp_bytes, uint32_t** out, uint64_t* n_out) {
    hipStream_t st = h->stream;
    HIPC(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_word, d_rank, (int64_t)len, st));
    uint32_t last[2] = {0, 0};
    HIPC(hipMemcpyAsync(&last[0], d_word + (len - 1), 4, hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(&last[1], d_rank + (len - 1), 4, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    *n_out = (uint64_t)last[0] + last[1];
    if (mem.alloc((void**)out, (*n_out + 1) * 4) != hipSuccess) return fail(KQ_ERR_NOMEM, "no device memory for a list of %llu positions", (unsigned long long)*n_out);
    if (*n_out) hipLaunchKernelGGL(k_var_scatter, dim3(grid_for(h, len, 256)), dim3(256), 0, st, d_word, (const uint32_t*)d_rank, len, *out, *n_out);
    HIPC(hipGetLastError());
    return KQ_OK;
}

int kq_search_variants(kq_handle* h, const char* bases, uint64_t len, int depth, int max_span, uint32_t cov_cutoff, kq_variant_path* paths, uint64_t path_cap,
                       uint64_t* n_paths, char* seq, uint64_t seq_cap, uint64_t* n_seq) {
    if (!h || (!bases && len) || !n_paths || !n_seq) return fail(KQ_ERR_INVALID, "null argument");
    if (h->windowed) return fail(KQ_ERR_INVALID, "kq_search_variants does not take a windowed handle (KQ_OPT_BUCKET_WINDOW / KQ_OPT_SHARD_WINDOW)");
    if (depth < 0 || depth > kqvar::MAX_DEPTH) return fail(KQ_ERR_INVALID, "search depth %d outside 0..%d", depth, kqvar::MAX_DEPTH);
    if (max_span < 0 || max_span > kqvar::MAX_SPAN) return fail(KQ_ERR_INVALID, "max span %d outside 0..%d", max_span, kqvar::MAX_SPAN);
    if (len >= 0xFFFFFFFFull) return fail(KQ_ERR_INVALID, "sequence batch of %llu bytes: search in batches below 2^32 - 1 bytes", (unsigned long long)len);
    *n_paths = 0; *n_seq = 0;
    HIPC(hipSetDevice(h->device));
    if (len < (uint64_t)h->k) return KQ_OK;
    int rc = flush_pending(h);
    if (rc) return rc;
    materialize(h);
    void* d = nullptr;
    rc = stage_in(h, bases, len, &d);
    if (rc) return rc;
    hipStream_t st = h->stream;
    const uint8_t* d_text = (const uint8_t*)d;
    const bool want_out = paths && seq;
    DevScope mem;
    // 1. the pre-filter, 2. the position list and the breaks
    uint8_t* d_flags = nullptr;
    uint32_t *d_word = nullptr, *d_rank = nullptr, *d_pos = nullptr, *d_breaks = nullptr;
    void* d_tmp = nullptr;
    size_t tmp_bytes = 0, tmp_bytes64 = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_word, d_rank, (int64_t)len, st) != hipSuccess) return fail(KQ_ERR_HIP, "position scan setup failed");
    if (mem.alloc((void**)&d_flags, len) != hipSuccess || mem.alloc((void**)&d_word, len * 4) != hipSuccess || mem.alloc((void**)&d_rank, len * 4) != hipSuccess ||
        mem.alloc(&d_tmp, tmp_bytes) != hipSuccess)
        return fail(KQ_ERR_NOMEM, "no device memory for the position scratch of %llu bases", (unsigned long long)len);
    HIPC(hipMemsetAsync(d_flags, 0, len, st));
    const uint8_t* ab; uint64_t lead;
    aligned_view((const char*)d, &ab, &lead);
    hipLaunchKernelGGL(k_branch_scan, dim3(grid_for(h, n_tiles_of(lead, len), 1, 32)), dim3(TILE_THREADS), 0, st, h->view(), ab, lead, len, h->k, cov_cutoff, d_flags);
    hipLaunchKernelGGL(k_var_flag, dim3(grid_for(h, len, 256)), dim3(256), 0, st, (const uint8_t*)d_flags, len, d_word);
    HIPC(hipGetLastError());
    uint64_t n_pos = 0, n_breaks = 0;
    rc = var_compact(h, mem, d_word, d_rank, len, d_tmp, tmp_bytes, &d_pos, &n_pos);
    if (rc) return rc;
    if (!n_pos) return KQ_OK;
    hipLaunchKernelGGL(k_sg_invalid, dim3(grid_for(h, len, 256)), dim3(256), 0, st, d_text, len, d_word);
    rc = var_compact(h, mem, d_word, d_rank, len, d_tmp, tmp_bytes, &d_breaks, &n_breaks);
    if (rc) return rc;
    HIPC(hipStreamSynchronize(st));                                  // the scatter above reads what is released here
    mem.release(d_flags); mem.release(d_word); mem.release(d_rank); mem.release(d_tmp);
    d_tmp = nullptr;
    // 3. the searches, batch by batch
    const uint64_t block_bytes = kqvar::block_bytes(depth, max_span);
    const uint64_t batch = std::min<uint64_t>(n_pos, h->var_batch ? h->var_batch : std::max<uint64_t>(1, VAR_ARENA_BYTES / block_bytes));
    // no result is larger than this, whatever the caller offers
    const uint64_t most_paths = n_pos * kqvar::dest_bound(depth), most_seq = most_paths * (uint64_t)std::max(std::max(max_span, depth + 1), 1);
    const uint64_t cap_paths = std::min(path_cap, most_paths), cap_seq = std::min(seq_cap, most_seq);
    uint8_t* d_arena = nullptr;
    unsigned long long *d_cnt = nullptr, *d_off = nullptr;               // [0, batch): paths, [batch, 2 batch): sequence bytes
    VarState* d_state = nullptr;
    kq_variant_path* d_paths = nullptr;
    char* d_seq = nullptr;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes64, d_cnt, d_off, (int64_t)batch, st) != hipSuccess) return fail(KQ_ERR_HIP, "offset scan setup failed");
    if (mem.alloc((void**)&d_state, sizeof(VarState)) != hipSuccess || mem.alloc((void**)&d_cnt, 2 * batch * 8) != hipSuccess || mem.alloc((void**)&d_off, 2 * batch * 8) != hipSuccess ||
        mem.alloc(&d_tmp, tmp_bytes64) != hipSuccess)
        return fail(KQ_ERR_NOMEM, "no device memory");
    if (mem.alloc((void**)&d_arena, batch * block_bytes) != hipSuccess)
        return fail(KQ_ERR_NOMEM, "no device memory for the state blocks of %llu searches of depth %d, span %d", (unsigned long long)batch, depth, max_span);
    if (want_out && (mem.alloc((void**)&d_paths, cap_paths * sizeof(kq_variant_path)) != hipSuccess || mem.alloc((void**)&d_seq, cap_seq) != hipSuccess))
        return fail(KQ_ERR_NOMEM, "no device memory for %llu paths and %llu sequence bytes", (unsigned long long)cap_paths, (unsigned long long)cap_seq);
    uint64_t tot_paths = 0, tot_seq = 0;
    bool emit = want_out;                                                // until the totals pass a cap: then the rest is only counted
    VarState state{};
    for (uint64_t lo = 0; lo < n_pos; lo += batch) {
        const uint64_t n = std::min(batch, n_pos - lo);
        HIPC(hipMemsetAsync(d_arena, 0xFF, n * block_bytes, st));       // the node indexes: every slot free (the rest of a block is written before it is read)
        HIPC(hipMemsetAsync(d_state, 0, sizeof(VarState), st));
        hipLaunchKernelGGL(k_var_search, dim3(grid_for(h, n, 256)), dim3(256), 0, st, h->view(), d_text, len, (const uint32_t*)(d_pos + lo), n, (const uint32_t*)d_breaks,
                           (uint32_t)n_breaks, depth, max_span, cov_cutoff, d_arena, block_bytes, d_cnt, d_cnt + batch, d_state);
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(&state, d_state, sizeof state, hipMemcpyDeviceToHost, st));      // only the batch's totals and the error mask return to the host
        HIPC(hipStreamSynchronize(st));
        if (state.err) return fail(KQ_ERR_HIP, "candidate-error search: a search left its state block's bounds (error mask %u)", state.err);      // cannot happen: kq_variant_core.h
        const uint64_t base_paths = tot_paths, base_seq = tot_seq;
        tot_paths += state.n_paths; tot_seq += state.n_seq;
        if (tot_paths > cap_paths || tot_seq > cap_seq) emit = false;
        if (!emit || !state.n_paths) continue;
        // 4. where every search of the batch writes, then the records and bases themselves
        HIPC(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes64, d_cnt, d_off, (int64_t)n, st));
        HIPC(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes64, d_cnt + batch, d_off + batch, (int64_t)n, st));
        hipLaunchKernelGGL(k_var_emit, dim3(grid_for(h, n, 256)), dim3(256), 0, st, h->view(), d_text, len, (const uint32_t*)(d_pos + lo), n, (const uint32_t*)d_breaks,
                           (uint32_t)n_breaks, depth, max_span, d_arena, block_bytes, (const unsigned long long*)d_off, (const unsigned long long*)(d_off + batch), base_paths,
                           base_seq, d_paths, cap_paths, d_seq, cap_seq, d_state);
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(&state, d_state, sizeof state, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        if (state.err) return fail(KQ_ERR_HIP, "candidate-error search: a path left its bounds (error mask %u)", state.err);      // cannot happen: the totals fit
    }
    *n_paths = tot_paths; *n_seq = tot_seq;
    if (!want_out) return KQ_OK;
    if (tot_paths > path_cap || tot_seq > seq_cap)
        return fail(KQ_ERR_CAPACITY, "%llu paths with %llu sequence bytes: the buffers hold %llu and %llu", (unsigned long long)tot_paths, (unsigned long long)tot_seq,
                    (unsigned long long)path_cap, (unsigned long long)seq_cap);
    // 5. copy out
    hipError_t e1 = tot_paths ? hipMemcpyAsync(paths, d_paths, tot_paths * sizeof(kq_variant_path), hipMemcpyDeviceToHost, st) : hipSuccess;
    hipError_t e2 = tot_seq ? hipMemcpyAsync(seq, d_seq, tot_seq, hipMemcpyDeviceToHost, st) : hipSuccess;
    hipError_t e3 = hipStreamSynchronize(st);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return fail(KQ_ERR_HIP, "candidate-error search: copy out failed: %s", hipGetErrorString(e3 != hipSuccess ? e3 : e1 != hipSuccess ? e1 : e2));
    return KQ_OK;
}

// ---- union / import / export ---------------------------------------------------------------------
int kq_merge(kq_handle* dst, kq_handle* src) {
    if (!dst || !src) return fail(KQ_ERR_INVALID, "null handle");
    if (dst == src) return fail(KQ_ERR_INVALID, "cannot merge a handle into itself");
    if (dst->k != src->k || dst->map_count != src->map_count || dst->device != src->device)
        return fail(KQ_ERR_MISMATCH, "handles differ in k / map_count / device");    // src/input.cpp:136-139
    HIPC(hipSetDevice(dst->device));
    { int frc = flush_pending(dst); if (frc) return frc; }
    { int frc = flush_pending(src); if (frc) return frc; }
    materialize(src);                                   // on src's stream, before the sync below
    int rc = kq_sync(src);
    if (rc) return rc;
    rc = read_state(src);
    if (rc) return rc;
    rc = reserve(dst, src->host_state()->slots_used, src->host_state()->kmers_added);
    if (rc) return rc;
    // enough source entries to pay for streaming dst once: merge region by region in LDS; else per-entry atomics
    if (dst->merge_path == 2 || (dst->merge_path == 0 && src->host_state()->slots_used * 64 >= dst->n_slots())) {
        const int empty = (dst->table_empty || dst->slots_dirty) ? 1 : 0;     // a dirty (lazily cleared) array is never read
        hipLaunchKernelGGL(k_merge_regions, dim3((unsigned)std::min<uint64_t>(dst->n_alloc_regions(), 1u << 30)), dim3(P3_THREADS), 0, dst->stream,
                           dst->view(), src->view(), empty);
        dst->slots_dirty = false;                       // every region image has been written
        dst->table_empty = false;
        HIPC(hipGetLastError());
        return kq_sync(dst);
    }
    materialize(dst);
    dst->table_empty = false;
    hipLaunchKernelGGL(k_merge, dim3(grid_for(dst, src->n_slots(), 256)), dim3(256), 0, dst->stream, dst->view(), src->view());
    HIPC(hipGetLastError());
    return kq_sync(dst);
}

int kq_import(kq_handle* h, const kq_entry* entries, uint64_t n) {
    if (!h || (!entries && n)) return fail(KQ_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(h->device));
    if (!n) return KQ_OK;
    uint64_t inst = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const kq_entry& e = entries[i];
        inst += e.cov;
        bool ok = e.cov > 0 && e.key != EMPTY_KEY;
        for (int w = 0; w < 4; ++w) ok = ok && e.fw[w] <= e.cov && e.bw[w] <= e.cov;   // an edge is seen at most once per instance
        if (!ok) return fail(KQ_ERR_INVALID, "entry %llu is not a valid k-mer record (cov 0, or an edge counter above cov)",
                             (unsigned long long)i);
    }
    int rc = reserve(h, n, inst);
    if (rc) return rc;
    void* d = nullptr;
    rc = stage_in(h, entries, n * sizeof(kq_entry), &d);
    if (rc) return rc;
    materialize(h);
    h->table_empty = false;
    hipLaunchKernelGGL(k_import, dim3(grid_for(h, n, 256)), dim3(256), 0, h->stream, h->view(), (const kq_entry*)d, n);
    HIPC(hipGetLastError());
    return kq_sync(h);
}

// key order on the device: radix sort of (key, index) + gather into a fresh array (*d_sorted, which stays in the caller's `mem`;
// the temporaries are released before the return).  false, and nothing kept, when there is no memory for it (or n >= 2^32)
static bool sort_entries_dev(kq_handle* h, DevScope& mem, const kq_entry* d_in, uint64_t n, kq_entry** d_sorted_out) {
    kq_entry* d_sorted = nullptr; uint64_t *d_k1 = nullptr, *d_k2 = nullptr; uint32_t *d_i1 = nullptr, *d_i2 = nullptr; void* d_tmp = nullptr;
    size_t tmp_bytes = 0;
    bool on_device = n < (1ull << 32) && !(h->test_export & 1) &&
        hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, d_k1, d_k2, d_i1, d_i2, (int64_t)n, 0, 2 * h->k, h->stream) == hipSuccess &&
        mem.alloc((void**)&d_sorted, n * sizeof(kq_entry)) == hipSuccess && mem.alloc((void**)&d_k1, n * 8) == hipSuccess &&
        mem.alloc((void**)&d_k2, n * 8) == hipSuccess && mem.alloc((void**)&d_i1, n * 4) == hipSuccess &&
        mem.alloc((void**)&d_i2, n * 4) == hipSuccess && mem.alloc(&d_tmp, tmp_bytes) == hipSuccess;
    if (on_device) {
        hipLaunchKernelGGL(k_entry_keys, dim3(grid_for(h, n, 256)), dim3(256), 0, h->stream, d_in, n, d_k1, d_i1);
        on_device = hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, d_k1, d_k2, d_i1, d_i2, (int64_t)n, 0, 2 * h->k, h->stream) == hipSuccess;
        if (on_device) {
            hipLaunchKernelGGL(k_entry_gather, dim3(grid_for(h, n, 256)), dim3(256), 0, h->stream, d_in, d_i2, n, d_sorted);
            on_device = hipStreamSynchronize(h->stream) == hipSuccess;
        }
    }
    if (!on_device) (void)hipGetLastError();
    for (void* q : {(void*)d_k1, (void*)d_k2, (void*)d_i1, (void*)d_i2, d_tmp, on_device ? nullptr : (void*)d_sorted}) mem.release(q);
    *d_sorted_out = on_device ? d_sorted : nullptr;
    return on_device;
}
// device -> caller: through two pinned bounce buffers (a copy into pageable memory runs at a fraction of the PCIe
// rate: 0.25 s for 850 MB); the DMA of chunk i+1 overlaps the host copy of chunk i
static hipError_t copy_out_bounced(kq_handle* h, void* out, const void* src, size_t bytes) {
    const bool test_chunks = (h->test_export & 2) != 0;
    const BouncePlan p = bounce_plan(bytes, test_chunks ? EXPORT_TEST_CHUNK : EXPORT_CHUNK, test_chunks);
    PinnedMem bounce[2];
    if (p.bounced && bounce[0].alloc(p.chunk) == hipSuccess && bounce[1].alloc(p.chunk) == hipSuccess)
        return bounce_copy(p, hipSuccess,
            [&](int b, size_t off, size_t len) { return hipMemcpyAsync(bounce[b].get(), (const char*)src + off, len, hipMemcpyDeviceToHost, h->stream); },
            [&]() { return hipStreamSynchronize(h->stream); },
            [&](size_t off, int b, size_t len) { memcpy((char*)out + off, bounce[b].get(), len); });
    (void)hipGetLastError();
    return hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost);
}

int kq_export(kq_handle* h, uint16_t map_lo, uint16_t map_hi, kq_entry* out, uint64_t cap, uint64_t* n_out) {
    if (!h || !n_out) return fail(KQ_ERR_INVALID, "null argument");
    if (map_lo > map_hi || map_hi > h->map_count) return fail(KQ_ERR_INVALID, "map range [%u,%u) outside [0,%d]", map_lo, map_hi, h->map_count);
    HIPC(hipSetDevice(h->device));
    int rc = check_errors(h);
    if (rc) return rc;
    DevScope mem;
    unsigned long long* d_n = nullptr;
    kq_entry* d_out = nullptr;
    HIPC(mem.alloc((void**)&d_n, sizeof(unsigned long long)));
    (void)hipMemsetAsync(d_n, 0, sizeof(unsigned long long), h->stream);
    if (out && cap) {
        if (mem.alloc((void**)&d_out, cap * sizeof(kq_entry)) != hipSuccess) return fail(KQ_ERR_NOMEM, "export buffer allocation failed");
    }
    materialize(h);
    hipLaunchKernelGGL(k_export, dim3(grid_for(h, h->n_slots(), 1024)), dim3(256), 0, h->stream, h->view(), (uint32_t)h->map_count,
                       (uint32_t)map_lo, (uint32_t)map_hi, d_out, d_out ? cap : 0, d_n);
    unsigned long long n = 0;
    hipError_t e = hipMemcpyAsync(&n, d_n, sizeof n, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) rc = fail(KQ_ERR_HIP, "export failed: %s", hipGetErrorString(e));
    *n_out = n;
    if (!rc && out) {
        if (n > cap) rc = fail(KQ_ERR_CAPACITY, "export buffer too small: need %llu, have %llu", n, (unsigned long long)cap);
        else if (n) {
            // key order on the device when there is memory for it, else on the host
            kq_entry* d_sorted = nullptr;
            const bool on_device = sort_entries_dev(h, mem, d_out, n, &d_sorted);
            e = copy_out_bounced(h, out, on_device ? d_sorted : d_out, (size_t)n * sizeof(kq_entry));
            if (e != hipSuccess) rc = fail(KQ_ERR_HIP, "export copy failed: %s", hipGetErrorString(e));
            else if (!on_device) parallel_sort_entries(out, n);
        }
    }
    return rc;
}

// ---- database map files as device-built / device-parsed images (kq_dbimage.h) -----------------------------------------
int kq_export_map_images(kq_handle* h, uint16_t map_lo, uint16_t map_hi, void* out, uint64_t cap, uint64_t* offsets,
                         kq_entry* hc_out, uint64_t hc_cap, uint64_t* n_hc) {
    if (!offsets || !n_hc) return fail(KQ_ERR_INVALID, "null offsets / n_hc");
    if (map_lo > map_hi) return fail(KQ_ERR_INVALID, "map range [%u,%u) is reversed", map_lo, map_hi);
    if (!h) return fail(KQ_ERR_INVALID, "null handle");
    if (map_hi > h->map_count) return fail(KQ_ERR_INVALID, "map range [%u,%u) outside [0,%d]", map_lo, map_hi, h->map_count);
    const uint32_t n_maps = (uint32_t)(map_hi - map_lo), n_sub = n_maps * DBI_SUBMAPS;
    offsets[0] = 0; *n_hc = 0;
    if (!n_maps) return KQ_OK;
    HIPC(hipSetDevice(h->device));
    int rc = check_errors(h);          // flushes pending records
    if (rc) return rc;
    materialize(h);
    DevScope mem;
    // sizes: k-mers per (map, submap) + the high-copy count
    unsigned long long* d_cnt = nullptr;
    HIPC(mem.alloc((void**)&d_cnt, (size_t)(n_sub + 1) * 8));
    HIPC(hipMemsetAsync(d_cnt, 0, (size_t)(n_sub + 1) * 8, h->stream));
    hipLaunchKernelGGL(k_dbi_hist, dim3(grid_for(h, h->n_slots(), 256)), dim3(256), 0, h->stream, h->view(), (uint32_t)h->map_count,
                       (uint32_t)map_lo, (uint32_t)map_hi, d_cnt);
    HIPC(hipGetLastError());
    std::vector<unsigned long long> cnt(n_sub + 1);
    HIPC(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    std::vector<ulonglong2> sub(n_sub + 1);                 // (byte offset of the submap's header, index of its first entry)
    uint64_t bytes = 0, n = 0;
    for (uint32_t s = 0; s < n_sub; ++s) {
        if (s % DBI_SUBMAPS == 0) { offsets[s / DBI_SUBMAPS] = bytes; bytes += 8; }
        sub[s] = make_ulonglong2(bytes, n);
        bytes += dbi_submap_bytes(cnt[s]);
        n += cnt[s];
    }
    offsets[n_maps] = bytes;
    sub[n_sub] = make_ulonglong2(bytes, n);
    *n_hc = cnt[n_sub];
    if (!out) return KQ_OK;
    if (cap < bytes) return fail(KQ_ERR_CAPACITY, "image buffer too small: need %llu bytes, have %llu", (unsigned long long)bytes, (unsigned long long)cap);
    if (hc_cap < *n_hc || (*n_hc && !hc_out)) return fail(KQ_ERR_CAPACITY, "high-copy buffer too small: need %llu entries, have %llu", (unsigned long long)*n_hc, (unsigned long long)hc_cap);
    if (n >= (1ull << 32)) return fail(KQ_ERR_INVALID, "%llu k-mers in maps [%u,%u): take the images in smaller map ranges (below 2^32 k-mers each)", (unsigned long long)n, map_lo, map_hi);
    // logical entries of the range in key order: the filter, sort and gather of kq_export
    kq_entry *d_ent = nullptr, *d_sorted = nullptr, *d_hc = nullptr;
    uint64_t *d_r1 = nullptr, *d_r2 = nullptr;
    unsigned long long *d_n = nullptr, *d_mat = nullptr;
    if (n) {
        if (mem.alloc((void**)&d_ent, (size_t)n * sizeof(kq_entry)) != hipSuccess) return fail(KQ_ERR_NOMEM, "no device memory for the %llu entries of maps [%u,%u)", (unsigned long long)n, map_lo, map_hi);
        HIPC(hipMemsetAsync(d_cnt, 0, 16, h->stream));      // [0]: k_export's counter, [1]: high-copy cursor
        d_n = d_cnt;
        hipLaunchKernelGGL(k_export, dim3(grid_for(h, h->n_slots(), 1024)), dim3(256), 0, h->stream, h->view(), (uint32_t)h->map_count,
                           (uint32_t)map_lo, (uint32_t)map_hi, d_ent, n, d_n);
        HIPC(hipGetLastError());
        if (!sort_entries_dev(h, mem, d_ent, n, &d_sorted)) return fail(KQ_ERR_NOMEM, "no device memory to sort the %llu entries of maps [%u,%u)", (unsigned long long)n, map_lo, map_hi);
        mem.release(d_ent);
        // records + stable split by (map, submap), least significant digit first
        const uint32_t G = (uint32_t)std::min<uint64_t>(1024, (n + 255) / 256);
        const uint64_t chunk = ((n + G - 1) / G + 255) / 256 * 256;
        if (mem.alloc((void**)&d_r1, (size_t)n * 8) != hipSuccess || mem.alloc((void**)&d_r2, (size_t)n * 8) != hipSuccess || mem.alloc((void**)&d_hc, (size_t)*n_hc * sizeof(kq_entry)) != hipSuccess ||
            mem.alloc((void**)&d_mat, (size_t)256 * G * 8) != hipSuccess) return fail(KQ_ERR_NOMEM, "no device memory for the record split of maps [%u,%u)", map_lo, map_hi);
        hipLaunchKernelGGL(k_dbi_records, dim3(grid_for(h, n, 256)), dim3(256), 0, h->stream, d_sorted, n, (uint32_t)h->map_count, (uint32_t)map_lo, d_r1, d_hc,
                           (uint64_t)*n_hc, d_n + 1);
        for (uint32_t shift = 32; (uint64_t)n_sub > (1ull << (shift - 32)); shift += 8) {
            hipLaunchKernelGGL(k_dbi_split_hist, dim3(G), dim3(256), 0, h->stream, d_r1, n, chunk, shift, d_mat);
            hipLaunchKernelGGL(k_dbi_split_scan, dim3(1), dim3(256), 0, h->stream, d_mat, G);
            hipLaunchKernelGGL(k_dbi_split_scatter, dim3(G), dim3(256), 0, h->stream, d_r1, n, chunk, shift, d_mat, d_r2);
            std::swap(d_r1, d_r2);
        }
        HIPC(hipGetLastError());
    }
    // the image
    uint8_t* d_img = nullptr;
    ulonglong2* d_sub = nullptr;
    if (mem.alloc((void**)&d_img, (size_t)bytes) != hipSuccess || mem.alloc((void**)&d_sub, sub.size() * sizeof(ulonglong2)) != hipSuccess)
        return fail(KQ_ERR_NOMEM, "no device memory for the %llu image bytes of maps [%u,%u)", (unsigned long long)bytes, map_lo, map_hi);
    HIPC(hipMemsetAsync(d_img, 0, (size_t)bytes, h->stream));
    HIPC(hipMemcpyAsync(d_sub, sub.data(), sub.size() * sizeof(ulonglong2), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_dbi_build, dim3(grid_for(h, n_sub, 4, 16)), dim3(256), 0, h->stream, d_sorted, d_r1, d_sub, n_sub, d_img);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(h->stream));
    hipError_t e = copy_out_bounced(h, out, d_img, (size_t)bytes);
    if (e == hipSuccess && *n_hc) e = hipMemcpy(hc_out, d_hc, (size_t)*n_hc * sizeof(kq_entry), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(KQ_ERR_HIP, "image copy failed: %s", hipGetErrorString(e));
    if (*n_hc) parallel_sort_entries(hc_out, *n_hc);
    return KQ_OK;
}

int kq_import_map_image(kq_handle* h, uint16_t map, const void* image, uint64_t n_bytes, uint64_t* n_entries, uint64_t* n_tombstones) {
    if (!image || !n_entries || !n_tombstones) return fail(KQ_ERR_INVALID, "null image / n_entries / n_tombstones");
    *n_entries = 0; *n_tombstones = 0;
    std::vector<DbiExtent> ext(DBI_SUBMAPS);
    uint64_t total = 0;
    if (const char* why = dbi_walk((const uint8_t*)image, n_bytes, ext.data(), &total)) return fail(KQ_ERR_INVALID, "%s (map %u)", why, map);
    if (!h) return fail(KQ_ERR_INVALID, "null handle");
    if (map >= h->map_count) return fail(KQ_ERR_INVALID, "map %u outside [0,%d)", map, h->map_count);
    if (!total) return KQ_OK;                               // 6152 bytes: an empty map
    HIPC(hipSetDevice(h->device));
    DevScope mem;
    uint8_t* d_img = nullptr; DbiExtent* d_ext = nullptr; DbiCheck* d_res = nullptr;
    if (mem.alloc((void**)&d_img, (size_t)n_bytes) != hipSuccess || mem.alloc((void**)&d_ext, ext.size() * sizeof(DbiExtent)) != hipSuccess || mem.alloc((void**)&d_res, sizeof(DbiCheck)) != hipSuccess)
        return fail(KQ_ERR_NOMEM, "no device memory for a map image of %llu bytes", (unsigned long long)n_bytes);
    HIPC(hipMemcpyAsync(d_img, image, (size_t)n_bytes, hipMemcpyHostToDevice, h->stream));
    HIPC(hipMemcpyAsync(d_ext, ext.data(), ext.size() * sizeof(DbiExtent), hipMemcpyHostToDevice, h->stream));
    HIPC(hipMemsetAsync(d_res, 0, sizeof(DbiCheck), h->stream));
    hipLaunchKernelGGL(k_dbi_check, dim3(DBI_SUBMAPS), dim3(256), 0, h->stream, d_img, d_ext, (uint32_t)h->k, (uint32_t)h->map_count, (uint32_t)map, d_res);
    HIPC(hipGetLastError());
    DbiCheck res;
    HIPC(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    if (res.bad_size) return fail(KQ_ERR_INVALID, "inconsistent submap size in the image of map %u", map);
    if (res.bad_map) return fail(KQ_ERR_INVALID, "%llu k-mers of the image do not belong to map %u", res.bad_map, map);
    if (res.bad_entry) return fail(KQ_ERR_INVALID, "%llu slots of the image of map %u are no valid k-mer records (cov 0, or an edge counter above cov)", res.bad_entry, map);
    int rc = reserve(h, total, res.instances);
    if (rc) return rc;
    materialize(h);
    h->table_empty = false;
    hipLaunchKernelGGL(k_dbi_add, dim3(DBI_SUBMAPS), dim3(256), 0, h->stream, h->view(), d_img, d_ext);
    HIPC(hipGetLastError());
    rc = kq_sync(h);
    if (rc) return rc;
    *n_entries = res.n_entries; *n_tombstones = res.n_tombstones;
    return KQ_OK;
}

// ---- subgraph mode (kq_subgraph.h; reference src/subgraph.cpp) --------------------------------------------------------
// the checks every subgraph entry point makes before any device work
static int sg_check(kq_handle* db, kq_handle* sub) {
    if (!db || !sub) return fail(KQ_ERR_INVALID, "null handle");
    if (db == sub) return fail(KQ_ERR_INVALID, "the subgraph needs a handle of its own (db == sub)");
    if (db->windowed || sub->windowed) return fail(KQ_ERR_INVALID, "subgraph calls do not take a windowed handle (KQ_OPT_BUCKET_WINDOW / KQ_OPT_SHARD_WINDOW)");
    if (db->k != sub->k || db->map_count != sub->map_count || db->device != sub->device)
        return fail(KQ_ERR_MISMATCH, "handles differ in k / map_count / device");
    return KQ_OK;
}
// both tables as they are after everything counted so far; the database's stream has drained, the work goes to sub's
static int sg_begin(kq_handle* db, kq_handle* sub) {
    HIPC(hipSetDevice(sub->device));
    { int frc = flush_pending(sub); if (frc) return frc; }
    { int frc = flush_pending(db); if (frc) return frc; }
    materialize(db);
    int rc = kq_sync(db);
    if (rc) return rc;
    materialize(sub);
    return KQ_OK;
}
static uint64_t pow2_at_least(uint64_t n) { uint64_t c = 1024; while (c < n) c *= 2; return c; }

int kq_subgraph_seed_dev(kq_handle* db, kq_handle* sub, const char* d_bases, uint64_t len, uint32_t flags) {
    int rc = sg_check(db, sub);
    if (rc) return rc;
    if (!d_bases && len) return fail(KQ_ERR_INVALID, "null sequence");
    if (flags & ~1u) return fail(KQ_ERR_INVALID, "unknown flags 0x%x", flags);
    if (len >= 0xFFFFFFFFull) return fail(KQ_ERR_INVALID, "sequence batch of %llu bytes: seed in batches below 2^32 - 1 bytes", (unsigned long long)len);
    rc = sg_begin(db, sub);
    if (rc) return rc;
    const int k = db->k;
    if (len < (uint64_t)k) return KQ_OK;
    hipStream_t st = sub->stream;
    const uint64_t n_pos = len - (uint64_t)k + 1, set_size = pow2_at_least(2 * n_pos);
    DevScope mem;
    uint32_t *d_flag = nullptr, *d_seg = nullptr, *d_set = nullptr;
    uint64_t* d_key = nullptr; uint8_t* d_info = nullptr; void* d_tmp = nullptr;
    struct Res { SgSeedOut out; unsigned int err, pad; } res;
    Res* d_res = nullptr;
    size_t tmp_bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_flag, d_seg, (int64_t)len, st) != hipSuccess) return fail(KQ_ERR_HIP, "segment scan setup failed");
    if (mem.alloc((void**)&d_flag, len * 4) != hipSuccess || mem.alloc((void**)&d_seg, len * 4) != hipSuccess || mem.alloc((void**)&d_key, n_pos * 8) != hipSuccess ||
        mem.alloc((void**)&d_info, n_pos) != hipSuccess || mem.alloc((void**)&d_set, set_size * 4) != hipSuccess || mem.alloc(&d_tmp, tmp_bytes) != hipSuccess ||
        mem.alloc((void**)&d_res, sizeof(Res)) != hipSuccess)
        return fail(KQ_ERR_NOMEM, "no device memory for the seed scratch of %llu bases", (unsigned long long)len);
    const uint8_t* ab; uint64_t lead;
    aligned_view(d_bases, &ab, &lead);
    HIPC(hipMemsetAsync(d_key, 0xFF, n_pos * 8, st));
    HIPC(hipMemsetAsync(d_set, 0xFF, set_size * 4, st));
    HIPC(hipMemsetAsync(d_res, 0, sizeof(Res), st));
    hipLaunchKernelGGL(k_sg_invalid, dim3(grid_for(sub, len, 256)), dim3(256), 0, st, (const uint8_t*)d_bases, len, d_flag);
    HIPC(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_flag, d_seg, (int64_t)len, st));
    hipLaunchKernelGGL(k_sg_keys, dim3(grid_for(sub, n_tiles_of(lead, len), 1, 32)), dim3(TILE_THREADS), 0, st, ab, lead, len, k, d_key, d_info);
    hipLaunchKernelGGL(k_sg_first, dim3(grid_for(sub, n_pos, 256)), dim3(256), 0, st, d_key, d_seg, n_pos, d_set, set_size - 1, &d_res->err);
    // what the winners will add, so that the table grows before they do
    hipLaunchKernelGGL(k_sg_seed_add<false>, dim3(grid_for(sub, set_size, 256)), dim3(256), 0, st, db->view(), sub->view(), d_set, set_size, d_key, d_info,
                       flags & 1u, &d_res->out);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (res.err) return fail(KQ_ERR_HIP, "seed: the (segment, k-mer) set overflowed");      // cannot happen: the set has two slots per position
    if (!res.out.n_kmers) return KQ_OK;
    rc = reserve(sub, res.out.n_kmers, res.out.n_instances);
    if (rc) return rc;
    sub->table_empty = false;
    hipLaunchKernelGGL(k_sg_seed_add<true>, dim3(grid_for(sub, set_size, 256)), dim3(256), 0, st, db->view(), sub->view(), d_set, set_size, d_key, d_info,
                       flags & 1u, &d_res->out);
    HIPC(hipGetLastError());
    return kq_sync(sub);
}
int kq_subgraph_seed(kq_handle* db, kq_handle* sub, const char* bases, uint64_t len, uint32_t flags) {
    int rc = sg_check(db, sub);
    if (rc) return rc;
    if (!bases && len) return fail(KQ_ERR_INVALID, "null sequence");
    if (flags & ~1u) return fail(KQ_ERR_INVALID, "unknown flags 0x%x", flags);
    HIPC(hipSetDevice(sub->device));
    void* d = nullptr;
    rc = stage_in(sub, bases, len, &d);
    if (rc) return rc;
    return kq_subgraph_seed_dev(db, sub, (const char*)d, len, flags);
}

}  // extern "C"
namespace {
// The found list of an expansion -- ents[0, n_seed) = the seed k-mers with their subgraph entries, ents[n_seed, n_ents) = what
// was found, in the order found -- and the visited key set (load <= 1/2) of the k-mers found.  Both double like a table.
struct SgFound {
    DevScope mem;
    SgExpandState* d_state = nullptr;
    kq_entry* d_ents = nullptr; uint64_t* d_vis = nullptr;
    uint64_t ents_cap = 0, vis_size = 0;
    // room for `need` entries in all, n_ents of which are there
    int room(kq_handle* sub, uint64_t n_seed, uint64_t n_ents, uint64_t need) {
        hipStream_t st = sub->stream;
        if (need > ents_cap) {
            uint64_t cap = std::max<uint64_t>(ents_cap, 1024);
            while (cap < need) cap *= 2;
            kq_entry* fresh = nullptr;
            if (mem.alloc((void**)&fresh, cap * sizeof(kq_entry)) != hipSuccess) return fail(KQ_ERR_TABLE_FULL, "cannot grow the frontier list to %llu k-mers: out of device memory", (unsigned long long)cap);
            if (n_ents && d_ents) HIPC(hipMemcpyAsync(fresh, d_ents, n_ents * sizeof(kq_entry), hipMemcpyDeviceToDevice, st));
            HIPC(hipStreamSynchronize(st));
            mem.release(d_ents);
            d_ents = fresh; ents_cap = cap;
        }
        const uint64_t vis_need = 2 * (need - n_seed);
        if (vis_need > vis_size) {
            const uint64_t size = pow2_at_least(std::max(vis_need, 2 * vis_size));
            HIPC(hipStreamSynchronize(st));
            mem.release(d_vis);
            if (mem.alloc((void**)&d_vis, size * 8) != hipSuccess) { d_vis = nullptr; vis_size = 0; return fail(KQ_ERR_TABLE_FULL, "cannot grow the visited set to %llu slots: out of device memory", (unsigned long long)size); }
            vis_size = size;
            HIPC(hipMemsetAsync(d_vis, 0xFF, size * 8, st));
            if (n_ents > n_seed) hipLaunchKernelGGL(k_sg_visited_fill, dim3(grid_for(sub, n_ents - n_seed, 256)), dim3(256), 0, st, d_ents, n_seed, n_ents, d_vis, size - 1, d_state);
        }
        return KQ_OK;
    }
};
}  // namespace
extern "C" {

int kq_subgraph_expand(kq_handle* db, kq_handle* sub, int depth, uint64_t* n_added) {
    int rc = sg_check(db, sub);
    if (rc) return rc;
    if (!n_added) return fail(KQ_ERR_INVALID, "null n_added");
    if (depth < 0 || depth > 255) return fail(KQ_ERR_INVALID, "search depth %d outside 0..255", depth);      // uint8_t in the reference (src/subgraph.cpp:307)
    *n_added = 0;
    rc = sg_begin(db, sub);
    if (rc) return rc;
    rc = check_errors(sub);
    if (rc) return rc;
    const uint64_t n_seed = sub->host_state()->slots_used;
    if (!depth || !n_seed) return KQ_OK;
    hipStream_t st = sub->stream;
    SgFound fl;
    DevScope& mem = fl.mem;
    SgExpandState state{};
    SgExpandState*& d_state = fl.d_state;
    kq_entry*& d_ents = fl.d_ents; uint64_t*& d_vis = fl.d_vis;
    uint64_t &ents_cap = fl.ents_cap, &vis_size = fl.vis_size;
    // room for a round that finds 8 k-mers per frontier k-mer
    auto make_room = [&](uint64_t n_ents, uint64_t frontier) -> int { return fl.room(sub, n_seed, n_ents, n_ents + 8 * frontier); };
    if (mem.alloc((void**)&d_state, sizeof(SgExpandState)) != hipSuccess) return fail(KQ_ERR_NOMEM, "no device memory");
    rc = make_room(n_seed, n_seed);
    if (rc) return rc;
    // the seeds with their subgraph entries: the first frontier (the counter of k_export becomes n_ents)
    HIPC(hipMemsetAsync(d_state, 0, sizeof(SgExpandState), st));
    hipLaunchKernelGGL(k_export, dim3(grid_for(sub, sub->n_slots(), 1024)), dim3(256), 0, st, sub->view(), (uint32_t)sub->map_count, 0u, (uint32_t)sub->map_count,
                       d_ents, ents_cap, &d_state->n_ents);
    HIPC(hipGetLastError());
    uint64_t f_lo = 0, f_hi = n_seed;
    for (int round = 0; round < depth && f_hi > f_lo; ++round) {
        rc = make_room(f_hi, f_hi - f_lo);
        if (rc) return rc;
        hipLaunchKernelGGL(k_sg_expand, dim3(grid_for(sub, (f_hi - f_lo) * 8, 256)), dim3(256), 0, st, db->view(), sub->view(), d_ents, f_lo, f_hi, ents_cap,
                           d_vis, vis_size - 1, d_state);
        HIPC(hipGetLastError());
        // only the size of the next frontier returns to the host
        HIPC(hipMemcpyAsync(&state, d_state, sizeof state, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        if (state.err) return fail(KQ_ERR_HIP, "expand: frontier list or visited set overflowed (%u)", state.err);      // cannot happen: make_room
        if (round == 0 && state.n_ents < n_seed) return fail(KQ_ERR_HIP, "expand: %llu of %llu seeds listed", (unsigned long long)state.n_ents, (unsigned long long)n_seed);
        f_lo = f_hi; f_hi = state.n_ents;
    }
    const uint64_t n_found = f_hi - n_seed;
    if (n_found) {                                   // after the last round: the seed set was "seeds only" throughout (src/subgraph.cpp:321)
        rc = reserve(sub, n_found, state.n_instances);
        if (rc) return rc;
        hipLaunchKernelGGL(k_import, dim3(grid_for(sub, n_found, 256)), dim3(256), 0, st, sub->view(), (const kq_entry*)(d_ents + n_seed), n_found);
        HIPC(hipGetLastError());
        rc = kq_sync(sub);
        if (rc) return rc;
    }
    *n_added = n_found;
    return KQ_OK;
}

// Scratch budget of the best-first searches: every search of a batch owns one state block of kqbf::block_bytes(depth) bytes
// (2.8 KB at depth 21, 33 KB at depth 255), so a batch is SG_BF_ARENA_BYTES / block bytes searches (at least one, at most the
// seeds there are): 380 000 at depth 21, 32 000 at depth 255 -- either fills the chip's 2^19 lanes most of the way, and 1 GiB is
// small next to a database that is worth a device search.  KQ_OPT_SUBGRAPH_BATCH fixes the number instead (tests).
constexpr uint64_t SG_BF_ARENA_BYTES = 1ull << 30;

int kq_subgraph_best_first(kq_handle* db, kq_handle* sub, int depth, uint32_t cov_cutoff, uint64_t* n_added) {
    int rc = sg_check(db, sub);
    if (rc) return rc;
    if (!n_added) return fail(KQ_ERR_INVALID, "null n_added");
    if (depth < 0 || depth > kqbf::MAX_DEPTH) return fail(KQ_ERR_INVALID, "search depth %d outside 0..255", depth);      // uint8_t in the reference (src/subgraph.cpp:460)
    *n_added = 0;
    rc = sg_begin(db, sub);
    if (rc) return rc;
    rc = check_errors(sub);
    if (rc) return rc;
    const uint64_t n_seed = sub->host_state()->slots_used;
    if (!depth || !n_seed) return KQ_OK;             // depth 0: the one pop meets seeds or inserts nodes, and nothing lies between a destination and its source
    hipStream_t st = sub->stream;
    SgFound fl;
    const uint64_t block_bytes = kqbf::block_bytes(depth);
    const uint32_t n_slots = kqbf::node_bound(depth);
    const uint64_t batch = std::min<uint64_t>(n_seed, db->sg_batch ? db->sg_batch : std::max<uint64_t>(1, SG_BF_ARENA_BYTES / block_bytes));
    uint8_t* d_arena = nullptr;
    struct Res { SgBfState bf; SgExpandState ex; } res{};
    Res* d_res = nullptr;
    if (fl.mem.alloc((void**)&d_res, sizeof(Res)) != hipSuccess) return fail(KQ_ERR_NOMEM, "no device memory");
    fl.d_state = &d_res->ex;
    if (fl.mem.alloc((void**)&d_arena, batch * block_bytes) != hipSuccess)
        return fail(KQ_ERR_NOMEM, "no device memory for the state blocks of %llu searches of depth %d", (unsigned long long)batch, depth);
    rc = fl.room(sub, n_seed, 0, n_seed + 1);
    if (rc) return rc;
    // the sources: the seed k-mers with their merged subgraph entries (the counter of k_export becomes n_ents)
    HIPC(hipMemsetAsync(d_res, 0, sizeof(Res), st));
    hipLaunchKernelGGL(k_export, dim3(grid_for(sub, sub->n_slots(), 1024)), dim3(256), 0, st, sub->view(), (uint32_t)sub->map_count, 0u, (uint32_t)sub->map_count,
                       fl.d_ents, fl.ents_cap, &d_res->ex.n_ents);
    HIPC(hipGetLastError());
    uint64_t n_ents = n_seed;
    for (uint64_t lo = 0; lo < n_seed; lo += batch) {
        const uint64_t n = std::min(batch, n_seed - lo);
        HIPC(hipMemsetAsync(d_arena, 0xFF, n * block_bytes, st));      // the node indexes: every slot free (the rest of a block is written before it is read)
        HIPC(hipMemsetAsync(&d_res->bf, 0, sizeof(SgBfState), st));
        hipLaunchKernelGGL(k_sg_bf_search, dim3(grid_for(sub, n, 256)), dim3(256), 0, st, db->view(), sub->view(), (const kq_entry*)(fl.d_ents + lo), n, depth, cov_cutoff,
                           d_arena, block_bytes, &d_res->bf);
        HIPC(hipGetLastError());
        // only the batch's total and the status words return to the host (with them the length of the found list after the batch before)
        HIPC(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        if (lo == 0 && res.ex.n_ents != n_seed) return fail(KQ_ERR_HIP, "best-first: %llu of %llu seeds listed", (unsigned long long)res.ex.n_ents, (unsigned long long)n_seed);
        if (res.bf.err) return fail(KQ_ERR_HIP, "best-first: a search left its state block's bounds (error mask %u)", res.bf.err);      // cannot happen: 9 + 4 depth nodes
        if (res.ex.err) return fail(KQ_ERR_HIP, "best-first: found list or visited set overflowed (%u)", res.ex.err);      // cannot happen: room()
        n_ents = res.ex.n_ents;
        if (!res.bf.n_found) continue;
        rc = fl.room(sub, n_seed, n_ents, n_ents + res.bf.n_found);      // every discovered node may be a new k-mer
        if (rc) return rc;
        hipLaunchKernelGGL(k_sg_bf_collect, dim3(grid_for(sub, n * n_slots, 256)), dim3(256), 0, st, db->view(), (const uint8_t*)d_arena, block_bytes, n, n_slots,
                           fl.d_ents, fl.ents_cap, fl.d_vis, fl.vis_size - 1, &d_res->ex);
        HIPC(hipGetLastError());
    }
    HIPC(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (res.ex.err) return fail(KQ_ERR_HIP, "best-first: found list or visited set overflowed (%u)", res.ex.err);          // cannot happen: room()
    n_ents = res.ex.n_ents;
    const uint64_t n_found = n_ents - n_seed;
    if (n_found) {                                   // after the last batch: the seed set was "seeds only" during every search (src/subgraph.cpp:453)
        rc = reserve(sub, n_found, res.ex.n_instances);
        if (rc) return rc;
        hipLaunchKernelGGL(k_import, dim3(grid_for(sub, n_found, 256)), dim3(256), 0, st, sub->view(), (const kq_entry*)(fl.d_ents + n_seed), n_found);
        HIPC(hipGetLastError());
        rc = kq_sync(sub);
        if (rc) return rc;
    }
    *n_added = n_found;
    return KQ_OK;
}

int kq_subgraph_trim(kq_handle* sub, uint32_t cov_cutoff) {
    if (!sub) return fail(KQ_ERR_INVALID, "null handle");
    if (sub->windowed) return fail(KQ_ERR_INVALID, "subgraph calls do not take a windowed handle (KQ_OPT_BUCKET_WINDOW / KQ_OPT_SHARD_WINDOW)");
    HIPC(hipSetDevice(sub->device));
    int rc = flush_pending(sub);
    if (rc) return rc;
    materialize(sub);
    hipLaunchKernelGGL(k_sg_trim, dim3(grid_for(sub, sub->n_slots(), 256)), dim3(256), 0, sub->stream, sub->view(), cov_cutoff);
    HIPC(hipGetLastError());
    return kq_sync(sub);
}

// ---- the subgraph as a compacted graph (kq_gfa.h; reference src/kreeq.cpp:360-600) ------------------------------------------
// With KQ_OPT_PROFILE the stages leave marks (kq_get_profile): gfa_order, gfa_links, gfa_rank_<i> for the i-th pointer-jumping
// round of the call, gfa_cut, gfa_heads, gfa_edges, gfa_write.
static const char* gfa_round_name(uint32_t i) {                          // 2 rankings of at most 1 + 32 rounds
    static const std::vector<std::string> names = [] { std::vector<std::string> v; for (int j = 1; j <= 66; ++j) v.push_back("gfa_rank_" + std::to_string(j)); return v; }();
    return names[std::min<size_t>(i, names.size() - 1)].c_str();
}
int kq_subgraph_gfa(kq_handle* sub, uint32_t flags, kq_gfa_segment* segs, uint64_t seg_cap, char* seq, uint64_t seq_cap, kq_gfa_edge* edges, uint64_t edge_cap,
                    kq_gfa_counts* counts) {
    if (!sub || !counts) return fail(KQ_ERR_INVALID, "null argument");
    if (flags & ~(uint32_t)KQ_GFA_NO_COLLAPSE) return fail(KQ_ERR_INVALID, "unknown flags 0x%x", flags);
    if (sub->windowed) return fail(KQ_ERR_INVALID, "subgraph calls do not take a windowed handle (KQ_OPT_BUCKET_WINDOW / KQ_OPT_SHARD_WINDOW)");
    *counts = kq_gfa_counts{};
    HIPC(hipSetDevice(sub->device));
    int rc = check_errors(sub);                                          // flushes; the state says how many k-mers there are
    if (rc) return rc;
    const uint64_t n64 = sub->host_state()->slots_used;
    if (n64 >= (1ull << 31)) return fail(KQ_ERR_INVALID, "subgraph of %llu k-mers: oriented k-mer ids are 32-bit (fewer than 2^31 k-mers)", (unsigned long long)n64);
    if (!n64) return KQ_OK;
    materialize(sub);
    hipStream_t st = sub->stream;
    marks_reset(sub);
    mark(sub, "gfa_begin");
    const uint32_t n = (uint32_t)n64, k = (uint32_t)sub->k;
    const uint64_t n2 = 2 * n64, n_items = 4 * n2;
    const bool collapse = !(flags & KQ_GFA_NO_COLLAPSE), want_out = segs && seq && edges;
    DevScope mem;
    GfaState state{};
    GfaState* d_state = nullptr;
    kq_entry *d_raw = nullptr, *d_ents = nullptr;
    uint64_t* d_keys = nullptr; uint32_t* d_succ = nullptr; GfaNode* d_node[2] = {nullptr, nullptr};
    unsigned long long *d_flag = nullptr, *d_len = nullptr, *d_seg_id = nullptr, *d_seq_off = nullptr, *d_eflag = nullptr, *d_epos = nullptr, *d_n = nullptr;
    void* d_tmp = nullptr;
    size_t tmp_heads = 0, tmp_items = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_heads, d_flag, d_seg_id, (int64_t)(n2 + 1), st) != hipSuccess ||
        hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_items, d_eflag, d_epos, (int64_t)(n_items + 1), st) != hipSuccess)
        return fail(KQ_ERR_HIP, "prefix sum setup failed");
    auto nomem = [&]() { return fail(KQ_ERR_NOMEM, "no device memory for the graph of %llu k-mers", (unsigned long long)n64); };
    // (a) the entries in key order, their keys alone for the rank lookup
    if (mem.alloc((void**)&d_state, sizeof(GfaState)) != hipSuccess || mem.alloc((void**)&d_n, 8) != hipSuccess || mem.alloc((void**)&d_raw, n64 * sizeof(kq_entry)) != hipSuccess) return nomem();
    HIPC(hipMemsetAsync(d_state, 0, sizeof(GfaState), st));
    HIPC(hipMemsetAsync(d_n, 0, 8, st));
    hipLaunchKernelGGL(k_export, dim3(grid_for(sub, sub->n_slots(), 1024)), dim3(256), 0, st, sub->view(), (uint32_t)sub->map_count, 0u, (uint32_t)sub->map_count, d_raw, n64, d_n);
    HIPC(hipGetLastError());
    unsigned long long n_listed = 0;
    HIPC(hipMemcpyAsync(&n_listed, d_n, 8, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (n_listed != n64) return fail(KQ_ERR_HIP, "graph: %llu of %llu k-mers listed", n_listed, (unsigned long long)n64);
    if (!sort_entries_dev(sub, mem, d_raw, n64, &d_ents)) return nomem();
    mem.release(d_raw);
    if (mem.alloc((void**)&d_keys, n64 * 8) != hipSuccess || mem.alloc((void**)&d_succ, n2 * 4) != hipSuccess || mem.alloc((void**)&d_node[0], n2 * sizeof(GfaNode)) != hipSuccess) return nomem();
    hipLaunchKernelGGL(k_gfa_keys, dim3(grid_for(sub, n64, 256)), dim3(256), 0, st, (const kq_entry*)d_ents, n, d_keys);
    mark(sub, "gfa_order");
    int cur = 0;
    uint32_t rounds = 0;
    if (collapse) {
        if (mem.alloc((void**)&d_node[1], n2 * sizeof(GfaNode)) != hipSuccess) return nomem();
        // (b) the links
        hipLaunchKernelGGL(k_gfa_links, dim3(grid_for(sub, n2, 256)), dim3(256), 0, st, (const kq_entry*)d_ents, (const uint64_t*)d_keys, n, k, d_succ);
        HIPC(hipGetLastError());
        mark(sub, "gfa_links");
        // (c) ranking; a second time after the cycles were opened
        uint32_t round_limit = 1;
        while ((1ull << (round_limit - 1)) < n2) ++round_limit;          // 1 + ceil(log2(2n))
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(k_gfa_rank_init, dim3(grid_for(sub, n2, 256)), dim3(256), 0, st, (const uint32_t*)d_succ, n, d_node[cur], d_state);
            bool live = true;
            for (uint32_t r = 0; r < round_limit && live; ++r) {
                HIPC(hipMemsetAsync(&d_state->changed, 0, sizeof(unsigned int), st));
                hipLaunchKernelGGL(k_gfa_rank_round, dim3(grid_for(sub, n2, 256)), dim3(256), 0, st, (const GfaNode*)d_node[cur], d_node[cur ^ 1], n, d_state);
                HIPC(hipGetLastError());
                mark(sub, gfa_round_name(rounds++));
                cur ^= 1;
                HIPC(hipMemcpyAsync(&state, d_state, sizeof state, hipMemcpyDeviceToHost, st));      // only the changed flag and the error mask return to the host
                HIPC(hipStreamSynchronize(st));
                if (state.err) return fail(KQ_ERR_HIP, "graph: a chain pointer left its bounds (error mask %u)", state.err);
                live = state.changed != 0;
            }
            if (!live) break;
            if (pass == 1) return fail(KQ_ERR_HIP, "graph: the chains did not rank in %u rounds after the cycles were opened", round_limit);
            hipLaunchKernelGGL(k_gfa_cut, dim3(grid_for(sub, n2, 256)), dim3(256), 0, st, (const GfaNode*)d_node[cur], n, d_succ, d_state);
            HIPC(hipGetLastError());
            mark(sub, "gfa_cut");
        }
        mem.release(d_node[cur ^ 1]);
        d_node[cur ^ 1] = nullptr;
    } else {                                                             // (f) every oriented k-mer is a chain of its own
        HIPC(hipMemsetAsync(d_succ, 0xFF, n2 * 4, st));
        hipLaunchKernelGGL(k_gfa_rank_init, dim3(grid_for(sub, n2, 256)), dim3(256), 0, st, (const uint32_t*)d_succ, n, d_node[0], d_state);
    }
    const GfaNode* d_rank = d_node[cur];
    // (d) segment ids and sequence offsets
    if (mem.alloc((void**)&d_flag, (n2 + 1) * 8) != hipSuccess || mem.alloc((void**)&d_len, (n2 + 1) * 8) != hipSuccess || mem.alloc((void**)&d_seg_id, (n2 + 1) * 8) != hipSuccess ||
        mem.alloc((void**)&d_seq_off, (n2 + 1) * 8) != hipSuccess || mem.alloc(&d_tmp, std::max(tmp_heads, tmp_items)) != hipSuccess)
        return nomem();
    hipLaunchKernelGGL(k_gfa_heads, dim3(grid_for(sub, n2 + 1, 256)), dim3(256), 0, st, d_rank, n, k, d_flag, d_len, d_state);
    HIPC(hipGetLastError());
    HIPC(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_heads, d_flag, d_seg_id, (int64_t)(n2 + 1), st));
    HIPC(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_heads, d_len, d_seq_off, (int64_t)(n2 + 1), st));
    HIPC(hipStreamSynchronize(st));                                      // the scans read what is released here
    mem.release(d_flag); mem.release(d_len);
    mark(sub, "gfa_heads");
    // (e) the edges: flags, then their places
    if (mem.alloc((void**)&d_eflag, (n_items + 1) * 8) != hipSuccess || mem.alloc((void**)&d_epos, (n_items + 1) * 8) != hipSuccess) return nomem();
    hipLaunchKernelGGL(k_gfa_edges<false>, dim3(grid_for(sub, n_items + 1, 256)), dim3(256), 0, st, (const kq_entry*)d_ents, (const uint64_t*)d_keys, (const uint32_t*)d_succ, d_rank,
                       (const unsigned long long*)d_seg_id, n, k, (uint32_t)collapse, d_eflag, (const unsigned long long*)nullptr, (kq_gfa_edge*)nullptr, 0ull, d_state);
    HIPC(hipGetLastError());
    HIPC(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_items, d_eflag, d_epos, (int64_t)(n_items + 1), st));
    unsigned long long n_segs = 0, n_seq = 0, n_edges = 0;
    mark(sub, "gfa_edges");
    HIPC(hipMemcpyAsync(&n_segs, d_seg_id + n2, 8, hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(&n_seq, d_seq_off + n2, 8, hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(&n_edges, d_epos + n_items, 8, hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(&state, d_state, sizeof state, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (state.err) return fail(KQ_ERR_HIP, "graph: a chain left its bounds (error mask %u)", state.err);
    counts->n_segments = n_segs; counts->n_seq = n_seq; counts->n_edges = n_edges; counts->n_dropped_edges = state.n_dropped; counts->n_cycles = state.n_cycles;
    if (!want_out) return KQ_OK;
    if (n_segs > seg_cap || n_seq > seq_cap || n_edges > edge_cap)
        return fail(KQ_ERR_CAPACITY, "%llu segments with %llu bases and %llu links: the buffers hold %llu, %llu and %llu", n_segs, n_seq, n_edges, (unsigned long long)seg_cap,
                    (unsigned long long)seq_cap, (unsigned long long)edge_cap);
    // the records and the bases
    mem.release(d_eflag);
    kq_gfa_segment* d_segs = nullptr; char* d_seq = nullptr; kq_gfa_edge* d_edges = nullptr;
    if (mem.alloc((void**)&d_segs, n_segs * sizeof(kq_gfa_segment)) != hipSuccess || mem.alloc((void**)&d_seq, n_seq) != hipSuccess || mem.alloc((void**)&d_edges, n_edges * sizeof(kq_gfa_edge)) != hipSuccess)
        return nomem();
    hipLaunchKernelGGL(k_gfa_segments, dim3(grid_for(sub, n2, 256)), dim3(256), 0, st, (const kq_entry*)d_ents, d_rank, n, k, (const unsigned long long*)d_seg_id,
                       (const unsigned long long*)d_seq_off, d_segs, (uint64_t)n_segs, d_seq, (uint64_t)n_seq, d_state);
    hipLaunchKernelGGL(k_gfa_edges<true>, dim3(grid_for(sub, n_items + 1, 256)), dim3(256), 0, st, (const kq_entry*)d_ents, (const uint64_t*)d_keys, (const uint32_t*)d_succ, d_rank,
                       (const unsigned long long*)d_seg_id, n, k, (uint32_t)collapse, (unsigned long long*)nullptr, (const unsigned long long*)d_epos, d_edges, (uint64_t)n_edges, d_state);
    HIPC(hipGetLastError());
    mark(sub, "gfa_write");
    HIPC(hipMemcpyAsync(&state, d_state, sizeof state, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (state.err) return fail(KQ_ERR_HIP, "graph: a record left its bounds (error mask %u)", state.err);      // cannot happen: the totals are the scans'
    hipError_t e1 = n_segs ? copy_out_bounced(sub, segs, d_segs, n_segs * sizeof(kq_gfa_segment)) : hipSuccess;
    hipError_t e2 = n_seq ? copy_out_bounced(sub, seq, d_seq, n_seq) : hipSuccess;
    hipError_t e3 = n_edges ? copy_out_bounced(sub, edges, d_edges, n_edges * sizeof(kq_gfa_edge)) : hipSuccess;
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return fail(KQ_ERR_HIP, "graph: copy out failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2 != hipSuccess ? e2 : e3));
    return KQ_OK;
}

}  // extern "C"
