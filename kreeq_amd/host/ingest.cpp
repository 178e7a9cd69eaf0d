// Reads -> GPU: the parser threads share a small POOL of page-locked buffers.  A thread takes a free buffer, fills it and
// submits it itself (kq_count_batch_async: enqueues the DMA and the count kernels behind it, returns at once); the buffer
// goes back to the pool when its copy has finished.  Parsing, PCIe copies and counting overlap without a consumer thread.
// Why a pool: what costs on this path is not PCIe (a page-locked buffer copies at 50+ GB/s) but making host pages
// DMA-able -- a copy out of a fresh pageable buffer takes 6-7 ms per 4-8 MB for exactly that, and buffers of their own for
// every parser thread paid it once per buffer (35 of the 38 ms of ingesting a 310 MB FASTQ).  A pool is locked once
// (kq_host_alloc: ~0.5 ms per buffer) and every copy after that runs at PCIe rate.
// Optional (KQ_INGEST_PACK=1): the parser thread packs a buffer to 2 bits per base + a validity bit (kq_pack_bases) before
// it submits it: 6 bytes per 16 bases cross PCIe instead of 16.
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "cli_common.h"
#include "fastx.h"

namespace kqhost {

namespace {

struct GpuSink {
    kq_handle* h;
    size_t cap;
    bool packed;
    bool device_parse = false;                    // KQ_INGEST_DEVICE: plain files travel as raw text, the records are found on the GPU (kq_count_fastx_async)
    struct Buf { char* ascii = nullptr; uint32_t* codes = nullptr; uint16_t* inv = nullptr; uint64_t ticket = 0; bool in_flight = false; };
    std::vector<Buf> pool;
    std::vector<int> free_list;                   // indices of buffers nobody holds
    std::vector<int> flying;                      // submitted, oldest first
    std::mutex m;
    std::condition_variable cv;
    bool failed = false;                          // a parser thread or a submit has failed: nobody waits for a buffer any more (under m)
    std::string cause;                            // what failed first (under m, set with `failed`): the threads that give up because of it
                                                  // throw the same text, so the error reported does not depend on which thread's exception is seen first
    void set_failed(const std::string& why) { if (!failed) { failed = true; cause = why; } }     // (call under m)
    std::atomic<long long> ns_wait{0}, ns_pack{0}, ns_call{0}, n_submit{0}, n_dev_submit{0};     // KQ_INGEST_TRACE: where the threads spend their time
    GpuSink(kq_handle* handle, unsigned n_buffers, size_t buffer_bytes, bool pack, bool dev_parse = false)
        : h(handle), cap(buffer_bytes), packed(pack && !dev_parse), device_parse(dev_parse), pool(n_buffers) {
        for (unsigned i = 0; i < n_buffers; ++i) free_list.push_back((int)(n_buffers - 1 - i));
    }
    // a buffer gets its memory from the thread that first takes it: the page locking of the pool runs in parallel
    void materialize(Buf& b) {
        if (b.ascii) return;
        // packed mode: the ASCII buffer never crosses PCIe (plain memory), the packed arrays do
        b.ascii = packed ? (char*)malloc(cap) : (char*)kq_host_alloc(cap);
        if (packed) { b.codes = (uint32_t*)kq_host_alloc((cap / 16 + 1) * 4); b.inv = (uint16_t*)kq_host_alloc((cap / 16 + 1) * 2); }
        if (!b.ascii || (packed && (!b.codes || !b.inv))) throw std::runtime_error("read buffer allocation failed");
    }
    // every copy that still reads a pool buffer has finished (kq_host_free's contract, include/kreeq_amd.h)
    void drain() {
        std::vector<uint64_t> tickets;
        { std::lock_guard<std::mutex> l(m); for (int i : flying) tickets.push_back(pool[i].ticket); for (int i : flying) free_list.push_back(i); flying.clear(); }
        for (uint64_t tk : tickets) (void)kq_host_wait(h, tk);
    }
    void fail(const std::string& why = "") { { std::lock_guard<std::mutex> l(m); set_failed(why); } cv.notify_all(); }
    ~GpuSink() {
        drain();
        for (auto& b : pool) { if (packed) free(b.ascii); else kq_host_free(b.ascii); kq_host_free(b.codes); kq_host_free(b.inv); }
    }
    // raw_fmt: 0 = buf holds '\n'-separated sequences, KQ_FASTX_* = raw text of whole records (device parser)
    void submit_buf(char* buf, size_t len, int raw_fmt) {
        int i = 0;
        while (pool[i].ascii != buf) ++i;
        Buf& b = pool[i];
        const auto t0 = std::chrono::steady_clock::now();
        if (packed && !raw_fmt) kq_pack_bases(buf, len, b.codes, b.inv);
        const auto t1 = std::chrono::steady_clock::now();
        // no lock around the call: kq_count_*_async may be called from several threads (they take turns inside the library)
        int rc = !len ? KQ_OK : raw_fmt ? kq_count_fastx_async(h, buf, len, raw_fmt, &b.ticket) : packed ? kq_count_packed_async(h, b.codes, b.inv, len, &b.ticket) : kq_count_batch_async(h, buf, len, &b.ticket);
        static const long fail_after = getenv("KQ_TEST_FAIL_SUBMIT") ? atol(getenv("KQ_TEST_FAIL_SUBMIT")) : -1;      // failure-path test: every submit from the n-th on fails
        const bool injected = rc == KQ_OK && len && fail_after >= 0 && n_submit.load() >= fail_after;
        if (injected) { (void)kq_host_wait(h, b.ticket); rc = KQ_ERR_NOMEM; }
        if (rc != KQ_OK || !len) {
            // a failed submit (out of device memory at scale ...) or a buffer that was taken and not filled: the buffer goes
            // back to the pool; on failure every thread waiting for a buffer is woken and throws (they used to
            // wait forever for buffers held by threads that had died)
            const std::string err = injected ? "submit failed (injected by KQ_TEST_FAIL_SUBMIT)" : rc != KQ_OK ? kq_last_error() : "";
            { std::lock_guard<std::mutex> l(m); free_list.push_back(i); if (rc != KQ_OK) set_failed("Error: " + err); }
            cv.notify_all();
            if (rc != KQ_OK) throw std::runtime_error("Error: " + err);
            return;
        }
        ns_pack += (t1 - t0).count(); ns_call += (std::chrono::steady_clock::now() - t1).count(); ++n_submit; if (raw_fmt) ++n_dev_submit;
        std::lock_guard<std::mutex> l(m);
        flying.push_back(i);
        cv.notify_one();
    }
    RawSink sink() {
        RawSink bs;
        bs.acquire = [this](unsigned, size_t* c) {
            const auto t0 = std::chrono::steady_clock::now();
            std::unique_lock<std::mutex> l(m);
            for (;;) {
                if (failed) throw std::runtime_error(cause.empty() ? "read ingest aborted" : cause);      // (the first failure is the one reported)
                if (!free_list.empty()) break;
                if (!flying.empty()) {                                // the oldest copy in flight: wait for it outside the lock
                    const int i = flying.front();
                    flying.erase(flying.begin());
                    const uint64_t tk = pool[i].ticket;
                    l.unlock();
                    const int wrc = kq_host_wait(h, tk);
                    const std::string werr = wrc != KQ_OK ? kq_last_error() : "";
                    l.lock();
                    free_list.push_back(i);                           // back to the pool whatever happened
                    if (wrc != KQ_OK) { set_failed("Error: " + werr); cv.notify_all(); throw std::runtime_error("Error: " + werr); }
                    cv.notify_one();
                    continue;
                }
                cv.wait(l);                                           // every buffer is being filled by another thread
            }
            const int i = free_list.back();
            free_list.pop_back();
            l.unlock();
            try { materialize(pool[i]); }
            catch (const std::exception& e) { { std::lock_guard<std::mutex> g(m); free_list.push_back(i); set_failed(e.what()); } cv.notify_all(); throw; }
            ns_wait += (std::chrono::steady_clock::now() - t0).count();
            *c = cap;
            return pool[i].ascii;
        };
        if (device_parse) bs.submit_raw = [this](unsigned, char* buf, size_t len, bool fastq) { submit_buf(buf, len, fastq ? KQ_FASTX_FASTQ : KQ_FASTX_FASTA); };
        bs.submit = [this](unsigned, char* buf, size_t len) { submit_buf(buf, len, 0); };
        // a sequence longer than a pool buffer: a page-locked buffer of its own, submitted like any other and released once
        // its copy has finished (the device side cuts it into slices with overlapping scans: k-mers and edges across a cut
        // are seen exactly once, kreeq_amd.hip count_seq_dev)
        bs.acquire_big = [this](unsigned, size_t n) {
            char* p = (char*)kq_host_alloc(n);
            if (!p) { const std::string why = "read buffer allocation failed (" + std::to_string(n) + " bytes)"; fail(why); throw std::runtime_error(why); }
            return p;
        };
        bs.submit_big = [this](unsigned, char* buf, size_t len) {
            uint64_t tk = 0;
            int rc = len ? kq_count_batch_async(h, buf, len, &tk) : KQ_OK;
            std::string err = rc != KQ_OK ? kq_last_error() : "";
            if (rc == KQ_OK && len) { rc = kq_host_wait(h, tk); if (rc != KQ_OK) err = kq_last_error(); }
            kq_host_free(buf);
            if (rc != KQ_OK) { fail("Error: " + err); throw std::runtime_error("Error: " + err); }
            ++n_submit;
        };
        bs.abort = [this] { fail(); };
        return bs;
    }
};

}  // namespace

void count_reads_file(kq_handle* h, const std::string& path, unsigned threads, uint64_t input_bytes, int device) {
    // buffers of 8-32 MiB: small enough that copies and counting of a 300 MB file overlap its parsing, large enough
    // (>= 7 M k-mers) for the partitioned count path; the pool has a buffer per parser thread up to 16 and 2 to spare
    size_t cap = (size_t)std::min<uint64_t>(32ull << 20, std::max<uint64_t>(8ull << 20, input_bytes / 64));
    threads = std::min(threads, 64u);
    unsigned n_buf = std::min(threads, 16u) + 2;
    if (const char* e = getenv("KQ_INGEST_CAP_MB")) cap = (size_t)atol(e) << 20;      // tuning aids (tools/bench_extra/cli_ingest_*.py)
    if (const char* e = getenv("KQ_INGEST_BUFFERS")) n_buf = (unsigned)std::max(2, atoi(e));
    const bool pack = env_flag("KQ_INGEST_PACK");
    const bool device_parse = env_flag("KQ_INGEST_DEVICE");         // (wins over KQ_INGEST_PACK: the text is packed nowhere, the count reads the parsed batch)
    // A job that knows its size sizes the pending-set arena once (the automatic arena starts small and doubles -- a table
    // pass, a synchronisation and a reallocation every time -- which a 300 MB file pays four or five times): about one k-mer
    // per two input bytes, 5 bytes per record, within half of the free HBM.  Larger inputs just fill it more than once.
    {
        uint64_t free_b = 0, total_b = 0;
        if (kq_device_memory(device, &free_b, &total_b) != KQ_OK) free_b = 8ull << 30;
        uint64_t want = std::max<uint64_t>(256ull << 20, input_bytes * 3);
        if (const char* e = getenv("KQ_CLI_PENDING_MB")) want = (uint64_t)atol(e) << 20;
        if (!getenv("KQ_CLI_PENDING_AUTO")) kq_or_die(kq_set_option(h, KQ_OPT_PENDING_BYTES, (int64_t)std::min<uint64_t>(want, free_b / 2)));
    }
    const auto t00 = std::chrono::steady_clock::now();
    GpuSink gs(h, n_buf, cap, pack, device_parse);
    const auto t0 = std::chrono::steady_clock::now();
    if (device_parse) read_raw_sink(path, threads, gs.sink());
    else read_batches_sink(path, threads, gs.sink());
    const auto t1 = std::chrono::steady_clock::now();
    kq_or_die(kq_flush(h));                                          // everything is enqueued; the table pass may start
    gs.drain();                                                      // the last copies out of the pool have finished before it is released
    if (device_parse) kq_or_die(kq_sync(h));                         // text the device parser refused (malformed FASTQ / FASTA) ends the run here
    if (getenv("KQ_INGEST_TRACE"))
        fprintf(stderr, "ingest: %u threads, %u buffers of %zu MiB, %lld submits, pool %.1f ms, wall %.1f ms + flush %.1f ms; thread-time sums: wait for a buffer %.1f ms, "
                        "pack %.1f ms, submit calls %.1f ms; device-parsed submits %lld\n", threads, n_buf, cap >> 20, (long long)gs.n_submit, (t0 - t00).count() * 1e-6, (t1 - t0).count() * 1e-6,
                (std::chrono::steady_clock::now() - t1).count() * 1e-6, gs.ns_wait * 1e-6, gs.ns_pack * 1e-6, gs.ns_call * 1e-6, (long long)gs.n_dev_submit);
}

// -j, or one parser thread per 32 MB of input within [4, all cores]: the threads take turns submitting (one stream feeds the
// GPU), and on a few hundred MB more of them only queue up behind each other (310 MB FASTQ: 8 threads 26-32 ms, 64: 38 ms)
unsigned parser_threads(const UserInput& ui, uint64_t input_bytes) {
    if (ui.maxThreads > 0) return (unsigned)ui.maxThreads;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    return (unsigned)std::min<uint64_t>(hw, std::max<uint64_t>(4, input_bytes >> 25));
}

}  // namespace kqhost
