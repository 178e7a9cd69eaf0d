// kq_export_host.h -- how a result leaves the device (copy_out_bounced of kreeq_amd.hip): in one copy, or in chunks through two
// pinned bounce buffers.  The arithmetic (bounced or direct, how many chunks, the length and the buffer of chunk c) and the
// double-buffer loop itself, with the copy, the synchronisation and the host read as parameters: kreeq_amd.hip passes the HIP
// calls, tests/native/export_plan_main.cpp passes host stand-ins that keep a state per buffer, and both run the same loop.
// Host only; includes nothing from HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define KQ_EXPORT_HD __host__ __device__
#else
#define KQ_EXPORT_HD
#endif

namespace kq {

// The two conditions of k_export (kq_kernels.h), stated once for the kernel and for the host program that runs them against
// buffers of exact size: an entry of map m belongs to the range [lo, hi), and the entry whose place in the list is o is
// written when the buffer of `cap` entries has that place (the count goes on past it: the caller learns the size it needs).
KQ_EXPORT_HD inline bool export_in_range(uint32_t m, uint32_t lo, uint32_t hi) { return m >= lo && m < hi; }
KQ_EXPORT_HD inline bool export_has_place(uint64_t o, uint64_t cap) { return o < cap; }

constexpr size_t EXPORT_CHUNK = (size_t)16 << 20;      // one bounce buffer
constexpr size_t EXPORT_DIRECT_CHUNKS = 4;             // up to this many chunks' worth of bytes go out in one copy
constexpr size_t EXPORT_TEST_CHUNK = 4096;             // KQ_OPT_TEST_EXPORT bit 1: no multiple of sizeof(kq_entry) = 48, so entries straddle chunks

struct BouncePlan {
    size_t bytes = 0, chunk = EXPORT_CHUNK;
    bool bounced = false;          // false: one copy of `bytes`
    size_t n_chunks = 0;           // (bounced only)
    size_t offset_of(size_t c) const { return c * chunk; }
    size_t len_of(size_t c) const { return std::min(chunk, bytes - c * chunk); }       // c < n_chunks: in (0, chunk]
    static int buffer_of(size_t c) { return (int)(c & 1); }
};

// `always`: chunks at any size but 0 (tests); else only above EXPORT_DIRECT_CHUNKS chunks
inline BouncePlan bounce_plan(size_t bytes, size_t chunk = EXPORT_CHUNK, bool always = false) {
    BouncePlan p;
    p.bytes = bytes;
    p.chunk = chunk;
    p.bounced = chunk != 0 && (always ? bytes != 0 : bytes > EXPORT_DIRECT_CHUNKS * chunk);
    p.n_chunks = p.bounced ? (bytes + chunk - 1) / chunk : 0;
    return p;
}

// The loop of a bounced plan.  copy_async(buffer, source offset, length) starts the copy of a chunk into a bounce buffer, sync()
// waits for every copy started, deliver(destination offset, buffer, length) is the host's read of a buffer.  The copy of chunk
// c + 1 is in flight during the host read of chunk c; a buffer is written again only after its last chunk was delivered, and
// delivered only after the sync that follows its copy succeeded.  The loop ends at the first error; -> that error, or `ok`
template <class Err, class CopyAsync, class Sync, class Deliver>
Err bounce_copy(const BouncePlan& p, Err ok, CopyAsync&& copy_async, Sync&& sync, Deliver&& deliver) {
    Err e = copy_async(BouncePlan::buffer_of(0), p.offset_of(0), p.len_of(0));
    for (size_t c = 0; c < p.n_chunks && e == ok; ++c) {
        e = sync();
        if (e != ok) break;
        if (c + 1 < p.n_chunks) e = copy_async(BouncePlan::buffer_of(c + 1), p.offset_of(c + 1), p.len_of(c + 1));
        deliver(p.offset_of(c), BouncePlan::buffer_of(c), p.len_of(c));
    }
    if (e == ok) e = sync();
    return e;
}

}  // namespace kq
