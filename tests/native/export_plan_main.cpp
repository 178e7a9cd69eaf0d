// Stand-alone check of how results leave the device (kreeq_amd/csrc/kq_export_host.h), meant to be built with
// -fsanitize=address,undefined.  (a) the plan: bounced or direct, chunk count and chunk lengths at the library's own chunk size,
// written out by hand.  (b) the double-buffer loop of copy_out_bounced, the SAME template the library instantiates with the HIP
// calls, run with host stand-ins: the "device" source, the destination and the two bounce buffers are heap blocks of exactly
// their size (a chunk one byte too long is a heap overflow), a copy only takes effect at the next sync (until then the buffer
// holds a poison pattern), and every buffer has a state: free -> copy pending -> ready -> free.  A copy into a buffer that is
// not free overwrites a chunk nobody read; a read of a buffer that is not ready reads a chunk whose copy was not waited for.
// (c) k_export's two conditions, over a list written into a buffer of exactly `cap` entries.
// `export_plan plan BYTES...` prints the library's plan of each byte count instead: "bytes bounced chunks last_length"
// (`testplan`: the plan under KQ_OPT_TEST_EXPORT bit 1).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "kq_export_host.h"

using namespace kq;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad < 50) fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++bad; } } while (0)

constexpr size_t MiB = (size_t)1 << 20, ENTRY = 48;

// ---- (a) the plan at the library's chunk size --------------------------------------------------------------------------
static void plan_table() {
    CHECK(EXPORT_CHUNK == 16 * MiB && EXPORT_DIRECT_CHUNKS == 4 && EXPORT_TEST_CHUNK == 4096 && EXPORT_TEST_CHUNK % ENTRY != 0);
    struct { size_t bytes; bool bounced; size_t n_chunks, last; } rows[] = {
        {0, false, 0, 0}, {1, false, 0, 0}, {ENTRY, false, 0, 0}, {64 * MiB - 1, false, 0, 0}, {64 * MiB, false, 0, 0}, {64 * MiB + 1, true, 5, 1},
        {1048576 * ENTRY, false, 0, 0},                      // 48 MiB: three chunks' worth, in one copy
        {1398101 * ENTRY, false, 0, 0},                      // 64 MiB - 16: the largest whole number of entries that goes direct
        {1398102 * ENTRY, true, 5, 32},                      // 64 MiB + 32
        {2097152 * ENTRY, true, 6, 16 * MiB},                // 96 MiB: six full chunks
        {2097152 * ENTRY + ENTRY, true, 7, ENTRY}, {2097152 * ENTRY - ENTRY, true, 6, 16 * MiB - ENTRY}, {80 * MiB, true, 5, 16 * MiB}};
    for (auto& r : rows) {
        const BouncePlan p = bounce_plan(r.bytes);
        CHECK(p.bytes == r.bytes && p.chunk == EXPORT_CHUNK && p.bounced == r.bounced && p.n_chunks == r.n_chunks);
        if (p.bounced) CHECK(p.len_of(p.n_chunks - 1) == r.last && p.len_of(0) == EXPORT_CHUNK && p.offset_of(p.n_chunks - 1) + r.last == r.bytes);
    }
    // the test chunk: at any size but 0
    CHECK(!bounce_plan(0, EXPORT_TEST_CHUNK, true).bounced && bounce_plan(1, EXPORT_TEST_CHUNK, true).n_chunks == 1 && bounce_plan(ENTRY * 256, EXPORT_TEST_CHUNK, true).n_chunks == 3);
    CHECK(bounce_plan(4096, EXPORT_TEST_CHUNK, true).n_chunks == 1 && bounce_plan(4097, EXPORT_TEST_CHUNK, true).n_chunks == 2 && bounce_plan(4097, EXPORT_TEST_CHUNK, true).len_of(1) == 1);
    CHECK(BouncePlan::buffer_of(0) == 0 && BouncePlan::buffer_of(1) == 1 && BouncePlan::buffer_of(2) == 0 && BouncePlan::buffer_of(7) == 1);
}

// ---- (b) the loop with host stand-ins ----------------------------------------------------------------------------------
static uint64_t n_runs = 0, n_chunks_run = 0;
static unsigned char pattern(size_t i, uint32_t seed) { return (unsigned char)((i * 2654435761u + seed) >> 11 ^ (i >> 3)); }

struct Sim {
    enum State { FREE, PENDING, READY };
    size_t bytes, chunk;
    std::unique_ptr<unsigned char[]> src, dst, buf[2];      // exactly bytes, bytes, chunk, chunk
    State st[2] = {FREE, FREE};
    size_t off[2] = {0, 0}, len[2] = {0, 0};
    std::vector<unsigned char> delivered;                  // times each destination byte was written
    size_t n_copy = 0, n_sync = 0, n_deliver = 0, n_overlapped = 0;
    long fail_copy_at = -1, fail_sync_at = -1;              // the call (counted from 0) that reports an error, -1: none

    Sim(size_t bytes_, size_t chunk_, uint32_t seed) : bytes(bytes_), chunk(chunk_), src(new unsigned char[bytes_]), dst(new unsigned char[bytes_]), delivered(bytes_, 0) {
        for (int b = 0; b < 2; ++b) { buf[b].reset(new unsigned char[chunk]); memset(buf[b].get(), 0xEE, chunk); }
        for (size_t i = 0; i < bytes; ++i) { src[i] = pattern(i, seed); dst[i] = 0x5A; }
    }
    int copy_async(int b, size_t o, size_t l) {
        if ((long)n_copy++ == fail_copy_at) return 1;
        CHECK(b == 0 || b == 1);
        CHECK(st[b] == FREE);                               // else: a buffer overwritten before it was read
        CHECK(l > 0 && l <= chunk && o + l <= bytes);
        memset(buf[b].get(), 0xEE, chunk);                  // what was there is gone from now on
        st[b] = PENDING; off[b] = o; len[b] = l;
        return 0;
    }
    int sync() {
        if ((long)n_sync++ == fail_sync_at) return 1;
        for (int b = 0; b < 2; ++b)
            if (st[b] == PENDING) { memcpy(buf[b].get(), src.get() + off[b], len[b]); st[b] = READY; }      // the sanitizer holds off[b] + len[b] to the source
        return 0;
    }
    void deliver(size_t o, int b, size_t l) {
        ++n_deliver;
        CHECK(st[b] == READY);                              // else: a chunk read before its copy was synced
        CHECK(o == off[b] && l == len[b]);
        if (st[b ^ 1] == PENDING) ++n_overlapped;           // the next chunk's copy is in flight during this read
        memcpy(dst.get() + o, buf[b].get(), l);             // the sanitizer holds o + l to the destination
        for (size_t i = o; i < o + l; ++i) ++delivered[i];
        st[b] = FREE;
    }
    int run(const BouncePlan& p) {
        return bounce_copy(p, 0, [&](int b, size_t o, size_t l) { return copy_async(b, o, l); }, [&]() { return sync(); }, [&](size_t o, int b, size_t l) { deliver(o, b, l); });
    }
};

static void run_case(size_t bytes, size_t chunk, uint32_t seed) {
    ++n_runs;
    for (bool always : {true, false}) {
        const BouncePlan p = bounce_plan(bytes, chunk, always);
        CHECK(p.bounced == (always ? bytes != 0 : bytes > 4 * chunk));
        Sim s(bytes, chunk, seed);
        if (!p.bounced) {                                   // one copy
            CHECK(p.n_chunks == 0);
            if (bytes) memcpy(s.dst.get(), s.src.get(), bytes);
            CHECK(memcmp(s.dst.get(), s.src.get(), bytes) == 0);
            continue;
        }
        size_t sum = 0;
        for (size_t c = 0; c < p.n_chunks; ++c) { CHECK(p.len_of(c) > 0 && p.len_of(c) <= chunk && (c + 1 == p.n_chunks || p.len_of(c) == chunk) && p.offset_of(c) == sum); sum += p.len_of(c); }
        CHECK(sum == bytes && p.n_chunks == (bytes + chunk - 1) / chunk);
        CHECK(s.run(p) == 0);
        n_chunks_run += p.n_chunks;
        CHECK(s.n_copy == p.n_chunks && s.n_deliver == p.n_chunks && s.n_sync == p.n_chunks + 1 && s.n_overlapped == p.n_chunks - 1);
        CHECK(s.st[0] == Sim::FREE && s.st[1] == Sim::FREE);
        CHECK(memcmp(s.dst.get(), s.src.get(), bytes) == 0);
        for (size_t i = 0; i < bytes; ++i) if (s.delivered[i] != 1) { CHECK(!"every destination byte is written once"); break; }
    }
}

// an error ends the loop: nothing is copied or read after it, what was delivered before it is right, the rest is untouched
static void run_failures(size_t bytes, size_t chunk) {
    const BouncePlan p = bounce_plan(bytes, chunk, true);
    for (int kind = 0; kind < 2; ++kind)
        for (long at = 0; at <= (long)p.n_chunks - kind; ++at) {
            Sim s(bytes, chunk, 99);
            (kind ? s.fail_copy_at : s.fail_sync_at) = at;
            CHECK(s.run(p) == 1);
            CHECK((kind ? s.n_copy : s.n_sync) == (size_t)at + 1);
            // a failed sync at call j (the wait for chunk j; call n_chunks is the closing one) and a failed copy at call j (chunk j,
            // started after the wait for chunk j - 1) both leave chunks [0, j) delivered
            const size_t done = std::min((size_t)at, p.n_chunks);
            CHECK(s.n_deliver == done);
            const size_t upto = std::min(bytes, done * chunk);
            CHECK(memcmp(s.dst.get(), s.src.get(), upto) == 0);
            for (size_t i = upto; i < bytes; ++i) if (s.dst[i] != 0x5A) { CHECK(!"bytes behind the error stay as they were"); break; }
        }
}

static void loop_cases() {
    uint32_t seed = 1;
    for (size_t chunk : {(size_t)1, (size_t)7, (size_t)48, (size_t)64, (size_t)100, (size_t)4096, (size_t)4099}) {
        for (size_t bytes : {(size_t)0, (size_t)1, ENTRY, 4 * chunk, 4 * chunk + 1, 4 * chunk + ENTRY, 5 * chunk - 1, 5 * chunk, 6 * chunk, 6 * chunk + ENTRY, 6 * chunk - 1, 6 * chunk + 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1})
            run_case(bytes, chunk, seed++);
        if (6 * chunk >= ENTRY) run_case(6 * chunk - ENTRY, chunk, seed++);
    }
    std::mt19937_64 rng(20240611);
    for (int i = 0; i < 400; ++i) {
        const size_t chunk = 1 + rng() % (i % 4 == 0 ? 5000 : 97);
        run_case(rng() % (12 * chunk + 3), chunk, seed++);
    }
    for (int i = 0; i < 40; ++i) run_case(ENTRY * (rng() % 3000), EXPORT_TEST_CHUNK, seed++);          // whole entries through the test chunk
    for (size_t chunk : {(size_t)48, (size_t)100})
        for (size_t bytes : {(size_t)1, chunk, 4 * chunk + 1, 6 * chunk}) run_failures(bytes, chunk);
}

// ---- (c) k_export's conditions -----------------------------------------------------------------------------------------
static void export_conditions() {
    // the filter: every map of a partition of [0, map_count) is taken by exactly one range
    for (uint32_t map_count : {1u, 3u, 128u})
        for (uint32_t cut1 = 0; cut1 <= map_count; ++cut1)
            for (uint32_t cut2 = cut1; cut2 <= map_count; cut2 += (map_count > 8 ? 7 : 1)) {
                const uint32_t cuts[4] = {0, cut1, cut2, map_count};
                for (uint32_t m = 0; m < map_count; ++m) {
                    int taken = 0;
                    for (int r = 0; r < 3; ++r) taken += export_in_range(m, cuts[r], cuts[r + 1]);
                    CHECK(taken == 1);
                }
                CHECK(!export_in_range(cut1, cut1, cut1) && !export_in_range(map_count, 0, map_count));
            }
    // the guard: n entries listed into a buffer of exactly `cap`: the first min(n, cap) places are written, the count is n
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)1024, (uint64_t)1025})
        for (uint64_t cap : {(uint64_t)0, (uint64_t)1, n ? n - 1 : n, n, n + 7}) {
            std::unique_ptr<uint64_t[]> out(new uint64_t[cap]);
            for (uint64_t i = 0; i < cap; ++i) out[i] = ~0ull;
            uint64_t listed = 0;
            for (uint64_t o = 0; o < n; ++o, ++listed)
                if (export_has_place(o, cap)) out[o] = o;      // the sanitizer holds o to the buffer
            CHECK(listed == n);
            for (uint64_t i = 0; i < cap; ++i) CHECK(out[i] == (i < n ? i : ~0ull));
        }
}

int main(int argc, char** argv) {
    if (argc >= 2 && (!strcmp(argv[1], "plan") || !strcmp(argv[1], "testplan"))) {
        const bool test = !strcmp(argv[1], "testplan");
        for (int i = 2; i < argc; ++i) {
            const BouncePlan p = bounce_plan((size_t)strtoull(argv[i], nullptr, 10), test ? EXPORT_TEST_CHUNK : EXPORT_CHUNK, test);
            printf("%zu %d %zu %zu\n", p.bytes, (int)p.bounced, p.n_chunks, p.bounced ? p.len_of(p.n_chunks - 1) : p.bytes);
        }
        return 0;
    }
    plan_table();
    loop_cases();
    export_conditions();
    printf("export plan: %llu byte counts, %llu chunks, %d failures\n", (unsigned long long)n_runs, (unsigned long long)n_chunks_run, bad);
    return bad ? 1 : 0;
}
