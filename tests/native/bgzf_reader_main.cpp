// The GPU-free part of the BGZF reader (kreeq_amd/host/bgzf_reader.h) as a stand-alone host program: the cutter of a member list
// into runs that fit a buffer, and the test that decides whether a file takes the device path.  The block walk is
// kqbgzf::scan (kreeq_amd/csrc/kq_bgzf_host.h), which is what the library's kq_bgzf_scan calls.
//   bgzf_reader cut FILE CAPACITY...   -> per capacity "cap C runs R members M bytes B" or "cap C refused"
//   bgzf_reader first FILE             -> "first 0" / "first 1"
//   bgzf_reader read FILE CAPACITY     -> the reader itself (bgzf_reader.cpp, linked in, with kq_bgzf_scan defined here) into a sink of
//                                         heap buffers of exactly CAPACITY bytes: per submit "run len L blocks N text T fastq F last E",
//                                         then "fallback" (the file does not take the path), "done" or "error: MESSAGE"
// then "<n> failures".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "bgzf_reader.h"
#include "kq_bgzf_host.h"

using namespace kqhost;

static_assert(sizeof(kq_bgzf_block) == sizeof(kqbgzf::Block), "kq_bgzf_block is kqbgzf::Block");

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static int scan(const void* data, uint64_t len, kq_bgzf_block* blocks, uint64_t cap, uint64_t* n_blocks, uint64_t* consumed) {
    return kqbgzf::scan(data, len, reinterpret_cast<kqbgzf::Block*>(blocks), cap, n_blocks, consumed);
}

extern "C" int kq_bgzf_scan(const void* data, uint64_t len, kq_bgzf_block* blocks, uint64_t cap, uint64_t* n_blocks, uint64_t* consumed) {
    return scan(data, len, blocks, cap, n_blocks, consumed);
}

// the file in a heap array of exactly its size: a read behind it is the sanitizer's
static uint8_t* read_file(const char* path, size_t* size) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    *size = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* d = (uint8_t*)malloc(*size ? *size : 1);
    if (*size && fread(d, 1, *size, f) != *size) { perror(path); exit(2); }
    fclose(f);
    return d;
}

static void cut(const std::vector<kq_bgzf_block>& m, uint64_t cap) {
    BgzfRun run;
    std::vector<kq_bgzf_block> rebased;
    if (cap < BGZF_MAX_MEMBER) {
        CHECK(bgzf_next_run(m.data(), m.size(), 0, cap, &run, &rebased) == BGZF_RUN_REFUSED, "capacity %llu was not refused", (unsigned long long)cap);
        printf("cap %llu refused\n", (unsigned long long)cap);
        return;
    }
    uint64_t cursor = 0, runs = 0, bytes = 0;
    for (;;) {
        const int rc = bgzf_next_run(m.data(), m.size(), cursor, cap, &run, &rebased);
        if (cursor >= m.size()) { CHECK(rc == BGZF_RUN_NONE && run.count == 0 && rebased.empty(), "a run behind the last member"); break; }
        CHECK(rc == BGZF_RUN_OK, "rc %d at member %llu", rc, (unsigned long long)cursor);
        if (rc != BGZF_RUN_OK) break;
        // never empty, in order, contiguous, within the capacity
        CHECK(run.count >= 1, "empty run at member %llu", (unsigned long long)cursor);
        CHECK(run.first == cursor && run.off == m[cursor].off, "run starts at member %llu, byte %llu", (unsigned long long)run.first, (unsigned long long)run.off);
        CHECK(run.len <= cap, "run of %llu bytes, capacity %llu", (unsigned long long)run.len, (unsigned long long)cap);
        CHECK(rebased.size() == run.count, "%zu rebased members, %llu in the run", rebased.size(), (unsigned long long)run.count);
        uint64_t at = 0;
        for (uint64_t i = 0; i < run.count && i < rebased.size(); ++i) {
            const kq_bgzf_block& a = m[cursor + i];
            const kq_bgzf_block& b = rebased[i];
            CHECK(b.off == at && a.off == run.off + at, "member %llu: rebased offset %llu, expected %llu", (unsigned long long)(cursor + i), (unsigned long long)b.off, (unsigned long long)at);
            CHECK(b.size == a.size && b.data_off == a.data_off && b.data_len == a.data_len && b.crc32 == a.crc32 && b.isize == a.isize, "member %llu changed", (unsigned long long)(cursor + i));
            at += a.size;
        }
        CHECK(at == run.len, "run length %llu, members %llu", (unsigned long long)run.len, (unsigned long long)at);
        // as many as fit: the next member would not have
        const uint64_t next = cursor + run.count;
        if (next < m.size()) CHECK(run.len + m[next].size > cap, "member %llu would have fitted", (unsigned long long)next);
        cursor = next; bytes += run.len; ++runs;
    }
    printf("cap %llu runs %llu members %llu bytes %llu\n", (unsigned long long)cap, (unsigned long long)runs, (unsigned long long)cursor, (unsigned long long)bytes);
}

// every submitted run is the next piece of the file, its list is what a scan of the buffer finds, and only the final one is `last`
static void read_through(const char* path, const uint8_t* data, size_t size, size_t cap) {
    size_t at = 0, held = 0;
    bool seen_last = false;
    BgzfSink sink;
    sink.acquire = [&](unsigned, size_t* c) { CHECK(held == 0, "two buffers held at once"); ++held; *c = cap; return (char*)malloc(cap); };
    sink.submit = [&](unsigned, char* buf, size_t len) { CHECK(len == 0, "text submitted by the BGZF reader"); --held; free(buf); };
    sink.submit_bgzf = [&](unsigned, char* buf, size_t len, const kq_bgzf_block* blocks, uint64_t n_blocks, bool fastq, bool last) {
        CHECK(!seen_last, "a run behind the last one");
        CHECK(len >= 1 && len <= cap && n_blocks >= 1, "run of %zu bytes, %llu members", len, (unsigned long long)n_blocks);
        // members without text in front of the first text are dropped, nothing else is
        while (at + len <= size && memcmp(buf, data + at, len) != 0 && at + 28 <= size && data[at + 16] == 27 && data[at + 17] == 0) at += 28;
        CHECK(at + len <= size && memcmp(buf, data + at, len) == 0, "the run is not the file's bytes at %zu", at);
        std::vector<kq_bgzf_block> found(n_blocks);
        uint64_t n = 0, used = 0, text = 0;
        const int rc = scan(buf, len, found.data(), n_blocks, &n, &used);
        CHECK(rc == KQ_OK && n == n_blocks && used == len, "scan of the run: rc %d, %llu members, %llu of %zu bytes", rc, (unsigned long long)n, (unsigned long long)used, len);
        for (uint64_t i = 0; i < n_blocks && i < n; ++i) {
            const kq_bgzf_block &a = found[i], &b = blocks[i];                  // (field by field: the struct ends in padding)
            CHECK(a.off == b.off && a.size == b.size && a.data_off == b.data_off && a.data_len == b.data_len && a.crc32 == b.crc32 && a.isize == b.isize, "member %llu of the run differs from the scan's", (unsigned long long)i);
            text += blocks[i].isize;
        }
        at += len;
        seen_last = last;
        printf("run len %zu blocks %llu text %llu fastq %d last %d\n", len, (unsigned long long)n_blocks, (unsigned long long)text, (int)fastq, (int)last);
        --held; free(buf);
    };
    bool aborted = false;
    sink.abort = [&] { aborted = true; };
    try {
        const bool taken = read_bgzf_sink(path, sink);
        if (taken) CHECK((at == 0 || (seen_last && at == size)) && !aborted, "stopped at byte %zu of %zu, last %d", at, size, (int)seen_last);
        else CHECK(at == 0 && !aborted, "runs were submitted before the file was given up");
        printf(taken ? "done\n" : "fallback\n");
    } catch (const std::exception& e) {
        CHECK(aborted && !seen_last, "abort() %d, last %d", (int)aborted, (int)seen_last);
        printf("error: %s\n", e.what());
    }
    CHECK(held == 0, "%zu buffers not handed back", held);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: bgzf_reader cut FILE CAPACITY... | first FILE | read FILE CAPACITY\n"); return 2; }
    size_t size = 0;
    uint8_t* data = read_file(argv[2], &size);
    if (!strcmp(argv[1], "first")) {
        printf("first %d\n", (int)bgzf_first_member(scan, data, size));
    } else if (!strcmp(argv[1], "read")) {
        if (argc < 4) return 2;
        read_through(argv[2], data, size, (size_t)strtoull(argv[3], nullptr, 10));
    } else {
        uint64_t n = 0, used = 0;
        int rc = scan(data, size, nullptr, 0, &n, &used);
        std::vector<kq_bgzf_block> m(n);
        if (n) rc = scan(data, size, m.data(), n, &n, &used);
        CHECK(rc == KQ_OK && used == size, "scan: rc %d, %llu of %zu bytes", rc, (unsigned long long)used, size);
        for (int a = 3; a < argc; ++a) cut(m, strtoull(argv[a], nullptr, 10));
    }
    free(data);
    printf("%d failures\n", failures);
    return failures != 0;
}
