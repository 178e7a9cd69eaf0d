// bgzf_reader.h -- the host side of reading a BGZF file (bgzip / htslib output) for the device inflate: the
// compressed members are handed on as they lie in the file, in runs of whole members that fit a buffer of the ingest pool, so
// that a BGZF stream on the device (kq_count_bgzf_dev's: inflate, cut at record ends, carry, parse) can take them.  What the
// host does is the member walk (kq_bgzf_scan: 18 header bytes per member), one memcpy of the compressed bytes and one zlib
// call on the first member with text, which tells FASTQ from FASTA.
// NOT WIRED INTO THE CLI YET: the library has no entry that takes such a run from page-locked host memory with a ticket, so
// no sink in ingest.cpp sets submit_bgzf and `kreeq` never calls read_bgzf_sink.  tests/test_bgzf_reader_host.py runs it.
//
// The first part of this header is arithmetic only -- no I/O, no HIP, no zlib -- so that a stand-alone host program can run it
// under sanitizers (tests/native/bgzf_reader_main.cpp): which files take the path, and how a member list is cut into runs
// that fit a pool buffer.  The reader itself is declared below and lives in bgzf_reader.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "fastx.h"
#include "kreeq_amd.h"

namespace kqhost {

constexpr uint64_t BGZF_MAX_MEMBER = 65536;      // BSIZE is a u16: no member is larger

inline bool has_gz_suffix(const std::string& path) { return path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0; }

// kq_bgzf_scan, or a function with its contract (the stand-alone test program has no library to link)
using BgzfScanFn = int (*)(const void* data, uint64_t len, kq_bgzf_block* blocks, uint64_t cap, uint64_t* n_blocks, uint64_t* consumed);

// Does the scan accept a first member that lies wholly in [data, data + len)?  Plain single-member gzip (no 'BC' subfield), an
// empty file and a file that ends inside its first member do not: they take the host reader, which reports them as it always has
inline bool bgzf_first_member(BgzfScanFn scan, const void* data, uint64_t len) {
    kq_bgzf_block b;
    uint64_t n = 0, used = 0;
    const int rc = scan(data, std::min<uint64_t>(len, BGZF_MAX_MEMBER), &b, 1, &n, &used);
    return (rc == KQ_OK || rc == KQ_ERR_CAPACITY) && n >= 1;      // (several small members in 64 KiB: more than the one asked for)
}

// A run: the members [first, first + count) of a list, the bytes [off, off + len) of what the list's offsets refer to
struct BgzfRun { uint64_t first = 0, count = 0, off = 0, len = 0; };

enum { BGZF_RUN_NONE = 0, BGZF_RUN_OK = 1, BGZF_RUN_REFUSED = -1 };

// The next run of whole members from `cursor` on that fits `capacity` bytes: as many as fit, in list order.  `members` is the
// list of a file or of a piece of it (consecutive members: each begins where the one before ends); `rebased` receives the run's
// members with offsets relative to the run's first byte, which is what the device entries take beside the copied bytes.
// A capacity below one maximal member is refused (a run could be empty); with it, a run is never empty while members remain.
// Members without text (ISIZE 0, the EOF marker among them) are members like any other: they travel with their neighbours.
inline int bgzf_next_run(const kq_bgzf_block* members, uint64_t n_members, uint64_t cursor, uint64_t capacity, BgzfRun* run, std::vector<kq_bgzf_block>* rebased) {
    if (capacity < BGZF_MAX_MEMBER) return BGZF_RUN_REFUSED;
    *run = BgzfRun{};
    rebased->clear();
    if (cursor >= n_members) return BGZF_RUN_NONE;
    run->first = cursor;
    run->off = members[cursor].off;
    uint64_t i = cursor;
    while (i < n_members && run->len + members[i].size <= capacity) {
        kq_bgzf_block b = members[i];
        b.off = run->len;
        rebased->push_back(b);
        run->len += members[i].size;
        ++i;
    }
    run->count = i - cursor;
    return BGZF_RUN_OK;
}

// ---- the reader (bgzf_reader.cpp) -------------------------------------------------------------------------------------------

//   submit_bgzf(thread, buf, len, blocks, n_blocks, fastq, last)   buf (from acquire) holds len bytes of whole members, `blocks`
//                             lists them with offsets relative to buf; `last`: the file ends with this run (KQ_BGZF_END)
//                             (the sink owns buf again)
// The runs of a file are submitted in file order by the calling thread: the stream on the device has a carry.
struct BgzfSink : RawSink {
    std::function<void(unsigned thread, char* buf, size_t len, const kq_bgzf_block* blocks, uint64_t n_blocks, bool fastq, bool last)> submit_bgzf;
};

// Maps the file, walks its members piecewise (kq_bgzf_scan), copies run after run into buffers from sink.acquire and hands them to
// sink.submit_bgzf.  Returns false, with nothing submitted, for a file that does not take this path: no .gz name, not
// mappable, a first member that is not BGZF, or a first byte of text other than '@' and '>' -- the caller reads it on the host.
// Throws std::runtime_error for a later member that is not BGZF (with its byte offset) and for a file that ends inside a member
// ("truncated BGZF file"), after sink.abort().
bool read_bgzf_sink(const std::string& path, const BgzfSink& sink);

}  // namespace kqhost
