#include "bgzf_reader.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <cstring>
#include <stdexcept>

namespace kqhost {

namespace {

// a .gz file mapped read-only, or nothing (a pipe, an empty file, a name without .gz)
struct MappedGz {
    int fd = -1;
    const uint8_t* data = nullptr;
    size_t size = 0;
    explicit MappedGz(const std::string& path) {
        struct stat st;
        if (!has_gz_suffix(path) || stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode) || st.st_size <= 0) return;
        fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) return;
        void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) return;
        data = (const uint8_t*)m; size = (size_t)st.st_size;
        madvise(m, size, MADV_SEQUENTIAL);
    }
    ~MappedGz() { if (data) munmap((void*)data, size); if (fd >= 0) close(fd); }
    MappedGz(const MappedGz&) = delete;
    MappedGz& operator=(const MappedGz&) = delete;
};

// the first byte of a member's text (zlib, raw DEFLATE), or -1 if zlib refuses the member
int first_text_byte(const uint8_t* member, const kq_bgzf_block& b) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return -1;
    unsigned char out[1];
    z.next_in = const_cast<Bytef*>(member + b.data_off); z.avail_in = b.data_len;
    z.next_out = out; z.avail_out = 1;
    const int rc = inflate(&z, Z_SYNC_FLUSH);
    const bool got = (rc == Z_OK || rc == Z_STREAM_END || rc == Z_BUF_ERROR) && z.avail_out == 0;
    inflateEnd(&z);
    return got ? out[0] : -1;
}

}  // namespace

bool read_bgzf_sink(const std::string& path, const BgzfSink& sink) {
    MappedGz f(path);
    if (!f.data || !sink.submit_bgzf || !bgzf_first_member(kq_bgzf_scan, f.data, f.size)) return false;
    std::vector<kq_bgzf_block> members(4096), rebased;
    int fastq = -1;                                        // not known before the first member with text
    size_t pos = 0;
    try {
        while (pos < f.size) {
            size_t cap = 0;
            char* buf = sink.acquire(0, &cap);
            // the members that lie wholly in the next `cap` bytes
            const uint64_t window = std::min<uint64_t>(f.size - pos, cap);
            uint64_t n = 0, used = 0;
            int rc = kq_bgzf_scan(f.data + pos, window, members.data(), members.size(), &n, &used);
            if (n > members.size()) {
                // more members than the list holds: KQ_ERR_CAPACITY, or KQ_ERR_INVALID with that many in front of a foreign member
                members.resize(n);
                rc = kq_bgzf_scan(f.data + pos, window, members.data(), members.size(), &n, &used);
            }
            if (n > members.size()) { sink.submit(0, buf, 0); throw std::runtime_error("Error: " + path + " changed while it was read"); }
            if (!n) {
                sink.submit(0, buf, 0);                        // the buffer goes back empty
                if (rc == KQ_ERR_INVALID) throw std::runtime_error("Error: the gzip member at byte " + std::to_string(pos) + " of " + path + " is not a BGZF block");
                if (cap < BGZF_MAX_MEMBER) throw std::runtime_error("Error: read buffers of " + std::to_string(cap) + " bytes cannot hold a BGZF member");
                throw std::runtime_error("Error: truncated BGZF file " + path + " (the member at byte " + std::to_string(pos) + " does not lie wholly in the file)");
            }
            // (a member behind them that is not BGZF shows in the next round, at its own offset)
            if (fastq < 0) {
                for (uint64_t i = 0; i < n && fastq < 0; ++i)
                    if (members[i].isize) {
                        const int c = first_text_byte(f.data + pos + members[i].off, members[i]);
                        if (c != '@' && c != '>') { sink.submit(0, buf, 0); return false; }      // nothing has been submitted: the host reader reports it
                        fastq = c == '@';
                    }
            }
            if (fastq < 0) { sink.submit(0, buf, 0); pos += used; continue; }      // members without text in front of the first text: nothing to carry yet
            // the window is at most `cap` bytes, so its members are ONE run
            BgzfRun run;
            const int got = bgzf_next_run(members.data(), n, 0, cap, &run, &rebased);
            if (got != BGZF_RUN_OK || run.count != n) {
                sink.submit(0, buf, 0);
                throw std::runtime_error("Error: read buffers of " + std::to_string(cap) + " bytes cannot hold a BGZF member");
            }
            memcpy(buf, f.data + pos + run.off, run.len);
            sink.submit_bgzf(0, buf, run.len, rebased.data(), rebased.size(), fastq == 1, pos + used == f.size);
            pos += used;
        }
    } catch (...) {
        if (sink.abort) sink.abort();
        throw;
    }
    return true;
}

}  // namespace kqhost
