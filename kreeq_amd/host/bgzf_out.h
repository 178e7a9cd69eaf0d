// bgzf_out.h -- the host side of -o x.{kwig,bed,csvtable}.gz: BGZF members made with zlib (raw deflate per piece of 0xff00 bytes
// of text, the container of the device writer, the same end-of-file marker), as a stream buffer the host writers print into.
#pragma once
#include <zlib.h>

#include <cstdint>
#include <cstring>
#include <ostream>
#include <streambuf>
#include <string>
#include <vector>

namespace kqhost {

constexpr size_t kBgzfText = 0xff00;      // text bytes per member (bgzip's choice)

inline const std::string& bgzf_eof_marker() {
    static const std::string m("\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00", 28);
    return m;
}

// one member for n <= 0xff00 bytes of text; a stored block when deflate does not make it smaller.  Empty string: zlib failed
inline std::string bgzf_member(const char* text, size_t n, int level = 1) {
    std::vector<unsigned char> data(n + 64 + n / 1000);
    size_t len = 0;
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return "";
    z.next_in = (Bytef*)text; z.avail_in = (uInt)n;
    z.next_out = data.data(); z.avail_out = (uInt)data.size();
    const int rc = deflate(&z, Z_FINISH);
    len = z.total_out;
    deflateEnd(&z);
    if (rc != Z_STREAM_END || len >= n + 5) {                      // one stored block: 18 + 5 + n + 8 bytes, so that BSIZE always fits
        data[0] = 1; data[1] = (unsigned char)(n & 0xFF); data[2] = (unsigned char)(n >> 8); data[3] = (unsigned char)(~n & 0xFF); data[4] = (unsigned char)((~n >> 8) & 0xFF);
        if (n) memcpy(data.data() + 5, text, n);
        len = n + 5;
    }
    const uint32_t size = (uint32_t)(18 + len + 8), crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)text, (uInt)n), isize = (uint32_t)n;
    std::string m("\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00", 16);
    m.push_back((char)((size - 1) & 0xFF)); m.push_back((char)((size - 1) >> 8));
    m.append((const char*)data.data(), len);
    for (int i = 0; i < 4; ++i) m.push_back((char)((crc >> (8 * i)) & 0xFF));
    for (int i = 0; i < 4; ++i) m.push_back((char)((isize >> (8 * i)) & 0xFF));
    return m;
}

// what is printed into it leaves as BGZF members through `sink`; finish() writes the last member and the end-of-file marker
class BgzfBuf : public std::streambuf {
    std::ostream& sink_;
    std::vector<char> buf_;
    bool ok_ = true;
    bool flush_member() {
        const size_t n = (size_t)(pptr() - pbase());
        if (n) {
            const std::string m = bgzf_member(pbase(), n);
            if (m.empty()) ok_ = false;
            sink_.write(m.data(), (std::streamsize)m.size());
        }
        setp(buf_.data(), buf_.data() + buf_.size());
        return ok_;
    }
protected:
    int_type overflow(int_type c) override {
        flush_member();
        if (!traits_type::eq_int_type(c, traits_type::eof())) { *pptr() = traits_type::to_char_type(c); pbump(1); }
        return ok_ ? traits_type::not_eof(c) : traits_type::eof();
    }
public:
    explicit BgzfBuf(std::ostream& sink) : sink_(sink), buf_(kBgzfText) { setp(buf_.data(), buf_.data() + buf_.size()); }
    // ends the member in progress (a member boundary where the caller wants one)
    void cut() { flush_member(); }
    bool finish() { flush_member(); sink_.write(bgzf_eof_marker().data(), (std::streamsize)bgzf_eof_marker().size()); sink_.flush(); return ok_ && sink_.good(); }
};

}  // namespace kqhost
