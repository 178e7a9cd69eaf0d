// kq_bgzf_host.h -- the block walk of a BGZF file (the block-gzip container of bgzip / htslib: multi-member gzip whose members
// carry their own compressed size).  Host only, no HIP or project header: g++ reads this file as it is (the ABI's kq_bgzf_scan in
// kreeq_amd.hip and tests/native/inflate_core_main.cpp both call kqbgzf::scan).
//
// One member:   0  ID1 ID2 CM FLG = 1f 8b 08 04      4  MTIME XFL OS (6 bytes, not looked at)      10  XLEN (u16)
//              12  XLEN bytes of extra subfields {SI1 SI2 SLEN(u16) data}: one of them is 'B' 'C' 2 BSIZE(u16), BSIZE = size - 1
//       12 + XLEN  the raw DEFLATE stream, data_len = size - XLEN - 20 bytes
//        size - 8  CRC-32 (u32) and ISIZE (u32) of the member's text, ISIZE <= 65536
// Every read is checked against `len` before it is made.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace kqbgzf {

constexpr int OK = 0, ERR_INVALID = -1, ERR_CAPACITY = -6;      // == KQ_OK / KQ_ERR_INVALID / KQ_ERR_CAPACITY
constexpr uint32_t MAX_ISIZE = 65536;

struct Block { uint64_t off; uint32_t size; uint32_t data_off; uint32_t data_len; uint32_t crc32; uint32_t isize; };      // == kq_bgzf_block

inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t rd32(const uint8_t* p) { return rd16(p) | (rd16(p + 2) << 16); }

// Walks members from data[0].  Stops at the first member that does not lie wholly inside len: *consumed = its offset, OK (a caller
// feeds a file piecewise).  A member that is not BGZF: ERR_INVALID, *consumed = its offset, *n_blocks = the blocks before it.
// More than cap blocks: ERR_CAPACITY, *n_blocks = the number needed (blocks may be NULL with cap 0), *consumed as for OK.
inline int scan(const void* data, uint64_t len, Block* blocks, uint64_t cap, uint64_t* n_blocks, uint64_t* consumed) {
    const uint8_t* d = (const uint8_t*)data;
    uint64_t pos = 0, n = 0;
    int rc = OK;
    while (len - pos >= 4) {
        const uint8_t* m = d + pos;
        if (m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || m[3] != 4) { rc = ERR_INVALID; break; }
        if (len - pos < 12) break;                                      // XLEN is not here yet
        const uint32_t xlen = rd16(m + 10);
        if (len - pos < 12ull + xlen) break;                            // the extra field is not all here yet
        uint32_t bsize = 0; bool found = false;
        for (uint32_t x = 0; x + 4 <= xlen;) {                          // (x + 4 + slen <= xlen is checked before the subfield is used)
            const uint8_t* s = m + 12 + x;
            const uint32_t slen = rd16(s + 2);
            if (x + 4 + slen > xlen) break;
            if (s[0] == 'B' && s[1] == 'C' && slen == 2 && !found) { bsize = rd16(s + 4); found = true; }
            x += 4 + slen;
        }
        if (!found) { rc = ERR_INVALID; break; }
        const uint32_t size = bsize + 1;
        if (size < xlen + 20) { rc = ERR_INVALID; break; }              // header 12 + XLEN, trailer 8: data_len would be negative
        if (len - pos < size) break;                                    // the member is not all here yet
        const uint32_t isize = rd32(m + size - 4);
        if (isize > MAX_ISIZE) { rc = ERR_INVALID; break; }
        if (n < cap && blocks) {
            Block b;
            b.off = pos; b.size = size; b.data_off = 12 + xlen; b.data_len = size - xlen - 20; b.crc32 = rd32(m + size - 8); b.isize = isize;
            blocks[n] = b;
        }
        ++n;
        pos += size;
    }
    if (n_blocks) *n_blocks = n;
    if (consumed) *consumed = pos;
    if (rc == OK && n > cap) return ERR_CAPACITY;
    return rc;
}

}  // namespace kqbgzf
