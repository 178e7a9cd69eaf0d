// kq_dbimage_host.h -- the layout of one <db>/.map.<m>.bin (a phmap dump of 256 submaps) as plain host
// C++: sizes, and the header walk of the reader with every bound check.  No HIP, no allocation, no exception: the
// library uses it in front of any device work, and a stand-alone program can run it under sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define KQ_DBI_HD __host__ __device__
#else
#define KQ_DBI_HD
#endif

namespace kq {

constexpr uint32_t DBI_SUBMAPS = 256;                       // PM<T>: N = 8 (reference include/kreeq.h:138-144)
constexpr uint64_t DBI_VERSION = 0xFFFFFFFFFFFFFFF5ull;
constexpr uint32_t DBI_GROUP = 16, DBI_SLOT = 24;           // SSE2 group width; key + DBGkmer (9 B) padded to 8
constexpr uint64_t DBI_EMPTY_FILE = 8 + 24ull * DBI_SUBMAPS;   // 6152: 256 submaps of size 0

KQ_DBI_HD inline uint64_t dbi_growth(uint64_t cap) { return cap - cap / 8; }      // CapacityToGrowth, group width 16
// smallest 2^n - 1 with room for `size` entries (what sequential insertion into a fresh raw_hash_set ends with)
KQ_DBI_HD inline uint64_t dbi_capacity(uint64_t size) {
    if (!size) return 0;
    uint64_t cap = 1;
    while (dbi_growth(cap) < size) cap = cap * 2 + 1;
    return cap;
}
// bytes of one submap in the dump: version, size, capacity [, ctrl[cap + 17], slots[cap], growth_left]
inline uint64_t dbi_submap_bytes(uint64_t size) {
    if (!size) return 24;
    const uint64_t cap = dbi_capacity(size);
    return 24 + (cap + DBI_GROUP + 1) + cap * DBI_SLOT + 8;
}

struct DbiExtent { uint64_t ctrl_off, slot_off, cap, size; };           // of one submap, offsets from the start of the image

// Walks the 256 submap headers of an image of n bytes.  Returns nullptr and fills ext[256] / *total_size when every
// extent lies inside the image and the image ends where the last submap ends; else the reason.
inline const char* dbi_walk(const uint8_t* img, uint64_t n, DbiExtent* ext, uint64_t* total_size) {
    uint64_t off = 0, total = 0;
    auto rd64 = [&](uint64_t* v) { if (n - off < 8) return false; memcpy(v, img + off, 8); off += 8; return true; };
    uint64_t nsub = 0;
    if (!img || !rd64(&nsub)) return "truncated map image";
    if (nsub != DBI_SUBMAPS) return "map image does not hold 256 submaps";
    for (uint32_t s = 0; s < DBI_SUBMAPS; ++s) {
        uint64_t ver = 0, size = 0, cap = 0;
        if (!rd64(&ver) || !rd64(&size) || !rd64(&cap)) return "truncated map image";
        if (ver != DBI_VERSION) return "unexpected phmap dump version in map image";
        ext[s] = DbiExtent{0, 0, 0, 0};
        if (size == 0) continue;
        // cap = 2^n - 1 and size <= cap: both also keep the products below from overflowing
        if (cap == 0 || (cap & (cap + 1)) != 0 || cap >= (1ull << 56) || size > cap) return "inconsistent submap header in map image";
        const uint64_t ctrl_bytes = cap + DBI_GROUP + 1, slot_bytes = cap * DBI_SLOT;
        if (n - off < ctrl_bytes) return "truncated map image";
        ext[s].ctrl_off = off; off += ctrl_bytes;
        if (n - off < slot_bytes) return "truncated map image";
        ext[s].slot_off = off; off += slot_bytes;
        uint64_t growth_left;
        if (!rd64(&growth_left)) return "truncated map image";
        ext[s].cap = cap; ext[s].size = size;
        total += size;
    }
    if (off != n) return "trailing bytes in map image";
    *total_size = total;
    return nullptr;
}

}  // namespace kq
