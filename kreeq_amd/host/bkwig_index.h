// bkwig_index.h -- the index in front of a .bkwig payload (written by DBG::writeIndex, src/kreeq-output.cpp:305-355; read by
// readIndex, src/decompressor.cpp:78-117):
//   u8 k | u32 nPaths | per path: u16 header length, header, u32 nComponents | per component: u64 absPos, u64 len, u8 step
// followed by the payload: 12 bytes (u32 cov, fw, bw) per position, component after component.  Host only, no project header.
#pragma once
#include <cstdint>
#include <istream>
#include <string>
#include <vector>

struct BkwigComponent { uint64_t byte_pos, abs_pos, len; uint8_t step; };          // byte_pos: offset inside the payload
struct BkwigPath { std::string header; std::vector<BkwigComponent> comps; };
struct BkwigIndex {
    uint8_t k = 0;
    std::vector<BkwigPath> paths;                        // in file order
    uint64_t index_bytes = 0;                            // without the k byte (indexByteSize of the reference)
    uint64_t payload_bytes = 0;                          // 12 x the sum of the component lengths
    uint64_t payload_offset() const { return 1 + index_bytes; }
    const BkwigPath* find(const std::string& header) const {
        for (auto& p : paths) if (p.header == header) return &p;
        return nullptr;
    }
};

// false (with `err`) when the stream ends inside the index
inline bool read_bkwig_index(std::istream& in, BkwigIndex& idx, std::string& err) {
    auto get = [&](void* p, size_t n) { in.read((char*)p, (std::streamsize)n); idx.index_bytes += n; return (bool)in; };
    idx = BkwigIndex{};
    in.read((char*)&idx.k, 1);
    uint32_t n_paths = 0;
    if (!in || !get(&n_paths, 4)) { err = "the file ends inside its index"; return false; }
    for (uint32_t i = 0; i < n_paths; ++i) {
        uint16_t hl = 0;
        uint32_t nc = 0;
        BkwigPath path;
        if (!get(&hl, 2)) { err = "the file ends inside its index"; return false; }
        path.header.resize(hl);
        if ((hl && !get(&path.header[0], hl)) || !get(&nc, 4)) { err = "the file ends inside its index"; return false; }
        for (uint32_t c = 0; c < nc; ++c) {
            BkwigComponent comp{idx.payload_bytes, 0, 0, 0};
            if (!get(&comp.abs_pos, 8) || !get(&comp.len, 8) || !get(&comp.step, 1)) { err = "the file ends inside its index"; return false; }
            if (comp.len > (UINT64_MAX - idx.payload_bytes) / 12) { err = "a component length overflows the payload size"; return false; }
            idx.payload_bytes += 12 * comp.len;
            path.comps.push_back(comp);
        }
        idx.paths.push_back(std::move(path));
    }
    return true;
}
