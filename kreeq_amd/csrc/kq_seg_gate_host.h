// kq_seg_gate_host.h -- which last split level a slice of 5-byte records takes (sort_to_regions in kreeq_amd.hip): the kernel with one
// workgroup per sub-bucket segment (k_lv_segment_s in kq_kernels.h) or the unit path, which cuts a segment into units of P2_UNIT records.
// A workgroup per segment has a long tail when one sub-bucket is hot (a satellite repeat), so the segment kernel is for slices whose 256
// hash-prefix buckets are even: the offsets P1 made of them are read back with the record count of a filtered pass anyway.
// Host arithmetic only, no device code, so that it can be exercised by a stand-alone program (tests/native/seg_gate_main.cpp).
#pragma once
#include <cstdint>

namespace kq {

constexpr uint32_t SEG_GATE_DIV = 16;            // a bucket may hold mean / 16 more than the mean

// off[0 .. n_buckets]: ascending offsets of the buckets' records.  True when the largest bucket holds at most 1/16 more than the mean:
// for hashed k-mers a bucket's sigma is below 0.1 % of its size, so an ordinary slice passes by a wide margin, and a slice that passes
// can hide at most a sixteenth of a mean bucket of excess in one sub-bucket (four mean segments at 64 sub-buckets per bucket).
// No records: true (every segment is empty, either path only writes offsets).  Offsets that descend: false.
inline bool seg_gate_even(const unsigned long long* off, uint32_t n_buckets) {
    if (off == nullptr || n_buckets == 0) return false;
    unsigned long long largest = 0;
    for (uint32_t b = 0; b < n_buckets; ++b) {
        if (off[b + 1] < off[b]) return false;
        const unsigned long long c = off[b + 1] - off[b];
        if (c > largest) largest = c;
    }
    const unsigned long long total = off[n_buckets] - off[0];
    // largest <= (total / n) * (1 + 1 / DIV)  <=>  largest * n * DIV <= total * (DIV + 1), in 128 bits: no rounding, no overflow
    return (unsigned __int128)largest * n_buckets * SEG_GATE_DIV <= (unsigned __int128)total * (SEG_GATE_DIV + 1);
}

}  // namespace kq
