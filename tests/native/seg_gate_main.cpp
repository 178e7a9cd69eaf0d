// Stand-alone check of the gate between the two last split levels (kreeq_amd/csrc/kq_seg_gate_host.h), meant to be built with
// -fsanitize=address,undefined: uniform offsets, one bucket at the threshold and just above it, all records in one bucket, no
// records, empty buckets.  The offset arrays are exactly-sized heap blocks, so a read past entry n_buckets is reported.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kq_seg_gate_host.h"

using namespace kq;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++bad; } } while (0)

// offsets of the given bucket counts, starting at `base`
static std::vector<unsigned long long> offsets(const std::vector<unsigned long long>& counts, unsigned long long base = 0) {
    std::vector<unsigned long long> off(counts.size() + 1);
    off[0] = base;
    for (size_t i = 0; i < counts.size(); ++i) off[i + 1] = off[i] + counts[i];
    return off;
}
static bool gate(const std::vector<unsigned long long>& counts, unsigned long long base = 0) {
    const std::vector<unsigned long long> off = offsets(counts, base);
    return seg_gate_even(off.data(), (uint32_t)counts.size());
}

int main() {
    const uint32_t N = 256;
    // uniform buckets of any size pass, whatever the first offset
    for (unsigned long long c : {1ull, 16ull, 4096ull, 9000000ull, (1ull << 32) / N}) {
        CHECK(gate(std::vector<unsigned long long>(N, c)));
        CHECK(gate(std::vector<unsigned long long>(N, c), 12345));
    }
    // one bucket above the others: largest * N * 16 <= total * 17 decides, exactly
    //   255 buckets of c and one of c + x: passes iff (c + x) * 4096 <= (256 c + x) * 17, i.e. x * 4079 <= 256 c
    for (unsigned long long c : {4079ull, 40790ull, 4079000ull, 15ull * 4079}) {
        const unsigned long long x = 256 * c / 4079;              // the threshold (256 c is a multiple of 4079 here)
        for (uint32_t where : {0u, 1u, 100u, N - 1}) {
            std::vector<unsigned long long> v(N, c);
            v[where] = c + x;
            CHECK(gate(v));
            v[where] = c + x + 1;
            CHECK(!gate(v));
            v[where] = c + x - 1;
            CHECK(gate(v));
        }
    }
    // a bucket exactly 1/16 above the mean of 16 x 17 x 256 records per bucket ...
    {
        const unsigned long long mean = 16 * 17 * 256;
        std::vector<unsigned long long> v(N, mean);
        v[7] = mean + mean / 16;                                    // ... paid for by the others, so that the mean stays
        for (uint32_t i = 8; i < 8 + 16; ++i) v[i] -= mean / 256;
        unsigned long long total = 0;
        for (unsigned long long c : v) total += c;
        CHECK(total == mean * N);
        CHECK(gate(v));
        v[7] += 1; v[30] -= 1;
        CHECK(!gate(v));
    }
    // iid-like noise of a few per mille passes
    {
        std::vector<unsigned long long> v(N);
        for (uint32_t i = 0; i < N; ++i) v[i] = 1000000 + (i * 7919u) % 4001;      // +- 0.2 %
        CHECK(gate(v));
    }
    // every record in one bucket: fails wherever the bucket is; so does half of them
    for (uint32_t where : {0u, 128u, N - 1}) {
        std::vector<unsigned long long> v(N, 0);
        v[where] = 1;
        CHECK(!gate(v));
        v[where] = 3000000000ull;
        CHECK(!gate(v));
        v[(where + 1) % N] = 3000000000ull;
        CHECK(!gate(v));
    }
    // no records at all: every segment is empty, the answer is "even"
    CHECK(gate(std::vector<unsigned long long>(N, 0)));
    CHECK(gate(std::vector<unsigned long long>(N, 0), 99));
    // empty buckets among even ones (a bucket window, a tiny batch): the rest stands above the mean of all 256
    {
        std::vector<unsigned long long> v(N, 1000);
        for (uint32_t i = 0; i < 128; ++i) v[i] = 0;
        CHECK(!gate(v));
        v.assign(N, 1000);
        for (uint32_t i = 0; i < 15; ++i) v[i] = 0;                 // 241 x 1000 over 256: mean 941.4, limit 1000.2
        CHECK(gate(v));
        v[15] = 0;                                                  // 240 x 1000 over 256: mean 937.5, limit 996.1
        CHECK(!gate(v));
    }
    // sizes near the format limit of a slice (< 2^32 records) and far beyond it: no overflow
    CHECK(gate(std::vector<unsigned long long>(N, (1ull << 32) / N - 1)));
    CHECK(gate(std::vector<unsigned long long>(N, 1ull << 55)));
    {
        std::vector<unsigned long long> v(N, 1ull << 55);
        v[3] += (1ull << 55) / 8;
        CHECK(!gate(v));
    }
    // other bucket counts, one bucket, descending offsets, no input
    CHECK(gate(std::vector<unsigned long long>(1, 5)));
    CHECK(gate(std::vector<unsigned long long>(2, 5)));
    CHECK(!gate(std::vector<unsigned long long>{5, 6}));           // 6 * 2 * 16 = 192 > 11 * 17 = 187
    CHECK(gate(std::vector<unsigned long long>{32, 33}));          // 33 * 32 = 1056 <= 65 * 17 = 1105
    {
        const unsigned long long off[3] = {10, 5, 20};
        CHECK(!seg_gate_even(off, 2));
        CHECK(!seg_gate_even(off, 0));
        CHECK(!seg_gate_even(nullptr, 2));
    }
    printf("segment gate: %d failures\n", bad);
    return bad ? 1 : 0;
}
