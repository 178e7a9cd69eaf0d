// Stand-alone check of the offset-matrix geometry (kreeq_amd/csrc/kq_roff_host.h), meant to be built with
// -fsanitize=address,undefined: pitch, rows and bytes at the edges of the set count and of the region count, and every
// element a pass touches inside an exactly-sized heap block for small tables.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "kq_roff_host.h"

using namespace kq;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++bad; } } while (0)

int main() {
    // pitch: whole 64-byte lines, never below the set count, never above 64
    CHECK(roff_pitch(0) == 0);
    CHECK(roff_pitch(1) == 16);
    CHECK(roff_pitch(2) == 16);
    CHECK(roff_pitch(16) == 16);
    CHECK(roff_pitch(17) == 32);
    CHECK(roff_pitch(32) == 32);
    CHECK(roff_pitch(33) == 48);
    CHECK(roff_pitch(48) == 48);
    CHECK(roff_pitch(49) == 64);
    CHECK(roff_pitch(63) == 64);
    CHECK(roff_pitch(64) == 64);
    CHECK(roff_pitch(65) == 0);
    CHECK(roff_pitch(0xFFFFFFFFu) == 0);
    for (uint32_t n = 1; n <= ROFF_MAX_SETS; ++n) {
        const uint32_t p = roff_pitch(n);
        CHECK(p >= n && p < n + ROFF_PITCH_STEP && p % ROFF_PITCH_STEP == 0 && p <= ROFF_MAX_SETS);
    }
    // table sizes: the smallest table (2048 regions), the tight-record threshold (2^16), a 3 Gbp table, the format limit
    const uint64_t regions[] = {0, 1, 2048, (1ull << 16) - 1, 1ull << 16, 3400000, (1ull << 32) - 1};
    for (uint64_t R : regions) {
        CHECK(roff_rows(R) == R + 1);
        CHECK(roff_bytes(R) == (R + 1) * 256);
        // the last element a pass reads or writes at any pitch lies inside the buffer
        for (uint32_t n = 1; n <= ROFF_MAX_SETS; ++n) {
            const uint32_t p = roff_pitch(n);
            CHECK((roff_index(roff_rows(R) - 1, p, p - 1) + 1) * sizeof(uint32_t) <= roff_bytes(R));
        }
    }
    CHECK(roff_bytes((1ull << 32) - 1) == (1ull << 40));
    CHECK(roff_bytes(1ull << 32) == 0);
    CHECK(roff_bytes(~0ull) == 0);
    // small tables for real: write every element of every row at every pitch into an exactly-sized block
    for (uint64_t R : {0ull, 1ull, 63ull, 64ull, 65ull, 2048ull}) {
        const size_t bytes = roff_bytes(R);
        std::unique_ptr<uint32_t[]> buf(new uint32_t[bytes / sizeof(uint32_t)]);
        for (uint32_t n : {1u, 16u, 17u, 33u, 64u}) {
            const uint32_t p = roff_pitch(n);
            for (uint64_t r = 0; r < roff_rows(R); ++r)
                for (uint32_t c = 0; c < p; ++c) buf[roff_index(r, p, c)] = c < n ? (uint32_t)r : 0u;
            // rows are contiguous: element (r, 0) follows element (r - 1, p - 1)
            for (uint64_t r = 1; r < roff_rows(R); ++r) CHECK(roff_index(r, p, 0) == roff_index(r - 1, p, p - 1) + 1);
            CHECK(buf[roff_index(R, p, n - 1)] == (uint32_t)R);
            CHECK(n == p || buf[roff_index(R, p, p - 1)] == 0u);
        }
    }
    printf("offset-matrix geometry: %d failures\n", bad);
    return bad ? 1 : 0;
}
