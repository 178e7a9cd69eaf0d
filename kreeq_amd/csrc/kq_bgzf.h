// kq_bgzf.h -- BGZF members -> text on the device (gfx950 only), and the cut of a text at its last whole record.
//
// k_bgzf_inflate   one BGZF member per workgroup of ONE wave.  The member's text (<= 64 KiB) is built in LDS, which is also the
//                  LZ77 window: a member has no preset dictionary, so no back-reference leaves it.  The decoder is the core of
//                  kq_inflate_core.h; its state (bit buffer, positions, the symbol being decoded) is wave-uniform: every lane runs
//                  the same symbol loop on the same values and table reads are LDS broadcasts.  What one lane does: the stores of
//                  literals and table entries (lane 0).  What the lanes share: the loads of the compressed input (16 bytes per
//                  lane, 1 KiB per step, one step ahead of the bit reader, into a 2 KiB ring), match copies (64 bytes per step),
//                  the CRC-32 (a stripe per lane, combined by x^(8 n) mod P) and the store of the text (16 bytes per lane).
//                  LDS: 65552 (text + 16 bytes the funnel shift of the last store may read) + 2048 (ring) + 1076 (tables) bytes.
//                  The text goes to global memory only after the decode ended without an error code, at exactly ISIZE bytes, and
//                  the CRC-32 matched; a member that fails stores nothing and reports (index << 8 | code) by atomicMin, so the
//                  FIRST bad member of a call is the one reported, whatever the schedule.
//                  No workgroup reads what another one wrote, none waits for another one.
//                  LDS order: the wave's DS instructions execute in issue order, so a lane reads what another lane of the same wave
//                  stored by an earlier instruction; the wavefront-scope fences keep the compiler from moving them.
// k_bgzf_count_nl  '\n' count of a text (FASTQ cut)
// k_bgzf_cut       ONE workgroup walks the text backwards from its end:
//                    FASTQ  the byte after the last '\n' whose ordinal (from the start of the text) is = 0 mod 4: with N newlines
//                           that is the (N mod 4 + 1)-th from the end; 0 if N < 4
//                    FASTA  the last '>' behind a '\n'; 0 if there is none
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kq_inflate_core.h"

namespace kq {

constexpr uint32_t BZ_OUT = 65536, BZ_RING = 2048, BZ_CHUNK = 1024;
constexpr int BZ_CUT_THREADS = 256;
constexpr uint32_t BZ_CUT_WINDOW = BZ_CUT_THREADS * 16;

struct BzBlock { unsigned long long in_off, out_off; uint32_t data_len, crc, isize, pad; };      // in_off: of the DEFLATE data in the compressed buffer
struct BzStatus { unsigned long long first_bad, n_nl, cut, pad; };                              // first_bad: index << 8 | code, ~0 = none
struct BzLds {
    uint8_t out[BZ_OUT + 16];
    uint8_t ring[BZ_RING];
    kqinf::Tables tab;
};
static_assert(sizeof(BzLds) <= 80 * 1024, "two workgroups per CU");

__device__ __forceinline__ void bz_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

struct BzMem {
    BzLds& s;
    const uint8_t* ab;           // 16-byte aligned view of the compressed data
    uint32_t lead, span;         // the data is [lead, span) of the view
    uint32_t filled = 0;         // view bytes in the ring so far (a multiple of BZ_CHUNK)
    uint32_t lane;
    uint4 ahead;                 // this lane's 16 bytes of the chunk behind `filled`, already loaded

    __device__ __forceinline__ BzMem(BzLds& s_, const uint8_t* data, uint32_t data_len, uint32_t lane_)
        : s(s_), ab((const uint8_t*)((uintptr_t)data & ~(uintptr_t)15)), lead((uint32_t)((uintptr_t)data & 15)), span(lead + data_len), lane(lane_) {
        ahead = fetch(0);
    }
    // the aligned 16 bytes at view offset g + 16 lane, if they hold data (the first such chunk starts at or before `lead`)
    __device__ __forceinline__ uint4 fetch(uint32_t g) const {
        const uint32_t o = g + 16u * lane;
        return o < span ? *reinterpret_cast<const uint4*>(ab + o) : make_uint4(0, 0, 0, 0);
    }
    __device__ __forceinline__ void fill() {
        *reinterpret_cast<uint4*>(s.ring + ((filled + 16u * lane) & (BZ_RING - 1))) = ahead;
        filled += BZ_CHUNK;
        ahead = fetch(filled);
        bz_fence();
    }
    // The core reads bytes in ascending order, so the chunk a fill overwrites (two chunks back) is never read again.  At most
    // span / BZ_CHUNK + 1 fills per member.
    __device__ __forceinline__ uint32_t in_byte(uint32_t i) {
        const uint32_t p = i + lead;
        while (p >= filled) fill();
        return s.ring[p & (BZ_RING - 1)];
    }
    __device__ __forceinline__ void out_put(uint32_t pos, uint32_t b) { if (lane == 0) s.out[pos] = (uint8_t)b; }
    // every source byte lies before pos: with dist < len the copy repeats the last dist bytes, text[pos + j] = text[pos - dist + j mod dist]
    __device__ __forceinline__ void out_copy(uint32_t pos, uint32_t dist, uint32_t len) {
        bz_fence();
        for (uint32_t j = lane; j < len; j += 64) s.out[pos + j] = s.out[pos - dist + (dist >= len ? j : j % dist)];
        bz_fence();
    }
    __device__ __forceinline__ kqinf::Tables* tables() { return &s.tab; }
    __device__ __forceinline__ void st16(uint16_t* p, uint32_t v) { if (lane == 0) *p = (uint16_t)v; }
    __device__ __forceinline__ void st8(uint8_t* p, uint32_t v) { if (lane == 0) *p = (uint8_t)v; }
    __device__ __forceinline__ void tables_ready() { bz_fence(); }
};

__global__ void __launch_bounds__(64) k_bgzf_inflate(const uint8_t* __restrict__ comp, const BzBlock* __restrict__ blocks, uint32_t n_blocks,
                                                     uint8_t* __restrict__ text, BzStatus* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) BzLds s;
    const uint32_t blk = blockIdx.x, lane = threadIdx.x;
    if (blk >= n_blocks) return;
    const BzBlock b = blocks[blk];
    const uint32_t data_len = (uint32_t)__builtin_amdgcn_readfirstlane((int)b.data_len), isize = (uint32_t)__builtin_amdgcn_readfirstlane((int)b.isize);
    if (data_len > BZ_OUT || isize > BZ_OUT) return;          // (the host checked both)
    BzMem m(s, comp + b.in_off, data_len, lane);
    kqinf::Inflate<BzMem> inf(m, data_len, isize);
    int code = inf.run();
    bz_fence();
    if (code == kqinf::OK) {
        // CRC-32: lane l takes the bytes [l stripe, (l + 1) stripe); stripes are a multiple of 4 bytes plus 4, so that the lanes'
        // reads fall into different banks
        const uint32_t stripe = ((((isize + 63u) / 64u) + 3u) & ~3u) + 4u;
        const uint32_t lo = min(lane * stripe, isize), hi = min(lo + stripe, isize);
        uint32_t reg = 0xFFFFFFFFu;
        for (uint32_t i = lo; i < hi; ++i) reg = kqinf::crc_byte(reg, s.out[i]);
        uint32_t crc = hi > lo ? kqinf::gf2_mul(kqinf::gf2_xpow8(isize - hi), ~reg) : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) crc ^= __shfl_xor(crc, o, 64);
        if (crc != b.crc) code = kqinf::ERR_CRC;
    }
    if (code != kqinf::OK) {
        if (lane == 0) atomicMin(&status->first_bad, ((unsigned long long)blk << 8) | (unsigned long long)code);
        return;
    }
    // the text: bytes up to the first 16-byte boundary of the destination, 16-byte stores, the rest by bytes
    uint8_t* dst = text + b.out_off;
    const uint32_t head = min(isize, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    if (lane < head) dst[lane] = s.out[lane];
    const uint32_t n_vec = (isize - head) / 16u;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(s.out);
    for (uint32_t v = lane; v < n_vec; v += 64) {
        const uint32_t o = head + 16u * v, sh = 8u * (o & 3u);      // (o >> 2) + 4 <= (BZ_OUT + 12) / 4: inside s.out
        uint32_t x[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) x[i] = w[(o >> 2) + i];
        uint4 r;
        r.x = (uint32_t)(((((unsigned long long)x[1]) << 32) | x[0]) >> sh);
        r.y = (uint32_t)(((((unsigned long long)x[2]) << 32) | x[1]) >> sh);
        r.z = (uint32_t)(((((unsigned long long)x[3]) << 32) | x[2]) >> sh);
        r.w = (uint32_t)(((((unsigned long long)x[4]) << 32) | x[3]) >> sh);
        *reinterpret_cast<uint4*>(dst + o) = r;
    }
    const uint32_t tail = head + 16u * n_vec;
    if (tail + lane < isize) dst[tail + lane] = s.out[tail + lane];      // (fewer than 16 bytes)
}

// ---- the cut ----------------------------------------------------------------------------------------------------------------
// text is 16-byte aligned; bit j of the result = byte g + j is inside [0, total)
__device__ __forceinline__ uint32_t bz_inside(uint64_t g, uint64_t total) {
    return g >= total ? 0u : (total - g >= 16 ? 0xFFFFu : ((1u << (uint32_t)(total - g)) - 1u));
}

__global__ void __launch_bounds__(256) k_bgzf_count_nl(const uint8_t* __restrict__ text, uint64_t total, BzStatus* __restrict__ status) {
    const uint64_t n_chunks = (total + 15) / 16;
    unsigned long long n = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + 16 * c);
        n += (unsigned long long)__popc(fx_eq(v, '\n') & bz_inside(16 * c, total));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&status->n_nl, n);
}

template <int FMT>
__global__ void __launch_bounds__(BZ_CUT_THREADS) k_bgzf_cut(const uint8_t* __restrict__ text, uint64_t total, BzStatus* __restrict__ status) {
    __shared__ uint32_t s_cnt[BZ_CUT_THREADS];
    __shared__ unsigned long long s_found;                     // FASTQ: position of the '\n' + 1; FASTA: position of the '>' (> 0)
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_found = 0;
    unsigned long long need = 0;
    if (FMT == FX_FASTQ) {
        const unsigned long long n = status->n_nl;
        if (n < 4) { if (tid == 0) status->cut = 0; return; }  // (the whole workgroup leaves)
        need = (n & 3ull) + 1ull;
    }
    __syncthreads();
    for (uint64_t w = (total + BZ_CUT_WINDOW - 1) / BZ_CUT_WINDOW; w-- > 0;) {       // every window holds text: the walk ends at window 0
        const uint64_t g = w * BZ_CUT_WINDOW + 16u * tid;
        const uint32_t in = bz_inside(g, total);
        const uint4 v = in ? *reinterpret_cast<const uint4*>(text + g) : make_uint4(0, 0, 0, 0);
        const uint32_t nl = fx_eq(v, '\n') & in;
        if (FMT == FX_FASTQ) {
            const uint32_t c = (uint32_t)__popc(nl);
            s_cnt[tid] = c;
            __syncthreads();
            uint32_t above = 0, all = 0;
            for (uint32_t t = 0; t < (uint32_t)BZ_CUT_THREADS; ++t) { const uint32_t x = s_cnt[t]; all += x; if (t > tid) above += x; }
            if (above < need && need <= above + c) {
                uint32_t mk = nl;
                for (unsigned long long i = 1; i < need - above; ++i) mk &= ~(1u << (31 - __clz(mk)));      // need - above <= c = popc(nl)
                s_found = g + (uint64_t)(31 - __clz(mk)) + 1ull;
            }
            __syncthreads();
            if (s_found) break;
            need -= all;
        } else {
            const uint32_t prev = (in && g > 0 && text[g - 1] == '\n') ? 1u : 0u;
            const uint32_t starts = fx_eq(v, '>') & in & ((nl << 1) | prev);
            if (starts) atomicMax(&s_found, (unsigned long long)(g + (uint64_t)(31 - __clz(starts))));
            __syncthreads();
            const unsigned long long found = s_found;
            __syncthreads();                                   // every thread has read this window's result before the next window writes one
            if (found) break;
        }
    }
    __syncthreads();
    if (tid == 0) status->cut = s_found;
}

}  // namespace kq
