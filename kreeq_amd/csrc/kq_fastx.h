// kq_fastx.h -- FASTQ / FASTA text -> read batch, and ASCII -> 2-bit packing, on the device (gfx950 only).
//
// The parse contract (include/kreeq_amd.h, kq_parse_fastx_dev): with l(i) = number of '\n' before byte i (a '\n' belongs
// to the line it ends) and EOL-CR = a '\r' directly followed by '\n',
//   FASTQ: byte i is kept iff l(i) mod 4 == 1 and it is no EOL-CR                      -> seq0\nseq1\n...
//   FASTA: of a header line (first byte '>') only its '\n' is kept; of any other line every byte but '\n' and EOL-CR
//                                                                                      -> \nseq0\nseq1...
// Whether a byte is kept depends on its line's state, which depends on every '\n' before it: a reduce / scan / apply chain
// over UNITS of FX_UNIT bytes of the (16-byte aligned view of the) text, one unit per wave:
//   k_fx_summary   per unit: the change of the line state over the unit, and the number of kept bytes for every state the
//                  unit may be entered in (4 for FASTQ: the '\n' count mod 4 rotates which local residue is kept; 2 for
//                  FASTA: only the unit's first partial line depends on the incoming state)
//   k_fx_scan      ONE workgroup: every unit's incoming state and output offset (exclusive scans), the total, the check
//                  of the first byte
//   k_fx_apply     per unit: kept bytes -> their output positions (ranks inside a wave from __ballot + mbcnt, the running
//                  offset of a wave is wave-uniform), and the record-structure checks
// A unit belongs to one wave, which walks it front to back, so neither kernel needs LDS or a barrier, and no workgroup ever
// waits for another one (no look-back): three plain launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kq {

constexpr int FX_FASTQ = 1, FX_FASTA = 2;                  // == KQ_FASTX_FASTQ / KQ_FASTX_FASTA
constexpr int FX_THREADS = 256;                            // 4 waves = 4 units per workgroup
constexpr int FX_ITERS = 4;                                // 16-byte loads per lane and unit, all issued before the first use
constexpr uint32_t FX_UNIT = 64 * 16 * FX_ITERS;           // 4096 bytes per wave
constexpr int FX_SCAN_THREADS = 1024;

// k_fx_summary -> k_fx_scan:  FASTQ  v = 4 x 16 bit: kept bytes whose LOCAL line residue is q;  st = '\n' count mod 4
//                             FASTA  v = kept bytes entered outside a header | entered inside one << 32;
//                                    st = bit 0: the unit has a '\n', bit 1: the line open at its end is a header
// k_fx_scan -> k_fx_apply:    v = output offset of the unit, st = its incoming state (l mod 4 / in a header)
struct FxUnit { unsigned long long v; uint32_t st; uint32_t pad; };
struct FxResult { unsigned long long n_bases; uint32_t bad; uint32_t pad; };      // bad: FX_FASTQ / FX_FASTA when the text broke the format

__device__ __forceinline__ uint32_t fx_below(uint64_t mask) {      // set bits of a ballot below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint64_t fx_lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }
// bit j = byte j of the 16 equals ch (SWAR zero-byte test on x ^ ch, exact)
__device__ __forceinline__ uint32_t fx_eq4(uint32_t x, uint32_t ch) {
    x ^= ch * 0x01010101u;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu) >> 7;      // bit 8b = byte b is zero
    return (z | (z >> 7) | (z >> 14) | (z >> 21)) & 0xFu;
}
__device__ __forceinline__ uint32_t fx_eq(const uint4& v, uint32_t ch) {
    return fx_eq4(v.x, ch) | (fx_eq4(v.y, ch) << 4) | (fx_eq4(v.z, ch) << 8) | (fx_eq4(v.w, ch) << 12);
}
__device__ __forceinline__ uint32_t fx_pxor(uint32_t x) { x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; return x; }

// one lane's 16 bytes of the text: the aligned chunk at g of the view `ab`, text = [lo, hi) in view coordinates
struct FxChunk {
    uint4 v;
    uint32_t in;        // bytes of the chunk inside the text
    uint32_t nl;        // '\n'
    uint32_t eolcr;     // '\r' directly followed by '\n'
    uint32_t nxt;       // the byte behind the chunk when the chunk ends with '\n' or '\r' and that byte is text; else 256
};
__device__ __forceinline__ uint4 fx_fetch(const uint8_t* __restrict__ ab, uint64_t lo, uint64_t hi, uint64_t g) {
    return (g + 16 > lo && g < hi) ? *reinterpret_cast<const uint4*>(ab + g) : make_uint4(0, 0, 0, 0);
}
__device__ __forceinline__ FxChunk fx_chunk(const uint4& v, const uint8_t* __restrict__ ab, uint64_t lo, uint64_t hi, uint64_t g) {
    FxChunk c;
    c.v = v;
    const uint32_t a = g >= lo ? 0u : (lo - g >= 16 ? 16u : (uint32_t)(lo - g));
    const uint32_t b = g >= hi ? 0u : (hi - g >= 16 ? 16u : (uint32_t)(hi - g));
    c.in = b > a ? (((1u << b) - 1u) & ~((1u << a) - 1u)) : 0u;
    c.nl = fx_eq(v, '\n') & c.in;
    const uint32_t cr = fx_eq(v, '\r') & c.in;
    c.nxt = 256u;
    if (((c.nl | cr) >> 15) && g + 16 < hi) c.nxt = ab[g + 16];      // one-byte look-ahead across the chunk (and unit) edge
    c.eolcr = cr & ((c.nl >> 1) | ((c.nxt == '\n' ? 1u : 0u) << 15));
    return c;
}

// ---- FASTQ ----------------------------------------------------------------------------------------------------------
// bit planes of (r + number of '\n' before position j) mod 4 for the positions j = 0..16 of a chunk
__device__ __forceinline__ void fx_residues(uint32_t nl, uint32_t r, uint32_t& b0, uint32_t& b1) {
    const uint32_t i0 = fx_pxor(nl) << 1;                  // parity of the '\n' before j
    const uint32_t i1 = fx_pxor(nl & i0) << 1;             // bit 1 flips at every '\n' that finds the count odd
    const uint32_t r0 = (r & 1u) ? 0x1FFFFu : 0u, r1 = (r & 2u) ? 0x1FFFFu : 0u;
    b0 = i0 ^ r0;
    b1 = i1 ^ r1 ^ (i0 & r0);
}
__device__ __forceinline__ uint32_t fx_residue_is(uint32_t b0, uint32_t b1, uint32_t q) {
    return ((q & 1u) ? b0 : ~b0) & ((q & 2u) ? b1 : ~b1) & 0x1FFFFu;
}
// the '\n' count mod 4 before this lane's chunk (r = before the wave's 64 chunks), and r behind them
__device__ __forceinline__ uint32_t fx_fastq_prefix(uint32_t nl, uint32_t& r) {
    const uint32_t n = (uint32_t)__popc(nl);
    const uint64_t m0 = __ballot(n & 1u), m1 = __ballot(n & 2u);
    const uint32_t pre = (r + fx_below(m0) + 2u * fx_below(m1)) & 3u;
    r = (r + (uint32_t)__popcll(m0) + 2u * (uint32_t)__popcll(m1)) & 3u;
    return pre;
}

// ---- FASTA ----------------------------------------------------------------------------------------------------------
// header state behind a chunk's last '\n' = is the byte behind it a '>' (gt has 17 bits: position 16 = the look-ahead)
__device__ __forceinline__ uint32_t fx_fasta_out(uint32_t nl, uint32_t gt17) { return (gt17 >> (32 - __clz(nl))) & 1u; }      // (nl != 0)
// bytes of a chunk that lie in a header line, for a chunk entered in state `in`
__device__ __forceinline__ uint32_t fx_fasta_hdr(uint32_t nl, uint32_t gt17, uint32_t in) {
    uint32_t h = in ? 0xFFFFu : 0u;
    uint32_t starts = (nl << 1) & 0xFFFFu;                 // lines that start inside the chunk
    while (starts) {
        const uint32_t j = (uint32_t)__ffs(starts) - 1u;
        starts &= starts - 1u;
        const uint32_t up = (0xFFFFu << j) & 0xFFFFu;
        h = ((gt17 >> j) & 1u) ? (h | up) : (h & ~up);
    }
    return h;
}
__device__ __forceinline__ uint32_t fx_fasta_kept(const FxChunk& c, uint32_t hdr) {
    return c.in & ((hdr & c.nl) | (~hdr & ~c.nl & ~c.eolcr));
}
// state this lane's chunk is entered in: behind the last '\n' of the lanes below, or the wave's incoming state
__device__ __forceinline__ uint32_t fx_fasta_in(uint64_t has, uint64_t st, uint32_t wave_in) {
    const uint64_t below = has & fx_lanes_below();
    return below ? (uint32_t)(st >> (63 - __clzll(below))) & 1u : wave_in;
}

template <int FMT>
__global__ void __launch_bounds__(FX_THREADS) k_fx_summary(const uint8_t* __restrict__ ab, uint64_t lo, uint64_t hi, uint64_t n_units,
                                                           FxUnit* __restrict__ units) {
    const uint64_t unit = (uint64_t)blockIdx.x * (FX_THREADS / 64) + (threadIdx.x >> 6);
    if (unit >= n_units) return;                           // (whole waves leave: the ballots below see full waves)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t g0 = unit * FX_UNIT + 16u * lane;
    uint4 v[FX_ITERS];
#pragma unroll
    for (int it = 0; it < FX_ITERS; ++it) v[it] = fx_fetch(ab, lo, hi, g0 + (uint64_t)it * 1024u);
    unsigned long long acc = 0;
    uint32_t st = 0;
    if (FMT == FX_FASTQ) {
        uint32_t r = 0;
#pragma unroll
        for (int it = 0; it < FX_ITERS; ++it) {
            const FxChunk c = fx_chunk(v[it], ab, lo, hi, g0 + (uint64_t)it * 1024u);
            const uint32_t pre = fx_fastq_prefix(c.nl, r);
            uint32_t b0, b1;
            fx_residues(c.nl, pre, b0, b1);
            const uint32_t keepable = c.in & ~c.eolcr;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) acc += (unsigned long long)__popc(fx_residue_is(b0, b1, q) & keepable) << (16 * q);
        }
        st = r;
    } else {
        uint32_t in0 = 0, in1 = 1, any = 0;                // the wave's incoming state if the unit is entered outside / inside a header
#pragma unroll
        for (int it = 0; it < FX_ITERS; ++it) {
            const FxChunk c = fx_chunk(v[it], ab, lo, hi, g0 + (uint64_t)it * 1024u);
            const uint32_t gt17 = fx_eq(c.v, '>') | ((c.nxt == '>' ? 1u : 0u) << 16);
            const uint64_t has = __ballot(c.nl != 0);
            const uint64_t out = __ballot(c.nl != 0 && fx_fasta_out(c.nl, gt17));
            const uint32_t a = fx_fasta_in(has, out, in0), b = fx_fasta_in(has, out, in1);
            const uint32_t ka = (uint32_t)__popc(fx_fasta_kept(c, fx_fasta_hdr(c.nl, gt17, a)));
            const uint32_t kb = a == b ? ka : (uint32_t)__popc(fx_fasta_kept(c, fx_fasta_hdr(c.nl, gt17, b)));
            acc += (unsigned long long)ka | ((unsigned long long)kb << 32);
            if (has) { in0 = in1 = (uint32_t)(out >> (63 - __clzll(has))) & 1u; any = 1; }
        }
        st = any | (in0 << 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);      // (every field stays below 2^13)
    if (lane == 0) { FxUnit u; u.v = acc; u.st = st; u.pad = 0; units[unit] = u; }
}

// inclusive scan over the workgroup, op(earlier, later); *total = all FX_SCAN_THREADS values
template <class Op>
__device__ __forceinline__ unsigned long long fx_block_scan(unsigned long long x, Op op, unsigned long long ident, unsigned long long* s_w,
                                                            unsigned long long* total) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(x, o, 64);
        if ((int)lane >= o) x = op(y, x);
    }
    __syncthreads();                                       // (s_w of the scan before this one has been read)
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    unsigned long long pre = ident, all = ident;
    for (uint32_t i = 0; i < FX_SCAN_THREADS / 64; ++i) { if (i < w) pre = op(pre, s_w[i]); all = op(all, s_w[i]); }
    *total = all;
    return op(pre, x);
}

template <int FMT>
__global__ void __launch_bounds__(FX_SCAN_THREADS) k_fx_scan(const uint8_t* __restrict__ ab, uint64_t lo, FxUnit* __restrict__ units,
                                                             uint64_t n_units, FxResult* __restrict__ res) {
    __shared__ unsigned long long s_w[FX_SCAN_THREADS / 64];
    const auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
    const auto later = [](unsigned long long a, unsigned long long b) { return a > b ? a : b; };
    const uint32_t first = ab[lo];
    // state the text is entered in: line 0 of a FASTQ record / a FASTA header line -- anything else is refused
    const bool bad = first != (FMT == FX_FASTQ ? (uint32_t)'@' : (uint32_t)'>');
    unsigned long long state = FMT == FX_FASTQ ? 0ull : (first == '>' ? 1ull : 0ull), off = 0;
    for (uint64_t t = 0; t < n_units; t += FX_SCAN_THREADS) {
        const uint64_t u = t + threadIdx.x;
        FxUnit x; x.v = 0; x.st = 0; x.pad = 0;
        if (u < n_units) x = units[u];
        unsigned long long total, kept;
        uint32_t in;
        if (FMT == FX_FASTQ) {
            const unsigned long long incl = fx_block_scan((unsigned long long)x.st, add, 0ull, s_w, &total);
            in = (uint32_t)(state + incl - x.st) & 3u;
            kept = (x.v >> (16u * ((1u - in) & 3u))) & 0xFFFFull;          // kept: true residue 1 = local residue 1 - in
            state = (state + total) & 3ull;
        } else {
            // "the last unit with a '\n' so far, and the state behind it" as a maximum: (unit + 1) << 1 | header
            const unsigned long long mine = (x.st & 1u) ? (((u + 1) << 1) | (x.st >> 1)) : 0ull;
            const unsigned long long incl = fx_block_scan(mine, later, 0ull, s_w, &total);
            const unsigned long long prev = __shfl_up(incl, 1, 64);
            // exclusive value: the inclusive one of the thread before (across waves: rebuilt from the wave totals)
            unsigned long long excl = (threadIdx.x & 63) ? prev : 0ull;
            if ((threadIdx.x & 63) == 0) for (uint32_t i = 0; i < (threadIdx.x >> 6); ++i) excl = later(excl, s_w[i]);
            in = excl ? (uint32_t)(excl & 1ull) : (uint32_t)state;
            kept = in ? (x.v >> 32) : (x.v & 0xFFFFFFFFull);
            if (total) state = total & 1ull;
        }
        unsigned long long sum;
        const unsigned long long incl = fx_block_scan(kept, add, 0ull, s_w, &sum);
        if (u < n_units) { FxUnit y; y.v = off + incl - kept; y.st = in; y.pad = 0; units[u] = y; }
        off += sum;
    }
    if (threadIdx.x == 0) { res->n_bases = off; res->bad = bad ? (uint32_t)FMT : 0u; res->pad = 0; }
}

// out == nullptr: checks only (the sizing call, and a caller's buffer that is too small)
template <int FMT>
__global__ void __launch_bounds__(FX_THREADS) k_fx_apply(const uint8_t* __restrict__ ab, uint64_t lo, uint64_t hi, uint64_t n_units,
                                                         const FxUnit* __restrict__ units, uint8_t* __restrict__ out, FxResult* __restrict__ res) {
    const uint64_t unit = (uint64_t)blockIdx.x * (FX_THREADS / 64) + (threadIdx.x >> 6);
    if (unit >= n_units) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t g0 = unit * FX_UNIT + 16u * lane;
    uint4 v[FX_ITERS];
#pragma unroll
    for (int it = 0; it < FX_ITERS; ++it) v[it] = fx_fetch(ab, lo, hi, g0 + (uint64_t)it * 1024u);
    const FxUnit me = units[unit];
    uint64_t pos = me.v;                                   // wave-uniform: where the wave's next kept byte goes
    uint32_t state = me.st;
    uint32_t bad = 0;
#pragma unroll
    for (int it = 0; it < FX_ITERS; ++it) {
        const FxChunk c = fx_chunk(v[it], ab, lo, hi, g0 + (uint64_t)it * 1024u);
        uint32_t kept;
        if (FMT == FX_FASTQ) {
            const uint32_t pre = fx_fastq_prefix(c.nl, state);
            uint32_t b0, b1;
            fx_residues(c.nl, pre, b0, b1);
            kept = fx_residue_is(b0, b1, 1u) & c.in & ~c.eolcr;
            // the byte behind every '\n', if the text has one: line 0 of a record starts with '@', line 2 with '+'
            const uint32_t at17 = fx_eq(c.v, '@') | ((c.nxt == '@' ? 1u : 0u) << 16), plus17 = fx_eq(c.v, '+') | ((c.nxt == '+' ? 1u : 0u) << 16);
            const uint32_t in17 = c.in | ((c.nxt < 256u ? 1u : 0u) << 16);
            bad |= (c.nl << 1) & in17 & ((fx_residue_is(b0, b1, 0u) & ~at17) | (fx_residue_is(b0, b1, 2u) & ~plus17));
        } else {
            const uint32_t gt17 = fx_eq(c.v, '>') | ((c.nxt == '>' ? 1u : 0u) << 16);
            const uint64_t has = __ballot(c.nl != 0);
            const uint64_t outs = __ballot(c.nl != 0 && fx_fasta_out(c.nl, gt17));
            kept = fx_fasta_kept(c, fx_fasta_hdr(c.nl, gt17, fx_fasta_in(has, outs, state)));
            if (has) state = (uint32_t)(outs >> (63 - __clzll(has))) & 1u;
        }
        // rank of this lane's first kept byte among the wave's: a 5-bit count per lane, one ballot per bit
        const uint32_t n = (uint32_t)__popc(kept);
        uint32_t rank = 0, total = 0;
#pragma unroll
        for (uint32_t bit = 0; bit < 5; ++bit) {
            const uint64_t m = __ballot((n >> bit) & 1u);
            rank += fx_below(m) << bit;
            total += (uint32_t)__popcll(m) << bit;
        }
        if (out && kept) {
            uint8_t* p = out + pos + rank;
            const uint32_t w[4] = { c.v.x, c.v.y, c.v.z, c.v.w };
            if (kept == 0xFFFFu) {
                // the common case inside a sequence line: head bytes up to a 4-byte boundary, three or four u32, tail bytes
                const uint32_t a = (uint32_t)((uintptr_t)p & 3u);
                if (a == 0) {
                    uint32_t* p4 = reinterpret_cast<uint32_t*>(p);
                    p4[0] = w[0]; p4[1] = w[1]; p4[2] = w[2]; p4[3] = w[3];
                } else {
                    const uint32_t head = 4u - a, sh = 8u * head;
#pragma unroll
                    for (uint32_t j = 0; j < 3; ++j) if (j < head) p[j] = (uint8_t)(w[0] >> (8 * j));
                    uint32_t* p4 = reinterpret_cast<uint32_t*>(p + head);
#pragma unroll
                    for (int i = 0; i < 3; ++i) p4[i] = (w[i] >> sh) | (w[i + 1] << (32u - sh));
#pragma unroll
                    for (uint32_t j = 0; j < 3; ++j) if (j < a) p[head + 12 + j] = (uint8_t)(w[3] >> (sh + 8 * j));
                }
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) if ((kept >> j) & 1u) *p++ = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
            }
        }
        pos += total;
    }
    if (bad) atomicOr(&res->bad, (uint32_t)FMT);
}

// ---- ASCII -> 2-bit packed units (kq_pack_bases' layout) -----------------------------------------------------------------
// unit u = the bytes [16 u, 16 u + 16) of the text, which starts `lead` bytes into the aligned view: two aligned 16-byte loads
// and a byte funnel shift when lead != 0.  One u32 of codes (0 at invalid positions, like the host packer) + one u16 of
// invalid-base bits per unit; positions at or behind `len` are invalid.
__device__ __forceinline__ uint32_t fx_spread16(uint32_t x) {      // bit i -> bits 2i and 2i + 1
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x | (x << 1);
}
__global__ void __launch_bounds__(256) k_pack_bases(const uint8_t* __restrict__ ab, uint32_t lead, uint64_t len, uint32_t* __restrict__ codes,
                                                    uint16_t* __restrict__ inv) {
    const uint64_t n_units = (len + 15) / 16, end = lead + len;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = 16 * u;                         // view offset of the aligned chunk that holds the unit's first byte
        uint4 v = *reinterpret_cast<const uint4*>(ab + g);
        if (lead) {
            const uint4 n = g + 16 < end ? *reinterpret_cast<const uint4*>(ab + g + 16) : make_uint4(0, 0, 0, 0);
            const uint32_t w[8] = { v.x, v.y, v.z, v.w, n.x, n.y, n.z, n.w };
            const uint32_t q = lead >> 2, sh = 8 * (lead & 3);
            uint32_t o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint32_t a = 0, b = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) if ((int)q == j) { a = w[i + j]; b = w[i + j + 1]; }       // (static register indices)
                o[i] = (uint32_t)((((uint64_t)b << 32) | a) >> sh);
            }
            v = make_uint4(o[0], o[1], o[2], o[3]);
        }
        uint32_t c, m;
        convert16(v, g + 16 <= len, (int64_t)g, 0, (int64_t)len, c, m);
        codes[u] = c & ~fx_spread16(m);
        inv[u] = (uint16_t)m;
    }
}

}  // namespace kq
