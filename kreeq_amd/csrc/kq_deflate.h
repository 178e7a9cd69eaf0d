// kq_deflate.h -- text on the device -> BGZF members (gfx950 only).  The code builder is kq_deflate_core.h.
//
// k_bgzf_deflate   one member (<= 0xff00 bytes of text) per workgroup of ONE wave.  The member's text is loaded into LDS with
//                  16-byte loads (any alignment of d_text: an aligned view is funnel-shifted) and is the LZ77 window.
//                  The text is walked in STEPS of 64 positions, one per lane:
//                    match    the lane hashes the 3 bytes at its position (12 bits), reads the candidate the EARLIER steps left in
//                             the hash table (u16 positions in LDS) and measures the match against the text, 4 bytes per compare,
//                             up to 32 bytes ("32 or more"; the parse measures the rest of the matches it takes, up to
//                             min(258, end of text), with the whole wave: 4 bytes per lane, one ballot); distance <= 32 768 by
//                             check, >= 1 because the candidate is older than the step.  3-byte matches further back than 4096 are dropped (they cost more than 3 literals).
//                             A lane that found nothing older takes the LOWEST position of its own step with the same hash, if
//                             that lies below it (the start of a run inside the step).
//                    insert   every lane stores its position into its slot; lanes that hit the same slot resolve to the HIGHEST
//                             position: store, read back, the lanes above the value read store again (<= 64 rounds, each raises
//                             the slot), so the table after a step is a function of the text alone.
//                    parse    greedy, wave-uniform, one round per MATCH taken (not per byte): from the first position not yet
//                             covered, everything before the next lane with a match is a literal, then the match covers its
//                             length (ballot, count-trailing-zeros, one cross-lane read of the length).
//                  The walk runs TWICE: pass 1 counts the symbols (LDS atomics), lane 0 runs plan_block (lengths, codes, header
//                  items, dynamic or stored), pass 2 finds the same tokens again and emits their bits.  Tokens are not kept: a
//                  token array beside the text would take the LDS that lets two workgroups share a CU.
//                  Bits: per step an exclusive wave prefix sum over the tokens' bit lengths gives each lane its bit offset; the
//                  lanes OR their <= 48 bits into a 512-byte LDS stage that starts with the carried partial word, and the full
//                  32-bit words go to the member's slot with plain stores.  The header items go out the same way, 64 per step.
//                  CRC-32: a stripe per lane, combined by x^(8 n) mod P, as in k_bgzf_inflate.
//                  The member lies at slot + 2, so that its DEFLATE data (slot + 20) is 4-byte aligned.  A violated bound is an
//                  error code (member << 8 | code, atomicMin: the first bad member is reported) and the member's size becomes 0.
// k_bgzf_sizes_scan  ONE wave: exclusive scan of a batch's member sizes behind the running total of the call
// k_bgzf_gather    one workgroup per member: slot -> its place in the contiguous output, 16 bytes per lane and store
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kq_bgzf.h"
#include "kq_deflate_core.h"

namespace kq {

constexpr uint32_t DF_TEXT = kqdef::MEMBER_TEXT, DF_WORDS = (DF_TEXT + 16) / 4, DF_HASH_BITS = 12, DF_HASH = 1u << DF_HASH_BITS;
constexpr uint32_t DF_STAGE = 128, DF_SLOT = 65536, DF_LEAD = 2, DF_DATA = DF_LEAD + kqdef::HEADER_BYTES;      // DF_DATA = 20
constexpr uint32_t DF_SLOT_WORDS = (DF_SLOT - DF_DATA) / 4;
constexpr uint32_t DF_TOO_FAR = 4096, DF_EMPTY = 0xFFFF, DF_QUICK = 32;
constexpr int DF_GATHER_THREADS = 256;

struct DfStatus { unsigned long long first_bad, total; };      // first_bad: member << 8 | code, ~0 = none; total: bytes written so far
struct DfLds {
    uint32_t text[DF_WORDS];         // the member's text, zero behind its end (the 4-byte compares read up to 7 bytes past a position)
    uint16_t hash[DF_HASH];
    uint32_t stage[DF_STAGE];
    kqdef::Work w;
};
static_assert(sizeof(DfLds) <= 80 * 1024, "two workgroups per CU");
static_assert(DF_TEXT < DF_EMPTY, "a position fits a hash entry");

// what the wave carries through a pass
struct DfEmit {
    uint32_t* out;                   // the slot's DEFLATE data, as words
    uint32_t wpos = 0, carry = 0, cb = 0;      // full words written, the partial word and its bit count
    int err = 0;
};

// the 4 bytes at text position p; p + 7 < 4 DF_WORDS is the caller's bound, checked here once more
__device__ __forceinline__ uint32_t df_rd4(const DfLds& s, uint32_t p, int& err) {
    const uint32_t i = p >> 2;
    if (i + 1 >= DF_WORDS) { err = kqdef::ERR_BOUND; return 0; }
    const uint64_t v = (uint64_t)s.text[i] | (uint64_t)s.text[i + 1] << 32;
    return (uint32_t)(v >> (8u * (p & 3u)));
}
// an error any lane met becomes the wave's: the lanes never part ways over it
__device__ __forceinline__ bool df_bad(DfEmit& e) {
    if (!__ballot(e.err != 0)) return false;
    if (!e.err) e.err = kqdef::ERR_BOUND;
    return true;
}
__device__ __forceinline__ uint32_t df_hash(uint32_t w4) { return ((w4 & 0xFFFFFFu) * 0x9E3779B1u) >> (32 - DF_HASH_BITS); }

// One step of bit emission: every lane brings nb <= 48 bits (0: none), in lane order.
__device__ __forceinline__ void df_emit_step(DfLds& s, DfEmit& e, uint32_t lane, uint64_t bits, uint32_t nb) {
    uint32_t inc = nb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o, 64); if ((int)lane >= o) inc += t; }
    const uint32_t total = __shfl(inc, 63, 64), excl = inc - nb;
    s.stage[lane] = lane == 0 ? e.carry : 0u;
    s.stage[lane + 64] = 0u;
    bz_fence();
    if (nb) {
        const uint32_t off = e.cb + excl, wi = off >> 5, sh = off & 31u;      // off <= 31 + 63 x 48: wi <= 95
        if (wi + 2 < DF_STAGE) {
            const uint64_t lo = bits << sh;
            const uint32_t hi = sh ? (uint32_t)(bits >> (64u - sh)) : 0u;
            atomicOr(&s.stage[wi], (uint32_t)lo);
            if (lo >> 32) atomicOr(&s.stage[wi + 1], (uint32_t)(lo >> 32));
            if (hi) atomicOr(&s.stage[wi + 2], hi);
        } else e.err = kqdef::ERR_BOUND;
    }
    bz_fence();
    const uint32_t tot = e.cb + total, nw = tot >> 5;                        // nw <= 97 < DF_STAGE
    if (nw >= DF_STAGE || e.wpos + nw > DF_SLOT_WORDS) e.err = kqdef::ERR_BOUND;      // (wave-uniform values)
    if (df_bad(e)) return;
    for (uint32_t j = lane; j < nw; j += 64) e.out[e.wpos + j] = s.stage[j];
    e.carry = s.stage[nw];
    e.cb = tot & 31u;
    e.wpos += nw;
    bz_fence();
}

// One walk over the text.  EMIT = false counts the tokens into s.w.lfreq / dfreq, EMIT = true emits their bits.
template <bool EMIT>
__device__ __forceinline__ void df_pass(DfLds& s, uint32_t n, uint32_t lane, DfEmit& e) {
    for (uint32_t i = lane; i < DF_HASH; i += 64) s.hash[i] = (uint16_t)DF_EMPTY;
    bz_fence();
    uint32_t covered = 0;                                          // wave-uniform: positions below it lie inside a match already taken
    for (uint32_t base = 0; base < n; base += 64) {               // <= 1020 steps
        const uint32_t p = base + lane;
        const bool can = p + kqdef::MIN_MATCH <= n;
        uint32_t h = 0, mlen = 0, dist = 0;
        // the match of position p against an earlier position: length and distance, or nothing
        auto measure = [&](uint32_t cand) {
            const uint32_t maxlen = min(DF_QUICK, n - p);          // DF_QUICK means "32 or more": the parse measures the rest of a match it takes
            uint32_t len = 0;
            while (len < maxlen) {                                 // <= 8 rounds; p + len < n
                const uint32_t x = df_rd4(s, p + len, e.err) ^ df_rd4(s, cand + len, e.err);
                if (x) { len += (uint32_t)__builtin_ctz(x) >> 3; break; }
                len += 4;
            }
            len = min(len, maxlen);
            if (len >= kqdef::MIN_MATCH && !(len == kqdef::MIN_MATCH && p - cand > DF_TOO_FAR)) { mlen = len; dist = p - cand; }
        };
        if (can) {
            h = df_hash(df_rd4(s, p, e.err));                      // h < DF_HASH by the shift
            const uint32_t cand = s.hash[h];
            if (cand != DF_EMPTY && cand < p && p - cand <= kqdef::WINDOW && p >= covered) measure(cand);
        }
        bz_fence();
        // Lanes that found nothing older look inside the step: the slot is resolved to the LOWEST position of the step first
        // (store, read back, the lanes below the value read store again: <= 64 rounds, each lowers the slot), and a lane above
        // it measures against that one.  Skipped when no lane needs it.
        const bool wants = can && mlen == 0 && p >= covered;
        if (__ballot(wants)) {
            bool pend = can;
            for (int r = 0; r < 64; ++r) {
                if (pend) s.hash[h] = (uint16_t)p;
                bz_fence();
                if (pend) pend = (uint32_t)s.hash[h] > p;
                bz_fence();
                if (!__ballot(pend)) break;
            }
            if (wants) {
                const uint32_t cand = s.hash[h];                   // a position of this step: base <= cand <= p
                if (cand < p) measure(cand);
            }
            bz_fence();
        }
        // insert: the highest position of the step wins its slot
        bool pend = can;
        for (int r = 0; r < 64; ++r) {
            if (pend) s.hash[h] = (uint16_t)p;
            bz_fence();
            if (pend) pend = (uint32_t)s.hash[h] < p;              // the value read is a position of this step: the slot was just written
            bz_fence();
            if (!__ballot(pend)) break;
        }
        // parse
        const uint64_t has = __ballot(mlen != 0);
        uint64_t tok = 0;
        uint32_t c = covered > base ? covered - base : 0u;
        for (int r = 0; r < 64 && c < 64; ++r) {                   // every round takes a match or ends the step
            const uint64_t rest = has & (~0ull << c);
            if (!rest) { tok |= ~0ull << c; c = 64; break; }
            const uint32_t m = (uint32_t)__builtin_ctzll(rest);
            tok |= (~0ull << c) & (m == 63 ? ~0ull : ((1ull << (m + 1)) - 1ull));
            uint32_t len = (uint32_t)__shfl((int)mlen, (int)m, 64);      // >= 3 there
            const uint32_t pm = base + m, maxlen = min(kqdef::MAX_MATCH, n - pm);
            if (len == DF_QUICK && maxlen > DF_QUICK) {
                // the rest of the match, by the whole wave: lane l compares the 4 bytes at DF_QUICK + 4 l (64 lanes reach 288 >= 258)
                const uint32_t cm = pm - (uint32_t)__shfl((int)dist, (int)m, 64), off = DF_QUICK + 4u * lane;
                uint32_t same = 4;
                if (off < maxlen) {                                // pm + off < n, cm < pm
                    const uint32_t x = df_rd4(s, pm + off, e.err) ^ df_rd4(s, cm + off, e.err);
                    if (x) same = (uint32_t)__builtin_ctz(x) >> 3;
                }
                const uint64_t differ = __ballot(same < 4);
                if (differ) { const int f = __builtin_ctzll(differ); len = min(maxlen, DF_QUICK + 4u * (uint32_t)f + (uint32_t)__shfl((int)same, f, 64)); }
                else len = maxlen;
                if (lane == m) mlen = len;
            }
            c = m + len;
        }
        covered = base + c;
        const bool is_tok = ((tok >> lane) & 1ull) && p < n;
        const bool is_match = is_tok && mlen != 0;
        const uint32_t lit = ((const uint8_t*)s.text)[min(p, DF_TEXT - 1)];
        if (!EMIT) {
            if (is_match) {
                uint32_t sy, nb, ex;
                kqdef::len_sym(mlen, sy, nb, ex); atomicAdd(&s.w.lfreq[257u + sy], 1u);      // sy <= 28
                kqdef::dist_sym(dist, sy, nb, ex); atomicAdd(&s.w.dfreq[sy], 1u);            // sy <= 29: dist <= 32 768
            } else if (is_tok) atomicAdd(&s.w.lfreq[lit], 1u);
        } else {
            uint64_t bits = 0; uint32_t nb = 0;
            if (is_match) kqdef::match_bits(s.w, mlen, dist, bits, nb);
            else if (is_tok) kqdef::literal_bits(s.w, lit, bits, nb);
            df_emit_step(s, e, lane, bits, nb);
            if (e.err) return;                                     // (the wave's, after df_emit_step)
        }
    }
    bz_fence();
    df_bad(e);
}

__global__ void __launch_bounds__(64) k_bgzf_deflate(const uint8_t* __restrict__ text, uint64_t n_text, uint64_t first_member, uint32_t n_members,
                                                     uint8_t* __restrict__ slots, uint32_t* __restrict__ sizes, DfStatus* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) DfLds s;
    const uint32_t blk = blockIdx.x, lane = threadIdx.x;
    if (blk >= n_members) return;
    const uint64_t member = first_member + blk, t0 = member * (uint64_t)DF_TEXT;
    if (t0 >= n_text) { if (lane == 0) sizes[blk] = 0; return; }      // (the host launches no empty member)
    const uint32_t n = (uint32_t)min((uint64_t)DF_TEXT, n_text - t0);
    uint8_t* slot = slots + (uint64_t)blk * DF_SLOT;
    // the text: chunk c of 16 bytes = view bytes [lead + 16 c, lead + 16 c + 16) of the aligned view; zero behind the text
    {
        const uint8_t* src = text + t0;
        const uint8_t* ab = (const uint8_t*)((uintptr_t)src & ~(uintptr_t)15);
        const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uintptr_t)src & 15)), span = lead + n;
        const uint32_t ws = lead >> 2, sh = 8u * (lead & 3u);
        for (uint32_t c = lane; c < DF_WORDS / 4; c += 64) {       // DF_WORDS / 4 = 4081 chunks: the whole array is written
            uint32_t x[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (16u * c < span) { const uint4 v = *reinterpret_cast<const uint4*>(ab + 16u * c); x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
            if (16u * c + 16u < span) { const uint4 v = *reinterpret_cast<const uint4*>(ab + 16u * c + 16u); x[4] = v.x; x[5] = v.y; x[6] = v.z; x[7] = v.w; }
            uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (k == ws) {
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i) o[i] = (uint32_t)((((uint64_t)x[k + i + 1] << 32) | x[k + i]) >> sh);
                }
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {                     // bytes at or behind n become zero
                const uint32_t b0 = 16u * c + 4u * i;
                if (b0 >= n) o[i] = 0; else if (n - b0 < 4) o[i] &= (1u << (8u * (n - b0))) - 1u;
            }
            *reinterpret_cast<uint4*>(&s.text[4 * c]) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
    for (uint32_t i = lane; i < (uint32_t)kqdef::N_LIT; i += 64) s.w.lfreq[i] = 0;
    if (lane < (uint32_t)kqdef::N_DIST) s.w.dfreq[lane] = 0;
    bz_fence();
    DfEmit e;
    e.out = reinterpret_cast<uint32_t*>(slot + DF_DATA);
    df_pass<false>(s, n, lane, e);
    // the codes: one lane; the plan comes back through LDS
    if (lane == 0) {
        const kqdef::Plan pl = kqdef::plan_block(s.w, n);
        s.stage[0] = (uint32_t)pl.err; s.stage[1] = pl.dynamic ? 1u : 0u; s.stage[2] = pl.payload; s.stage[3] = pl.dyn_bits;
    }
    bz_fence();
    int code = e.err ? e.err : (int)s.stage[0];                    // (wave-uniform: df_pass ends with df_bad)
    const bool dynamic = s.stage[1] != 0 && code == kqdef::OK;
    uint32_t payload = s.stage[2];
    const uint32_t dyn_bits = s.stage[3];
    bz_fence();
    if (payload > kqdef::STORED_BYTES + n) code = kqdef::ERR_BOUND;
    if (code == kqdef::OK && dynamic) {
        const uint32_t n_items = min(s.w.n_items, kqdef::MAX_ITEMS);
        for (uint32_t b = 0; b < n_items && !e.err; b += 64) {     // the header, 64 items per step
            const uint32_t it = b + lane < n_items ? s.w.u.items[b + lane] : 0u;
            df_emit_step(s, e, lane, it & 0xFFFFFFu, it >> 24);
        }
        if (!e.err) df_pass<true>(s, n, lane, e);
        if (!e.err) {
            uint64_t bits = 0; uint32_t nb = 0;
            if (lane == 0) kqdef::literal_bits(s.w, kqdef::EOB, bits, nb);
            df_emit_step(s, e, lane, bits, nb);
        }
        if (!e.err && 32u * e.wpos + e.cb != dyn_bits) e.err = kqdef::ERR_BOUND;      // both passes found the same tokens (uniform)
        if (!e.err) {
            const uint32_t tail = (e.cb + 7u) / 8u;                // < 4 bytes of the partial word; 4 wpos + tail = payload < DF_SLOT - DF_DATA
            if (lane < tail) (reinterpret_cast<uint8_t*>(e.out))[4u * e.wpos + lane] = (uint8_t)(e.carry >> (8u * lane));
        }
        code = e.err;
    } else if (code == kqdef::OK) {
        // stored: 5 bytes, then the text; word j holds bytes 4 j .. 4 j + 3 of that
        payload = kqdef::STORED_BYTES + n;
        const uint8_t* tb = (const uint8_t*)s.text;
        auto byte_at = [&](uint32_t i) { return i < kqdef::STORED_BYTES ? kqdef::stored_byte(i, n) : (uint32_t)tb[min(i - kqdef::STORED_BYTES, DF_TEXT - 1)]; };
        for (uint32_t j = lane; j < payload / 4u; j += 64)         // whole words; 4 j + 3 < payload <= 65 285 < DF_SLOT - DF_DATA
            e.out[j] = byte_at(4u * j) | byte_at(4u * j + 1u) << 8 | byte_at(4u * j + 2u) << 16 | byte_at(4u * j + 3u) << 24;
        const uint32_t done = payload & ~3u;
        if (done + lane < payload) (reinterpret_cast<uint8_t*>(e.out))[done + lane] = (uint8_t)byte_at(done + lane);      // < 4 bytes
    }
    if (code != kqdef::OK) {
        if (lane == 0) { atomicMin(&status->first_bad, ((unsigned long long)member << 8) | (unsigned long long)code); sizes[blk] = 0; }
        return;
    }
    // CRC-32, striped as in k_bgzf_inflate
    const uint32_t stripe = ((((n + 63u) / 64u) + 3u) & ~3u) + 4u;
    const uint32_t lo = min(lane * stripe, n), hi = min(lo + stripe, n);
    uint32_t reg = 0xFFFFFFFFu;
    for (uint32_t i = lo; i < hi; ++i) reg = kqinf::crc_byte(reg, ((const uint8_t*)s.text)[i]);
    uint32_t crc = hi > lo ? kqinf::gf2_mul(kqinf::gf2_xpow8(n - hi), ~reg) : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) crc ^= __shfl_xor(crc, o, 64);
    const uint32_t size = kqdef::HEADER_BYTES + payload + kqdef::TRAILER_BYTES;      // <= 65 311
    if (lane < kqdef::HEADER_BYTES) slot[DF_LEAD + lane] = (uint8_t)kqdef::header_byte(lane, size);
    if (lane < kqdef::TRAILER_BYTES) slot[DF_DATA + payload + lane] = (uint8_t)kqdef::trailer_byte(lane, crc, n);
    if (lane == 0) sizes[blk] = size;
}

// offs[i] = total + sizes[0] + .. + sizes[i - 1]; total += the batch.  One wave; lane l takes a contiguous run of members.
__global__ void __launch_bounds__(64) k_bgzf_sizes_scan(const uint32_t* __restrict__ sizes, uint32_t n, unsigned long long* __restrict__ offs, DfStatus* __restrict__ status) {
    const uint32_t lane = threadIdx.x, per = (n + 63u) / 64u, lo = min(lane * per, n), hi = min(lo + per, n);
    unsigned long long sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += sizes[i];
    unsigned long long inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = __shfl_up(inc, o, 64); if ((int)lane >= o) inc += t; }
    const unsigned long long before = status->total;
    unsigned long long at = before + inc - sum;
    for (uint32_t i = lo; i < hi; ++i) { offs[i] = at; at += sizes[i]; }
    if (lane == 63) status->total = before + inc;                  // (the value stored depends on the one every lane read)
}

// member i: sizes[i] bytes from slot i + DF_LEAD to out + offs[i].  Bytes up to the first 16-byte boundary of the destination,
// 16-byte stores built from aligned words of the slot, the rest by bytes.
__global__ void __launch_bounds__(DF_GATHER_THREADS) k_bgzf_gather(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes,
                                                                   const unsigned long long* __restrict__ offs, uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    if (blk >= n) return;
    const uint32_t size = min(sizes[blk], kqdef::MEMBER_MAX);
    const uint8_t* slot = slots + (uint64_t)blk * DF_SLOT;
    uint8_t* dst = out + offs[blk];
    const uint32_t head = min(size, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    if (tid < head) dst[tid] = slot[DF_LEAD + tid];
    const uint32_t n_vec = (size - head) / 16u;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(slot);
    for (uint32_t v = tid; v < n_vec; v += DF_GATHER_THREADS) {
        const uint32_t o = head + 16u * v, q = DF_LEAD + o, sh = 8u * (q & 3u);      // (q >> 2) + 4 <= (2 + 65 311 + 16) / 4: inside the slot
        uint32_t x[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) x[i] = w[(q >> 2) + i];
        uint4 r;
        r.x = (uint32_t)(((((unsigned long long)x[1]) << 32) | x[0]) >> sh);
        r.y = (uint32_t)(((((unsigned long long)x[2]) << 32) | x[1]) >> sh);
        r.z = (uint32_t)(((((unsigned long long)x[3]) << 32) | x[2]) >> sh);
        r.w = (uint32_t)(((((unsigned long long)x[4]) << 32) | x[3]) >> sh);
        *reinterpret_cast<uint4*>(dst + o) = r;
    }
    const uint32_t tail = head + 16u * n_vec;
    if (tail + tid < size) dst[tail + tid] = slot[DF_LEAD + tail + tid];      // (fewer than 16 bytes)
}

}  // namespace kq
