"""Hand-built DEFLATE streams for the inflater (kreeq_amd/csrc/kq_inflate_core.h, k_bgzf_inflate): what zlib's compressor never
writes.  A bit-level builder on bgzf_inputs.BitWriter (canonical codes from code lengths; stored, fixed and dynamic block
writers, the dynamic header with the code-length symbols the caller chooses) and ONE list of cases that the host program
(tests/test_inflate_streams.py, tests/test_inflate_core_host.py) and the kernel (tests/test_gpu_inflate_streams.py) both run.
A good case carries its tokens; its text is text_of(tokens), the serial meaning of LZ77 tokens, and zlib's inflate is the
reference that says the stream means that text.  An error case carries the code the core must end in.  Every case has a predicate
that says which edge it contains.  Plain Python, no project code."""
import collections
import functools
import random
import struct
import zlib

import numpy as np

from tests import bgzf_inputs as B

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# a complete code over all 19 code-length symbols: 13 of 4 bits and 6 of 5 bits (13 / 16 + 6 / 32 = 1)
FULL_CL = {s: (4 if s < 13 else 5) for s in range(19)}
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32

# the message texts of kqinf::err_name, by code (tests/test_inflate_streams.py checks them against the header's own)
ERR_TEXT = {
    1: "reserved block type", 2: "stored block length mismatch", 3: "too many length or distance codes", 4: "over-subscribed code lengths",
    5: "incomplete code lengths", 6: "invalid code length repeat", 7: "invalid literal/length code", 8: "invalid distance code",
    9: "distance too far back", 10: "compressed data ends early", 11: "uncompressed size differs from ISIZE", 12: "data behind the final block",
    13: "CRC-32 mismatch",
}


def text_of(tokens):
    """the serial meaning of tokens (byte,) and (length, distance[, flag]): byte by byte, so that dist < len repeats"""
    out = bytearray()
    for t in tokens:
        if len(t) == 1:
            out.append(t[0])
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def canonical(lengths):
    """{symbol: (code with its bits reversed, length)} of the canonical Huffman code with these code lengths (RFC 1951 3.2.2);
    reversed, because BitWriter.bits writes from bit 0 up and Huffman codes go most significant bit first"""
    count = collections.Counter(l for l in lengths if l)
    code, nxt = 0, {}
    for bits in range(1, 16):
        code = (code + count.get(bits - 1, 0)) << 1
        nxt[bits] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (int(format(nxt[l], "0%db" % l)[::-1], 2), l)
            nxt[l] += 1
    return out


def kraft(lengths):
    """sum of 2^-l in units of 2^-15: 32768 = complete"""
    return sum(1 << (15 - l) for l in lengths if l)


def balanced(symbols, n, deeper=0):
    """n code lengths: a complete code over `symbols` (two or more) with lengths that differ by one at the most, `deeper` added"""
    symbols = sorted(symbols)
    k = len(symbols)
    assert k >= 2
    b = (k - 1).bit_length()
    short = (1 << b) - k
    out = [0] * n
    for i, s in enumerate(symbols):
        out[s] = (b - 1 if i < short else b) + deeper
    return out


def deep(ladder, rest, n):
    """n code lengths of a complete code: the 15 symbols of `ladder` get 2, 3, .. 14, 15, 15 bits (half of the code space), the
    symbols of `rest` share the other half evenly"""
    assert len(ladder) == 15 and not set(ladder) & set(rest)
    out = balanced(rest, n, deeper=1)
    for i, s in enumerate(ladder):
        out[s] = min(i + 2, 15)
    assert kraft(out) == 32768
    return out


def length_symbol(length, alt=False):
    """(symbol, extra bits, extra value); alt: 258 as symbol 284 with extra bits 31"""
    if length == 258 and alt:
        return 284, 5, 31
    s = max(i for i in range(29) if LEN_BASE[i] <= length)
    if s == 28 and length != 258:
        s = 27
    assert 0 <= length - LEN_BASE[s] < (1 << LEN_EXT[s]) or (LEN_EXT[s] == 0 and length == LEN_BASE[s])
    return 257 + s, LEN_EXT[s], length - LEN_BASE[s]


def distance_symbol(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    assert dist - DIST_BASE[s] < (1 << DIST_EXT[s])
    return s, DIST_EXT[s], dist - DIST_BASE[s]


def expand(clsyms):
    """the code lengths that a list of code-length symbols means: n = the length n, (16, r) = the previous length r times (3..6),
    (17, r) = r zeros (3..10), (18, r) = r zeros (11..138)"""
    out = []
    for c in clsyms:
        if isinstance(c, int):
            out.append(c)
        elif c[0] == 16:
            out += [out[-1]] * c[1]
        else:
            out += [0] * c[1]
    return out


def rle(lengths):
    """code-length symbols with repeats, greedily"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        run = 1
        while i + run < n and lengths[i + run] == lengths[i]:
            run += 1
        if lengths[i] == 0 and run >= 3:
            r = min(run, 138)
            out.append((18 if r >= 11 else 17, r))
            i += r
        elif i > 0 and lengths[i] == lengths[i - 1] and run >= 3:
            r = min(run, 6)
            out.append((16, r))
            i += r
        else:
            out.append(lengths[i])
            i += 1
    return out


class Stream:
    """one raw DEFLATE stream, block by block; .tokens and .blocks say what was written"""

    def __init__(self):
        self.w = B.BitWriter()
        self.tokens, self.blocks = [], []

    def pos(self):
        return 8 * len(self.w.out) + self.w.n

    def raw(self):
        return self.w.done()

    def stored(self, data, final=False):
        """a stored block at whatever bit position the stream is at: the 3 header bits, zeros to the byte boundary, LEN, NLEN"""
        self.blocks.append({"type": 0, "at": self.pos(), "len": len(data)})
        self.w.bits(int(final), 1).bits(0, 2)
        if self.w.n:
            self.w.bits(0, 8 - self.w.n)
        self.w.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + bytes(data)
        self.tokens += [(b,) for b in data]
        return self

    def body(self, tokens, lcodes, dcodes, alt258=False, end=True):
        w = self.w
        for t in tokens:
            if len(t) == 1:
                w.bits(*lcodes[t[0]])
                continue
            s, n, v = length_symbol(t[0], alt258 or (len(t) > 2 and t[2]))
            w.bits(*lcodes[s])
            w.bits(v, n)
            s, n, v = distance_symbol(t[1])
            w.bits(*dcodes[s])
            w.bits(v, n)
        if end:
            w.bits(*lcodes[256])
        self.tokens += list(tokens)
        return self

    def fixed(self, tokens, final=False, alt258=False):
        self.blocks.append({"type": 1, "at": self.pos(), "tokens": len(tokens)})
        self.w.bits(int(final), 1).bits(1, 2)
        return self.body(tokens, canonical(FIXED_LL), canonical(FIXED_DL), alt258)

    def header(self, hlit, hdist, clsyms, cl_lengths=None, hclen=None, final=False):
        """a dynamic block's header as given, checked against nothing (the error cases use it)"""
        cl_lengths = FULL_CL if cl_lengths is None else cl_lengths
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lengths.get(s, 0)])
        self.blocks.append({"type": 2, "at": self.pos(), "hlit": hlit, "hdist": hdist, "hclen": hclen, "clsyms": list(clsyms)})
        w = self.w
        w.bits(int(final), 1).bits(2, 2).bits(hlit - 257, 5).bits(hdist - 1, 5).bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl_lengths.get(s, 0), 3)
        codes = canonical([cl_lengths.get(s, 0) for s in range(19)])
        for c in clsyms:
            if isinstance(c, int):
                w.bits(*codes[c])
            else:
                w.bits(*codes[c[0]])
                w.bits(c[1] - (11 if c[0] == 18 else 3), {16: 2, 17: 3, 18: 7}[c[0]])
        return self

    def dynamic(self, tokens, ll, dl, final=False, clsyms=None, cl_lengths=None, hclen=None, alt258=False):
        """a dynamic block: literal/length code lengths ll (257..286 of them), distance code lengths dl (1..30); clsyms: the
        code-length symbols of the header (default: every length as itself), which must mean ll + dl"""
        ll, dl = list(ll), list(dl)
        clsyms = ll + dl if clsyms is None else clsyms
        assert expand(clsyms) == ll + dl and 257 <= len(ll) <= 286 and 1 <= len(dl) <= 30
        self.header(len(ll), len(dl), clsyms, cl_lengths, hclen, final)
        self.blocks[-1].update(ll=ll, dl=dl, tokens=len(tokens))
        return self.body(tokens, canonical(ll), canonical(dl), alt258)


def used(tokens, alt258=False):
    """-> (literal/length symbols, distance symbols) that the tokens use, the end-of-block code included"""
    ls, ds = {256}, set()
    for t in tokens:
        if len(t) == 1:
            ls.add(t[0])
        else:
            ls.add(length_symbol(t[0], alt258 or (len(t) > 2 and t[2]))[0])
            ds.add(distance_symbol(t[1])[0])
    return ls, ds


def lits(data):
    return [(b,) for b in data]


def rand_bytes(n, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


LL_ALL = balanced(range(286), 286)             # literals 0..225 in 8 bits, everything above in 9
DL_ALL = balanced(range(30), 30)


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    """raw: the DEFLATE data; code 0: it means `text` (= text_of(tokens)); code 1..13: the core ends in that error.  isize / crc:
    what the member's trailer says.  check(case, max_len, max_dist) -> the case holds the edge it is named for; max_len and
    max_dist are what the host program reports (longest code length built, farthest distance copied)"""

    def __init__(self, name, group, raw, text=None, code=0, tokens=None, blocks=None, isize=None, crc=None, check=None, member=None):
        self.name, self.group, self.raw, self.text, self.code = name, group, raw, text, code
        self.tokens, self.blocks, self.check = tokens, blocks or [], check or (lambda c, max_len, max_dist: True)
        if member is None:
            body = text if text is not None else b""
            member = B.member(raw, zlib.crc32(body) if crc is None else crc, len(body) if isize is None else isize)
        self.member = member


def good(name, group, s, check=None):
    text = text_of(s.tokens)
    return Case(name, group, s.raw(), text, 0, s.tokens, s.blocks, check=check)


def matches(c):
    return [t for t in c.tokens if len(t) > 1]


COPY_LENGTHS = (3, 4, 63, 64, 65, 127, 128, 129, 257, 258)
COPY_DISTS = range(1, 71)


def copy_cases():
    """every dist 1..70 with every length on both sides of the 64-lane step: one member per length.  Before each match come as
    many fresh random literals as its distance (four at the least), so the whole source window differs from byte to byte and
    from the window of the match before: a wrong source index changes the text"""
    out = []
    for k, L in enumerate(COPY_LENGTHS):
        rng = random.Random(1000 + L)
        tokens = []
        for d in COPY_DISTS:
            tokens += lits(rng.randrange(256) for _ in range(max(d, 4)))
            tokens.append((L, d))
        s = Stream()
        if k % 2:
            s.dynamic(tokens, LL_ALL, DL_ALL, final=True)
        else:
            s.fixed(tokens, final=True)
        out.append(good("copy_len%d_dist1to70" % L, "copies", s,
                        lambda c, ml, md, L=L: [t[:2] for t in matches(c)] == [(L, d) for d in COPY_DISTS] and md == 70 and
                        len(c.tokens[-1]) == 2))                 # (the last token is a match: it ends exactly at isize)
    # dist == len and dist == len +- 1 around 128 and 258, where the grid above does not reach
    rng = random.Random(77)
    tokens = []
    pairs = [(L, L + e) for L in (127, 128, 129, 257, 258) for e in (-1, 0, 1)]
    for L, d in pairs:
        tokens += lits(rng.randrange(256) for _ in range(d))
        tokens.append((L, d))
    out.append(good("copy_dist_len_pm1", "copies", Stream().dynamic(tokens, LL_ALL, DL_ALL, final=True),
                    lambda c, ml, md: [t[:2] for t in matches(c)] == pairs and md == 259))
    # the source starts at text byte 0: dist == out_pos, shorter than, equal to and longer than the copy
    for n, L in ((1, 258), (5, 3), (64, 64), (65, 64), (70, 258), (300, 258)):
        tokens = lits(rand_bytes(n, 300 + n)) + [(L, n)]
        out.append(good("copy_from_byte0_n%d_len%d" % (n, L), "copies", Stream().fixed(tokens, final=True),
                        lambda c, ml, md, n=n, L=L: matches(c) == [(L, n)] and len(c.text) == n + L and md == n))
    # 65 536 bytes of text, the last token (258, 32768): 32 768 random literals, then only copies from 32 768 back
    tokens = lits(rand_bytes(32768, 31)) + [(258, 32768)] * 126 + [(7,), (9,)] + [(258, 32768)]
    ll = balanced(list(range(257)) + [285], 286)
    s = Stream().dynamic(tokens, ll, DL_ALL, final=True, clsyms=rle(ll + DL_ALL))
    out.append(good("copy_65536_last_258_32768", "copies", s,
                    lambda c, ml, md: len(c.text) == 65536 and c.tokens[-1] == (258, 32768) and md == 32768))
    return out


DEEP_LADDER_L = list(range(65, 78)) + [284, 285]                 # 'A'..'M' in 2..14 bits, the two symbols of length 258 in 15
DEEP_LADDER_D = list(range(0, 13)) + [14, 29]                    # distance codes 0..12 in 2..14 bits, 14 and 29 in 15


def deep_cases():
    ll = deep(DEEP_LADDER_L, [s for s in range(286) if s not in DEEP_LADDER_L], 286)
    dl = deep(DEEP_LADDER_D, [s for s in range(30) if s not in DEEP_LADDER_D], 30)
    tokens = lits(rand_bytes(32768, 41))
    lengths = [LEN_BASE[i] + e for i in range(29) for e in sorted({0, (1 << LEN_EXT[i]) - 1})]
    assert lengths[-3:] == [227, 258, 258]                       # 227 + 31 = 258 through symbol 284, then 258 as symbol 285
    dists = [DIST_BASE[i] + e for i in range(30) for e in sorted({0, (1 << DIST_EXT[i]) - 1})]
    assert dists[-2:] == [24577, 32768]
    alt_at = lengths.index(258)
    for i, d in enumerate(dists):
        j = i % len(lengths)
        tokens += lits(b"AM" + bytes([i, 255 - i]))
        tokens.append((lengths[j], d, j == alt_at))
    tokens += [(258, 24577, True), (258, 32767), (258, 32767, True), (258, 32768), (258, 32768, True), (3, 32768), (65,), (77,)]
    s = Stream().dynamic(tokens, ll, dl, final=True, clsyms=rle(ll + dl))

    def check(c, max_len, max_dist):
        ls, ds = used(c.tokens)
        far = {t[1] for t in matches(c)}
        ext = {(length_symbol(t[0], len(t) > 2 and t[2])[0], length_symbol(t[0], len(t) > 2 and t[2])[2]) for t in matches(c)}
        dxt = {distance_symbol(t[1])[::2] for t in matches(c)}
        return (max_len == 15 and max_dist == 32768 and ls >= set(range(257, 286)) and ds == set(range(30)) and {24577, 32767, 32768} <= far and
                max(ll[s] for s in ls) == 15 and max(dl[d] for d in ds) == 15 and ll[284] == ll[285] == 15 and dl[29] == 15 and
                all((257 + i, 0) in ext and (257 + i, (1 << LEN_EXT[i]) - 1) in ext for i in range(29)) and
                all((i, 0) in dxt and (i, (1 << DIST_EXT[i]) - 1) in dxt for i in range(30)))
    return [good("deep_codes_far_distances", "deep", s, check)]


def header_cases():
    out = []

    def add(name, s, check):
        out.append(good("header_" + name, "headers", s, check))

    def hdr(c, i=0):
        return c.blocks[i]

    text = lits(b"header case text, literals only")
    # HLIT 257 and HDIST 1 with no distance code at all (one distance length, 0): literals only
    ll = balanced(range(257), 257)
    add("hlit257_hdist1_no_distance_code", Stream().dynamic(text, ll, [0], final=True),
        lambda c, ml, md: (hdr(c)["hlit"], hdr(c)["hdist"], hdr(c)["hclen"]) == (257, 1, 19) and hdr(c)["dl"] == [0] and md == 0)
    # HLIT 286 and HDIST 30, every symbol with a code, plain lengths
    toks = text + [(10, 5), (258, 20)]
    add("hlit286_hdist30_hclen19", Stream().dynamic(toks, LL_ALL, DL_ALL, final=True),
        lambda c, ml, md: (hdr(c)["hlit"], hdr(c)["hdist"], hdr(c)["hclen"]) == (286, 30, 19) and all(isinstance(x, int) for x in hdr(c)["clsyms"]))
    # the shortest header that can carry an end-of-block code: HCLEN 5 (16, 17, 18, 0, 8): lengths 0 and 8 only, 256 codes of 8 bits
    # (HCLEN 4 leaves only the length 0: no end-of-block code; it is an error case)
    ll = [8] * 255 + [0, 8]
    add("hclen5", Stream().dynamic(lits(bytes(range(0, 255, 7))), ll, [0], final=True, cl_lengths={0: 1, 8: 1}),
        lambda c, ml, md: hdr(c)["hclen"] == 5 and ml == 8)
    # symbol 16 repeats a literal/length code length on into the distance lengths
    ll = LL_ALL
    dl = [9, 9, 9, 9, 7, 6, 5, 4, 3, 2, 1] + [0] * 19             # 4 / 512 + 1 / 128 + 1 / 64 + .. + 1 / 2 = 1
    assert kraft(dl) == 32768 and ll[284] == ll[285] == 9
    cl = ll[:285] + [(16, 5)] + dl[4:]                            # the length of symbol 284, repeated over 285 and four distance codes
    add("repeat16_across_hlit", Stream().dynamic(toks + [(4, 1), (5, 9)], ll, dl, final=True, clsyms=cl),
        lambda c, ml, md: hdr(c)["clsyms"][284:286] == [9, (16, 5)] and hdr(c)["hlit"] == 286)
    # 16 directly behind a 17 and behind an 18: it repeats zero
    ll = balanced(list(range(32, 127)) + [256, 257, 258], 286)
    cl = [(18, 29), (16, 3)] + ll[32:127] + [(17, 3), (16, 6), (18, 120)] + ll[256:259] + [(18, 27)] + [1, 1]
    assert expand(cl) == ll + [1, 1]
    add("repeat16_behind_17_and_18", Stream().dynamic(text + [(3, 1), (4, 2)], ll, [1, 1], final=True, clsyms=cl),
        lambda c, ml, md: hdr(c)["clsyms"][:2] == [(18, 29), (16, 3)] and (17, 3) in hdr(c)["clsyms"] and (16, 6) in hdr(c)["clsyms"])
    # 18 with its longest run, 138, and a repeat that ends exactly at HLIT + HDIST
    ll = balanced(range(138, 259), 259)
    dl = [3] * 8 + [0] * 22
    cl = [(18, 138)] + ll[138:] + [3, (16, 6), 3, (18, 22)]
    add("repeat18_138_and_repeat_to_the_end", Stream().dynamic(lits(bytes(range(138, 256))) + [(4, 7), (3, 5)], ll, dl, final=True, clsyms=cl),
        lambda c, ml, md: hdr(c)["clsyms"][0] == (18, 138) and hdr(c)["clsyms"][-1] == (18, 22) and len(expand(hdr(c)["clsyms"])) == 259 + 30)
    ll = LL_ALL
    dl = [5] * 2 + [4] * 15                                        # 2 / 32 + 15 / 16 = 1
    cl = ll + dl[:11] + [(16, 6)]
    add("repeat16_to_the_end", Stream().dynamic(toks, ll, dl, final=True, clsyms=cl),
        lambda c, ml, md: hdr(c)["clsyms"][-1] == (16, 6) and hdr(c)["hdist"] == 17)
    # the single distance code of one bit, used
    ll = balanced(list(range(97, 123)) + [256, 257, 285], 286)
    add("single_one_bit_distance_code", Stream().dynamic(lits(b"abcxyz") + [(3, 1), (258, 1)], ll, [1], final=True, clsyms=rle(ll + [1])),
        lambda c, ml, md: hdr(c)["dl"] == [1] and md == 1 and len(matches(c)) == 2)
    # a literal set that holds only the end-of-block code, in one bit: two such non-final blocks ahead of a fixed one
    eob = [0] * 256 + [1]
    s = Stream()
    s.dynamic([], eob, [0], clsyms=rle(eob + [0])).dynamic([], eob, [0], clsyms=[(18, 138), (18, 118), 1, 0])
    s.fixed(lits(b"behind two empty blocks"), final=True)
    add("end_of_block_only_sets", s, lambda c, ml, md: [b["type"] for b in c.blocks] == [2, 2, 1] and c.blocks[0]["ll"] == eob and ml == 9)
    return out


def block_cases():
    """one member of more than 200 blocks: empty and short stored blocks, fixed, dynamic and empty non-final dynamic blocks, and
    a stored block that starts at each of the 8 bit positions (fixed blocks of 9-bit literals ahead of it shift the position)"""
    rng = random.Random(5)
    eob = [0] * 256 + [1]
    small_l = balanced(list(range(97, 123)) + [256, 257, 258, 259, 260], 286)
    small_d = balanced(range(8), 8)
    s = Stream()
    for i in range(208):
        kind = i % 8
        word = bytes(rng.randrange(97, 123) for _ in range(rng.randrange(1, 10)))
        if kind in (0, 4):                                       # a stored block at bit position (i / 4) mod 8
            want = (i // 4) % 8
            shift = (want - s.pos() - 10) % 8                    # a fixed block is 10 bits and its literals; those above 143 take 9 bits
            s.fixed(lits(bytes(rng.randrange(144, 256) for _ in range(shift))))
            assert s.pos() % 8 == want
            s.stored(b"" if kind == 0 else word)
        elif kind in (1, 5):
            s.fixed(lits(word) + ([(len(word) + 2, len(word))] if kind == 5 else []))
        elif kind in (2, 6):
            s.dynamic(lits(word) + [(3 + kind // 2, 1 + i % len(word))], small_l, small_d, clsyms=rle(small_l + small_d))
        elif kind == 3:
            s.dynamic([], eob, [0], clsyms=rle(eob + [0]))
        else:
            s.dynamic([], small_l, small_d, clsyms=rle(small_l + small_d))      # empty, but with whole tables
    s.stored(b"the end", final=True)

    def check(c, ml, md):
        stored = [b for b in c.blocks if b["type"] == 0]
        return (len(c.blocks) >= 200 and {b["at"] % 8 for b in stored} == set(range(8)) and any(b["len"] == 0 for b in stored) and
                {b["type"] for b in c.blocks} == {0, 1, 2} and sum(1 for b in c.blocks if b["type"] == 2 and b["tokens"] == 0) >= 50)
    out = [good("blocks_200_mixed", "blocks", s, check)]
    out.append(good("stored_len0", "blocks", Stream().stored(b"", final=True), lambda c, ml, md: c.raw == b"\x01\x00\x00\xff\xff"))
    out.append(good("stored_len1", "blocks", Stream().stored(b"Q", final=True), lambda c, ml, md: c.raw == b"\x01\x01\x00\xfe\xffQ"))
    return out


# ---- input geometry: members whose DEFLATE data has a chosen length ----------------------------------------------------------
CHUNK = 1024                                                     # BZ_CHUNK of kq_bgzf.h: the ring is filled this many bytes at a time
MAX_DATA = 65536 - 26                                            # the DEFLATE data of the largest member: 18 header and 8 trailer bytes
# data_len + lead reaches each of the first three chunk edges, one byte less and one byte more, at every lead 0..15
EDGE_LENGTHS = sorted({e - lead + d for e in (CHUNK, 2 * CHUNK, 3 * CHUNK) for lead in range(16) for d in (-1, 0, 1)})


def stored_member(n_data, seed):
    return Stream().stored(rand_bytes(n_data - 5, seed), final=True)


def coded_member(n_data, seed, tail_bits, with_matches):
    """a dynamic block over random bytes that ends `tail_bits` short of the end of byte n_data: tail_bits 0 puts the last bit of
    the end-of-block code into the last bit of the last byte.  LL_ALL gives literals 0..225 8 bits and the rest 9, so 9-bit
    literals set the length modulo 8"""
    rng = random.Random(seed)
    s = Stream()
    s.header(286, 30, rle(LL_ALL + DL_ALL), final=True)
    s.blocks[-1].update(ll=LL_ALL, dl=DL_ALL, tokens=0)
    lcodes, dcodes = canonical(LL_ALL), canonical(DL_ALL)
    target = 8 * n_data - tail_bits
    n_out = 0
    tight = n_data > 30000                                       # then a match may not make more text than its bits would as literals
    while with_matches and target - s.pos() > 1000:
        group = lits(rng.randrange(226) for _ in range(rng.randrange(20, 40)))
        n_out += len(group)
        if tight and n_out > 1025:
            group.append((3, rng.randrange(1025, min(n_out, 32768) + 1)))      # 9 + 5 + 9 bits or more for 3 bytes
        elif not tight:
            group.append((rng.choice((3, 4, 11, 35, 131)), rng.randrange(1, n_out + 1)))
        n_out += group[-1][0] if len(group[-1]) > 1 else 0
        s.body(group, lcodes, dcodes, end=False)
    rem = target - s.pos() - 9                                   # what literals must fill ahead of the 9-bit end-of-block code
    nine = rem % 8
    eight = (rem - 9 * nine) // 8
    assert eight >= 0, (n_data, rem)
    fill = lits(rng.randrange(226) for _ in range(eight)) + lits(rng.randrange(226, 256) for _ in range(nine))
    s.body(fill, lcodes, dcodes)
    assert s.pos() == target
    s.end_bits = target
    return s


def last_bit_is_read(c):
    """with the last bit of the data inverted, zlib no longer ends the stream there with the same text: the bit belongs to a code"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(c.raw[:-1] + bytes([c.raw[-1] ^ 0x80]))
        return not (d.eof and text == c.text)
    except zlib.error:
        return True


def input_geometry_cases():
    out = []
    # data_len 1 holds no whole stream (the shortest, a fixed block of the end-of-block code alone, is 10 bits): it is an error case
    out.append(good("data_len_2", "input_geometry", Stream().fixed([], final=True), lambda c, ml, md: len(c.raw) == 2))
    for n in EDGE_LENGTHS + [MAX_DATA]:
        out.append(good("data_len_%d_stored" % n, "input_geometry", stored_member(n, n), lambda c, ml, md, n=n: len(c.raw) == n and c.blocks[0]["type"] == 0))
        s = coded_member(n, n + 1, 5, False)
        out.append(good("data_len_%d_literals" % n, "input_geometry", s,
                        lambda c, ml, md, n=n: len(c.raw) == n and not matches(c) and len(c.text) > 0.95 * (n - 200)))
        s = coded_member(n, n + 2, 0, True)
        out.append(good("data_len_%d_eob_in_last_bit" % n, "input_geometry", s,
                        lambda c, ml, md, n=n, bits=s.end_bits: len(c.raw) == n and bits == 8 * n and last_bit_is_read(c) and len(matches(c)) > 10))
    return out


OUT_SIZES = list(range(0, 81)) + list(range(250, 261)) + [4095, 4096, 4097, 65535, 65536]


def output_geometry_cases():
    """zlib-made members of chosen ISIZE: the CRC stripes and the head / vector / tail store"""
    fq = B.fastq_text(65536, seed=12)
    out = []
    for n in OUT_SIZES:
        text = fq[:n] if n % 2 else fq[65536 - n:]
        out.append(Case("isize_%d" % n, "output_geometry", B.deflate_raw(text, level=1 if n > 5000 else 6), text, 0, None, None,
                        check=lambda c, ml, md, n=n: len(c.text) == n))
    return out


# ---- errors ----------------------------------------------------------------------------------------------------------------
def more_invalid_streams():
    """[(code, raw)] the core's error list beyond the mutations: repeat with nothing before it, an incomplete literal set, symbol
    286, distance code 30, trailing bytes, a missing end-of-block code when the input ends (members of ISIZE 1, the text b"a")"""
    W = B.BitWriter

    def dyn(clens, body):
        """dynamic header with HCLEN 19 and the code-length code lengths `clens` (indexed by symbol), then body(w)"""
        w = W().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(15, 4)
        for s in CL_ORDER:
            w.bits(clens.get(s, 0), 3)
        body(w)
        return w.bits(0, 24).done()

    cases = []
    # code-length code {16: 1 bit, 0: 1 bit}: canonical codes 0 -> symbol 0, 1 -> symbol 16; the first symbol is 16
    cases.append((B.ERR_REPEAT, dyn({16: 1, 0: 1}, lambda w: w.code(1, 1).bits(0, 2))))
    # code-length code {1: 1 bit, 18: 1 bit}: 0 -> symbol 1, 1 -> symbol 18.  257 literal lengths of 1 bit: over-subscribed
    cases.append((B.ERR_OVERSUBSCRIBED, dyn({1: 1, 18: 1}, lambda w: [w.code(0, 1) for _ in range(258)])))

    # {2: 1 bit, 18: 1 bit}: 0 -> symbol 2, 1 -> symbol 18: literal 0 and end-of-block 2 bits each, nothing else: incomplete
    def incomplete(w):
        w.code(0, 1)                                               # literal 0: 2 bits
        w.code(1, 1).bits(138 - 11, 7).code(1, 1).bits(117 - 11, 7)      # 255 zeros
        w.code(0, 1)                                               # 256: 2 bits
        w.code(0, 1)                                               # the one distance length
    cases.append((B.ERR_INCOMPLETE, dyn({2: 1, 18: 1}, incomplete)))
    cases.append((B.ERR_SYMBOL, W().bits(1, 1).bits(1, 2).fixed_lit(286).bits(0, 16).done()))
    cases.append((B.ERR_DIST_CODE, W().bits(1, 1).bits(1, 2).fixed_lit(ord("a")).fixed_lit(257).code(30, 5).bits(0, 16).done()))
    cases.append((B.ERR_TRAILING, W().bits(1, 1).bits(1, 2).fixed_lit(ord("a")).fixed_lit(256).done() + b"\0"))
    cases.append((B.ERR_INPUT_END, W().bits(1, 1).bits(1, 2).fixed_lit(ord("a")).done()))
    cases.append((B.ERR_INPUT_END, W().bits(0, 1).bits(1, 2).fixed_lit(ord("a")).fixed_lit(256).done()))      # not the final block, and no other follows
    cases.append((B.ERR_INPUT_END, b""))
    return cases


MORE_INVALID_NAMES = ["repeat_at_first_length", "oversubscribed_literals", "incomplete_literals", "symbol_286", "distance_code_30", "one_trailing_byte_fixed",
                      "no_end_of_block", "no_final_block", "no_data"]


def error_cases():
    out = []

    def add(name, code, raw, text=b"", isize=None, check=None):
        out.append(Case(name, "errors", raw, None, code, isize=len(text) if isize is None else isize, crc=zlib.crc32(text), check=check))

    text = B.fastq_text(B.BLOCK_TEXT)
    for name, m, code in B.mutations(B.bgzf_block(text, level=6), text):
        out.append(Case(name, "errors", m[18:-8], None, code, member=m))
    for name, (code, raw) in zip(MORE_INVALID_NAMES, more_invalid_streams()):
        add(name, code, raw, b"a")
    pad = 24                                                     # bits behind the bad code: the decoder walks 15 bits before it gives up

    ll = balanced(list(range(97, 123)) + [256, 257, 285], 286)
    s = Stream().header(286, 1, rle(ll + [1]), final=True)
    s.body(lits(b"a"), canonical(ll), {}, end=False)
    s.w.bits(*canonical(ll)[257])
    s.w.bits(1, 1).bits(0, pad)                                  # the one distance code is the bit 0; this is the bit 1
    add("one_bit_distance_code_unassigned_bit", B.ERR_DIST_CODE, s.raw(), b"aaaa")
    s = Stream().header(286, 1, rle(ll + [0]), final=True)
    s.body(lits(b"a"), canonical(ll), {}, end=False)
    s.w.bits(*canonical(ll)[257])
    s.w.bits(0, pad)
    add("length_symbol_without_distance_code", B.ERR_DIST_CODE, s.raw(), b"aaaa")
    w = B.BitWriter().bits(1, 1).bits(1, 2)
    add("distance_code_31", B.ERR_DIST_CODE, w.fixed_lit(ord("a")).fixed_lit(257).code(31, 5).bits(0, 16).done(), b"aaaa")
    body = rand_bytes(100, 8)
    s = Stream().fixed(lits(body) + [(3, 101)], final=True)
    add("distance_out_pos_plus_1", B.ERR_DISTANCE, s.raw(), body + body[:3])
    s = Stream().fixed(lits(body) + [(258, 100)], final=True)
    add("match_258_overruns_isize_by_1", B.ERR_OUTPUT, s.raw(), text_of(s.tokens)[:-1])
    s = Stream().fixed(lits(body[:7])).stored(body[:10], final=True)
    add("stored_overruns_isize", B.ERR_OUTPUT, s.raw(), text_of(s.tokens)[:-1])
    lens = LL_ALL + DL_ALL
    s = Stream().header(286, 30, lens[:-6] + [(16, 3), (16, 4)], final=True)       # 316 lengths are 310 + 3 + 3
    s.w.bits(0, pad)
    add("repeat_one_past_the_lengths", B.ERR_REPEAT, s.raw(), b"a")
    ll0 = balanced(range(256), 257)                              # 256 literals of 8 bits, no end-of-block code
    s = Stream().header(257, 1, ll0 + [0], final=True)
    s.w.bits(0, pad)
    add("no_end_of_block_length", B.ERR_INCOMPLETE, s.raw(), b"a")
    s = Stream().header(286, 2, LL_ALL + [2, 2], final=True)
    s.body(lits(b"a"), canonical(LL_ALL), {})
    add("two_code_incomplete_distance_set", B.ERR_INCOMPLETE, s.raw(), b"a")
    add("symbol_287", B.ERR_SYMBOL, B.BitWriter().bits(1, 1).bits(1, 2).fixed_lit(287).bits(0, 16).done(), b"a")
    # HCLEN 4 reads code lengths for 16, 17, 18 and 0 only: every literal length is 0, there is no end-of-block code
    s = Stream().header(257, 1, [(18, 138), (18, 120)], cl_lengths={18: 1, 0: 1}, hclen=4, final=True)
    s.w.bits(0, pad)
    add("hclen4_has_no_end_of_block", B.ERR_INCOMPLETE, s.raw(), b"a")
    ok = Stream().dynamic(lits(body), LL_ALL, DL_ALL, final=True)
    add("one_trailing_byte", B.ERR_TRAILING, ok.raw() + b"\0", body)
    add("nine_trailing_bytes", B.ERR_TRAILING, ok.raw() + b"\0" * 9, body)
    add("data_len_1", B.ERR_INPUT_END, b"\x03", b"")             # the first byte of the empty fixed block
    return out


GROUPS = ("copies", "deep", "headers", "blocks", "input_geometry", "output_geometry", "errors")


@functools.lru_cache(maxsize=None)
def cases():
    out = copy_cases() + deep_cases() + header_cases() + block_cases() + input_geometry_cases() + output_geometry_cases() + error_cases()
    assert len({c.name for c in out}) == len(out) and {c.group for c in out} == set(GROUPS)
    return out


def by_group(group):
    return [c for c in cases() if c.group == group]


def good_cases():
    return [c for c in cases() if c.code == 0]
