"""A small inflater (RFC 1951) that returns the TOKENS of a raw DEFLATE stream instead of its bytes: the suite's way to see which
matches a compressor took.  Stored, fixed and dynamic blocks; nothing here is shared with the project's own inflater."""

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Bits:
    def __init__(self, data):
        self.data, self.pos, self.acc, self.n = data, 0, 0, 0

    def need(self, k):
        while self.n < k:
            chunk = self.data[self.pos:self.pos + 8]
            self.pos += 8                                           # (past the end: zero bits, caught by `overrun` below)
            self.acc |= int.from_bytes(chunk, "little") << self.n
            self.n += 64

    def take(self, k):
        self.need(k)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def used_bits(self):
        return 8 * self.pos - self.n

    def to_byte(self):
        self.take(self.n % 8)


class Code:
    """a canonical Huffman code as a table over the next `width` bits (LSB first): entry = (symbol, length)"""

    def __init__(self, lengths):
        self.width = max(lengths)                                   # 0: a set without codes (no match in the block), never read
        assert self.width <= 15
        count = [0] * 16
        for l in lengths:
            count[l] += 1
        count[0] = 0
        nxt, code = [0] * 16, 0
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        assert sum(c << (15 - l) for l, c in enumerate(count) if l) <= 1 << 15, "an over-subscribed code"
        self.table = [None] * (1 << self.width)
        for sym, l in enumerate(lengths):
            if not l:
                continue
            c, nxt[l] = nxt[l], nxt[l] + 1
            r = int(format(c, "0%db" % l)[::-1], 2)                 # the writer sends a code's first bit first
            for k in range(r, 1 << self.width, 1 << l):
                self.table[k] = (sym, l)

    def read(self, b):
        b.need(self.width)
        e = self.table[b.acc & ((1 << self.width) - 1)]
        assert e is not None, "bits that are no code"
        b.acc >>= e[1]
        b.n -= e[1]
        return e[0]


FIXED_LIT = Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = Code([5] * 32)


def read_dynamic_codes(b):
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    clen = [0] * 19
    for i in range(hclen):
        clen[CLEN_ORDER[i]] = b.take(3)
    cc = Code(clen)
    lens = []
    while len(lens) < hlit + hdist:
        s = cc.read(b)
        if s < 16:
            lens.append(s)
        elif s == 16:
            assert lens, "a repeat with nothing before it"
            lens += [lens[-1]] * (3 + b.take(2))
        else:
            lens += [0] * (3 + b.take(3) if s == 17 else 11 + b.take(7))
    assert len(lens) == hlit + hdist, "a run past the last length"
    assert lens[256], "no end-of-block code"
    return Code(lens[:hlit]), Code(lens[hlit:])


def tokens_of(raw):
    """raw DEFLATE data -> (kind, tokens): kind is "stored", "fixed" or "dynamic" (or several joined by "+" when the blocks of
    a stream differ), a token is (literal,) or (length, distance); a stored block yields its bytes as literals"""
    b = Bits(bytes(raw))
    kinds, out, size = [], [], 0
    final = 0
    while not final:
        final, btype = b.take(1), b.take(2)
        assert btype != 3, "block type 3"
        kind = ("stored", "fixed", "dynamic")[btype]
        if kind not in kinds:
            kinds.append(kind)
        if btype == 0:
            b.to_byte()
            n, inv = b.take(16), b.take(16)
            assert n ^ inv == 0xFFFF, "LEN and NLEN disagree"
            for _ in range(n):
                out.append((b.take(8),))
            size += n
            continue
        lit, dist = (FIXED_LIT, FIXED_DIST) if btype == 1 else read_dynamic_codes(b)
        while True:
            s = lit.read(b)
            if s < 256:
                out.append((s,))
                size += 1
            elif s == 256:
                break
            else:
                assert s <= 285, "length code %d" % s
                length = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
                d = dist.read(b)
                assert d <= 29, "distance code %d" % d
                d = DIST_BASE[d] + b.take(DIST_EXTRA[d])
                assert d <= size, "a distance of %d after %d bytes" % (d, size)
                out.append((length, d))
                size += length
    assert b.used_bits() <= 8 * len(raw), "the stream ends inside a block"
    assert (b.used_bits() + 7) // 8 == len(raw), "%d bytes behind the last block" % (len(raw) - (b.used_bits() + 7) // 8)
    return "+".join(kinds), out
