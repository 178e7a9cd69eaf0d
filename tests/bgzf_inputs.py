"""BGZF inputs for the tests, made with Python's zlib: a member writer, a file writer that cuts like bgzip (or where the caller
says), a bit writer for hand-made DEFLATE streams, and the lists of good blocks and of mutations that the host program
(tests/test_inflate_core_host.py) and the GPU tests (tests/test_gpu_bgzf.py) share."""
import struct
import zlib

import numpy as np

BLOCK_TEXT = 0xff00          # bgzip's text bytes per block
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

# error codes of kreeq_amd/csrc/kq_inflate_core.h
ERR_BTYPE, ERR_STORED_LEN, ERR_HEADER_COUNTS, ERR_OVERSUBSCRIBED, ERR_INCOMPLETE, ERR_REPEAT, ERR_SYMBOL, ERR_DIST_CODE = 1, 2, 3, 4, 5, 6, 7, 8
ERR_DISTANCE, ERR_INPUT_END, ERR_OUTPUT, ERR_TRAILING, ERR_CRC = 9, 10, 11, 12, 13


def member(raw: bytes, crc: int, isize: int, extra_before: bytes = b"") -> bytes:
    """one BGZF member around a raw DEFLATE stream; extra_before: whole extra subfields in front of 'BC'"""
    xlen = len(extra_before) + 6
    size = 12 + xlen + len(raw) + 8
    assert size <= 65536, size
    head = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", xlen) + extra_before + b"BC" + struct.pack("<HH", 2, size - 1)
    return head + raw + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def deflate_raw(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()) -> bytes:
    """raw DEFLATE of data; flush_at: text offsets at which a Z_FULL_FLUSH ends the current DEFLATE block"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, pos = [], 0
    for f in flush_at:
        out.append(c.compress(data[pos:f]))
        out.append(c.flush(zlib.Z_FULL_FLUSH))
        pos = f
    out.append(c.compress(data[pos:]))
    out.append(c.flush())
    return b"".join(out)


def bgzf_block(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), extra_before=b"") -> bytes:
    assert len(data) <= 65536
    return member(deflate_raw(data, level, strategy, flush_at), zlib.crc32(data), len(data), extra_before)


def bgzf_file(text: bytes, level=6, cuts=None, eof=True, empty_at=()) -> bytes:
    """text as a BGZF file: blocks of 0xff00 text bytes like bgzip, or cut at the text offsets `cuts` (ascending, each piece
    <= 65536 bytes); empty_at: indices of blocks in front of which an empty block is put; eof: the 28-byte EOF block"""
    if cuts is None:
        cuts = list(range(BLOCK_TEXT, len(text), BLOCK_TEXT))
    edges = [0] + list(cuts) + [len(text)]
    out = []
    for i in range(len(edges) - 1):
        if i in empty_at:
            out.append(EOF_BLOCK)
        out.append(bgzf_block(text[edges[i]:edges[i + 1]], level))
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def blocks_of(data: bytes):
    """[(off, size, data_off, data_len, crc, isize)] of a BGZF file, in Python (what kq_bgzf_scan must find)"""
    out, pos = [], 0
    while pos < len(data):
        assert data[pos:pos + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", data, pos + 10)[0]
        x, bsize = 0, None
        while x < xlen:
            si1, si2, slen = struct.unpack_from("<BBH", data, pos + 12 + x)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", data, pos + 12 + x + 4)[0]
            x += 4 + slen
        size = bsize + 1
        crc, isize = struct.unpack_from("<II", data, pos + size - 8)
        out.append((pos, size, 12 + xlen, size - xlen - 20, crc, isize))
        pos += size
    return out


class BitWriter:
    """DEFLATE bit order: fields from bit 0 of each byte up; Huffman codes most significant bit first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, v, n):
        for i in range(n - 1, -1, -1):
            self.bits((v >> i) & 1, 1)
        return self

    def fixed_lit(self, s):
        if s < 144:
            return self.code(0x30 + s, 8)
        if s < 256:
            return self.code(0x190 + s - 144, 9)
        if s < 280:
            return self.code(s - 256, 7)
        return self.code(0xC0 + s - 280, 8)

    def done(self) -> bytes:
        if self.n:
            self.out.append(self.acc & 0xFF)
            self.acc, self.n = 0, 0
        return bytes(self.out)


# ---------------------------------------------------------------------------------------------------------------- texts
def fastq_text(n_bytes, seed=1):
    rng = np.random.default_rng(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        n = int(rng.integers(50, 160))
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tolist())
        qual = bytes(rng.choice(np.frombuffer(b"FFFFF:,#", dtype=np.uint8), n).tolist())
        rec = b"@read%d/1\n" % i + seq + b"\n+\n" + qual + b"\n"
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:n_bytes]


def far_reference_text(gap, seed=3):
    """300 bytes, `gap` other bytes, the 300 bytes again: the second copy can only be coded as a match `300 + gap` back"""
    rng = np.random.default_rng(seed)
    head = bytes(rng.integers(128, 256, 300, dtype=np.uint8).tolist())
    other = bytes(rng.integers(0, 64, gap, dtype=np.uint8).tolist())
    return head + other + head


def fibonacci_text():
    """byte frequencies 1, 2, 3, 5, 8, ... 17711 over 21 byte values (with the end-of-block code's 1: a Fibonacci sequence of 22,
    whose optimal code would be 21 bits deep) and three more values 6000 times each: 24 byte values, 64 366 bytes, shuffled.
    DEFLATE limits the code to 15 bits"""
    f = [1, 2]
    while len(f) < 21:
        f.append(f[-1] + f[-2])
    f += [6000] * 3
    data = np.concatenate([np.full(c, 65 + i, dtype=np.uint8) for i, c in enumerate(f)])
    np.random.default_rng(5).shuffle(data)
    assert len(data) <= 65536 and len(f) >= 24
    return data.tobytes()


def good_blocks():
    """{name: (member bytes, text)}: every kind of block the tests decode"""
    fq = fastq_text(BLOCK_TEXT)
    out = {}

    def add(name, text, **kw):
        out[name] = (bgzf_block(text, **kw), text)

    add("empty", b"")
    out["eof_marker"] = (EOF_BLOCK, b"")
    add("one_byte", b"x")
    # one final stored block, written by hand (zlib at level 0 adds an empty final block of 5 bytes): 26 + 5 + 65505 = 65536
    big = bytes(np.random.default_rng(2).integers(0, 256, 65505, dtype=np.uint8).tolist())
    out["stored_max"] = (member(b"\x01" + struct.pack("<HH", 65505, 65505 ^ 0xFFFF) + big, zlib.crc32(big), 65505), big)
    add("stored_70", fq[:70], level=0)
    add("fixed", fq[:3000], strategy=zlib.Z_FIXED)
    for lv in (1, 6, 9):
        add("fastq_level%d" % lv, fq, level=lv)
    add("three_flushes", fq[:20000], flush_at=(5000, 5000, 12000))
    add("A_65536", b"A" * 65536)
    add("far_reference_issue", far_reference_text(32469))      # 33 069 bytes as the issue words it (the copy lies 32 769 back: beyond DEFLATE's reach)
    add("far_reference", far_reference_text(32100))            # the copy lies 32 400 back
    add("all_bytes", bytes(range(256)) + bytes(range(255, -1, -1)))
    add("fibonacci", fibonacci_text(), strategy=zlib.Z_HUFFMAN_ONLY)
    add("second_subfield", fq[:500], extra_before=b"XY" + struct.pack("<H", 3) + b"abc")
    return out


def crafted_distance_before_start() -> bytes:
    """fixed block: literal 'a', then a match of length 3 at distance 2"""
    w = BitWriter().bits(1, 1).bits(1, 2)
    w.fixed_lit(ord("a")).fixed_lit(257).code(1, 5)           # length symbol 257 = 3, distance code 1 = 2
    w.fixed_lit(256)
    return w.done()


def crafted_oversubscribed() -> bytes:
    """dynamic block whose code-length code gives three symbols one bit each"""
    w = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)      # HLIT 257, HDIST 1, HCLEN 4: 16, 17, 18, 0
    for v in (1, 1, 1, 0):
        w.bits(v, 3)
    w.bits(0, 16)
    return w.done()


def crafted_hlit_287() -> bytes:
    w = BitWriter().bits(1, 1).bits(2, 2).bits(30, 5).bits(0, 5).bits(0, 4)
    w.bits(0, 32)
    return w.done()


def mutations(block: bytes, text: bytes):
    """[(name, member bytes, expected error code)] of a good dynamic-Huffman member: the mutations of the issue's list.  The
    member layout is that of member() without extra_before: 18 header bytes, data, 8 trailer bytes."""
    raw, crc, isize = block[18:-8], zlib.crc32(text), len(text)
    assert (raw[0] >> 1) & 3 == 2 and isize > 10
    stored = bgzf_block(text[:50], level=0)
    sraw = bytearray(stored[18:-8])
    sraw[3] ^= 0x10                                           # NLEN
    btype3 = bytearray(raw)
    btype3[0] |= 0x06
    return [
        ("isize_plus_1", member(raw, crc, isize + 1), ERR_OUTPUT),
        ("isize_minus_1", member(raw, crc, isize - 1), ERR_OUTPUT),
        ("crc_bit", member(raw, crc ^ 0x00040000, isize), ERR_CRC),
        ("data_len_minus_1", member(raw[:-1], crc, isize), ERR_INPUT_END),
        ("data_len_half", member(raw[:len(raw) // 2], crc, isize), ERR_INPUT_END),
        ("btype_3", member(bytes(btype3), crc, isize), ERR_BTYPE),
        ("stored_nlen", member(bytes(sraw), zlib.crc32(text[:50]), 50), ERR_STORED_LEN),
        ("distance_before_start", member(crafted_distance_before_start(), zlib.crc32(b"aaaa"), 4), ERR_DISTANCE),
        ("oversubscribed", member(crafted_oversubscribed(), crc, isize), ERR_OVERSUBSCRIBED),
        ("hlit_287", member(crafted_hlit_287(), crc, isize), ERR_HEADER_COUNTS),
    ]
