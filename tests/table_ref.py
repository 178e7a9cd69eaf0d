"""Python restatement of the per-base tables: the oriented triples of a .bkwig payload, the two text layouts
(kreeq_amd/csrc/kq_table_core.h; reference src/kreeq-output.cpp:176-219, :275-281, src/decompressor.cpp:510-579), the .bkwig
index (src/kreeq-output.cpp:305-355, src/decompressor.cpp:78-117) and `kreeq-decompressor lookup` (src/decompressor.cpp:119-249).
It is the yardstick of the table tests; tests/test_table_ref.py pins it against the reference's goldens."""
import struct

import numpy as np

KWIG, BED, CSV = 1, 2, 3                  # KQ_TABLE_*
SEG_HEADER = 1                            # KQ_TABLE_SEG_HEADER
SEG_DTYPE = np.dtype([("first", "<u8"), ("n", "<u8"), ("abs_pos", "<u8"), ("name_off", "<u4"), ("name_len", "<u4"), ("n_ctx", "<u4"), ("flags", "<u4")])      # kq_table_seg
SEPARATORS = {BED: (b"\t", b":"), CSV: (b",", b",")}      # format -> (column, entry)


def triples_of(per_base, segments):
    """per_base: structured array with fw, bw, cov, isFw; segments: [(start, len)] -> uint32 [sum len, 3]: cov, the edge
    counter in the orientation of the k-mer, the other one"""
    out = []
    for start, n in segments:
        e = per_base[start:start + n]
        fw = e["isFw"] != 0
        out.append(np.stack([e["cov"], np.where(fw, e["fw"], e["bw"]), np.where(fw, e["bw"], e["fw"])], axis=1).astype(np.uint32))
    return np.concatenate(out) if out else np.zeros((0, 3), dtype=np.uint32)


class Piece:
    def __init__(self, first, n, abs_pos, name, n_ctx=0, header=False):
        self.first, self.n, self.abs_pos, self.name, self.n_ctx, self.header = first, n, abs_pos, name, n_ctx, header


def pack_pieces(pieces):
    """-> (kq_table_seg array, names bytes): every distinct name once"""
    names, where = b"", {}
    segs = np.zeros(len(pieces), dtype=SEG_DTYPE)
    for i, p in enumerate(pieces):
        if p.name not in where:
            where[p.name] = len(names)
            names += p.name
        segs[i] = (p.first, p.n, p.abs_pos, where[p.name], len(p.name), p.n_ctx, SEG_HEADER if p.header else 0)
    return segs, names


def format_table(fmt, k, triples, pieces):
    """the text kq_format_table must produce"""
    t = np.asarray(triples, dtype=np.uint32).reshape(-1, 3)
    text = [[b"%d" % v for v in t[:, c].tolist()] for c in range(3)]
    out = []
    for p in pieces:
        if fmt == KWIG:
            if p.header:
                out.append(b"fixedStep chrom=%s start=%d step=1\n" % (p.name, p.abs_pos))
            for g in range(p.first, p.first + p.n):
                out.append(text[0][g] + b"," + text[1][g] + b"," + text[2][g] + b"\n")
            continue
        col, ent = SEPARATORS[fmt]
        for i in range(p.n):
            lo = max(i - k + 1, -p.n_ctx)                    # the oldest position the window may read
            zeros = [b"0"] * (lo - (i - k + 1))
            out.append(p.name + col + b"%d" % (p.abs_pos + i) + col + col.join(ent.join(zeros + text[c][p.first + lo:p.first + i + 1]) for c in range(3)) + b"\n")
    return b"".join(out)


# ---- .bkwig ------------------------------------------------------------------------------------------------------------

class Bkwig:
    """k, paths = [(header, [(abs_pos, len, step, byte_pos)])] in file order, index_bytes (without the k byte), payload"""

    def __init__(self, data):
        self.k = data[0]
        at = 1
        (n_paths,) = struct.unpack_from("<I", data, at)
        at += 4
        self.paths, byte_pos = [], 0
        for _ in range(n_paths):
            (hl,) = struct.unpack_from("<H", data, at)
            header = data[at + 2:at + 2 + hl]
            at += 2 + hl
            (nc,) = struct.unpack_from("<I", data, at)
            at += 4
            comps = []
            for _ in range(nc):
                abs_pos, n, step = struct.unpack_from("<QQB", data, at)
                at += 17
                comps.append((abs_pos, n, step, byte_pos))
                byte_pos += 12 * n
            self.paths.append((header, comps))
        self.index_bytes = at - 1
        self.payload = data[at:]
        self.payload_expected = byte_pos

    def triples(self):
        return np.frombuffer(self.payload[:len(self.payload) // 12 * 12], dtype="<u4").reshape(-1, 3)

    def pieces(self, header=True):
        """one piece per component, in file order"""
        return [Piece(bp // 12, n, abs_pos, h, 0, header) for h, comps in self.paths for abs_pos, n, _, bp in comps]


def write_bkwig(k, paths, triples):
    """paths = [(header bytes, [(abs_pos, len)])]; triples: the payload"""
    out = [struct.pack("<BI", k, len(paths))]
    for header, comps in paths:
        out.append(struct.pack("<H", len(header)) + header + struct.pack("<I", len(comps)))
        for abs_pos, n in comps:
            out.append(struct.pack("<QQB", abs_pos, n, 1))
    return b"".join(out) + np.asarray(triples, dtype="<u4").tobytes()


def inflate(data, expand=False):
    """`kreeq-decompressor inflate [--expand]` -> stdout"""
    b = Bkwig(data)
    if len(b.payload) != b.payload_expected:
        return b"Error: file truncated\n"
    if expand:
        return format_table(CSV, b.k, b.triples(), b.pieces(False))
    return b"%d\n" % b.k + format_table(KWIG, b.k, b.triples(), b.pieces(True))


class LookupError_(Exception):
    pass


def lookup(data, ranges, span=0):
    """`kreeq-decompressor lookup`: ranges = [(header bytes, begin, end)] in file order -> stdout.  Headers in order of first
    appearance, a header's ranges in file order.  The offset arithmetic is the reference's (src/decompressor.cpp:136-151), with
    its quirk: a range that does not end strictly inside the component of its start keeps the PAYLOAD-START offset."""
    b = Bkwig(data)
    index = dict(b.paths)
    by_header = {}
    for header, begin, end in ranges:
        by_header.setdefault(header, []).append((begin, end))
    out = [b"%d\n" % b.k]
    for header, rs in by_header.items():
        if header not in index:
            raise LookupError_("Could not find header (%s)" % header.decode())
        for begin, end in rs:
            if begin < span + 1:
                raise LookupError_("range start before the sequence")
            start, end = begin - span - 1, end + span - 1
            offset, found = 0, False                              # relative to the payload
            for abs_pos, n, _, byte_pos in index[header]:
                if not abs_pos <= start < abs_pos + n:
                    continue
                found = True
                if end > abs_pos + n:
                    end = abs_pos + n
                elif abs_pos + n > end:
                    offset += byte_pos + (start - abs_pos) * 12
                    break
            if not found:
                raise LookupError_("range start outside every component")
            n = max(end - start, 0)
            vals = np.frombuffer(b.payload[offset:offset + 12 * n], dtype="<u4").reshape(-1, 3)
            out.append(b"%s:%d-%d\n" % (header, start + 1, end + 1))
            out.append(format_table(KWIG, b.k, vals, [Piece(0, len(vals), 0, b"", 0, False)]))
            out.append(b"\n")
    return b"".join(out)
