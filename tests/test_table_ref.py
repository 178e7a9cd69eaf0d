"""tests/table_ref.py -- the yardstick of the per-base table tests -- against the reference's own goldens: `lookup`
(validateFiles/test.48.tst), `inflate` (test.49.tst), and the .kwig body that the two committed .bkwig files stand for."""
import os

import numpy as np

from tests import helpers as H
from tests import table_ref as T


def golden(name):
    return open(H.golden_input(name), "rb").read()


def tst_stdout(n):
    _, exp = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", "test.%d.tst" % n))
    return exp


def lines_of(text):
    out = text.decode().split("\n")
    while out and out[-1] == "":
        out.pop()
    return out


def bed_ranges(name):
    return [(w[0].encode(), int(w[1]), int(w[2])) for w in (l.split() for l in open(H.golden_input(name))) if w]


def test_lookup_golden():
    assert lines_of(T.lookup(golden("decompressor1.bkwig"), bed_ranges("decompressor1.bed"))) == tst_stdout(48)


def test_inflate_golden():
    assert lines_of(T.inflate(golden("decompressor2.bkwig"))) == tst_stdout(49)


def test_index_and_payload_sizes():
    for name in ("decompressor1.bkwig", "decompressor2.bkwig"):
        b = T.Bkwig(golden(name))
        assert b.k == 21 and len(b.payload) == b.payload_expected and b.payload_expected == 12 * sum(n for _, comps in b.paths for _, n, _, _ in comps)
        paths = [(h, [(a, n) for a, n, _, _ in comps]) for h, comps in b.paths]
        assert T.write_bkwig(b.k, paths, b.triples()) == golden(name)          # the index writer is the reader's inverse


def test_kwig_body_from_bkwig():
    """the .kwig text of a .bkwig, rebuilt line by line with plain string formatting"""
    for name in ("decompressor1.bkwig", "decompressor2.bkwig"):
        b = T.Bkwig(golden(name))
        t = b.triples()
        want, g = ["21"], 0
        for header, comps in b.paths:
            for abs_pos, n, _, _ in comps:
                want.append("fixedStep chrom=%s start=%d step=1" % (header.decode(), abs_pos))
                want += ["%d,%d,%d" % tuple(t[g + i]) for i in range(n)]
                g += n
        assert lines_of(T.inflate(golden(name))) == want


def test_expanded_layout_by_hand():
    """k = 3: every window spelled out, history (n_ctx) and zeros before it, both separator sets"""
    t = np.array([[1, 20, 300], [4, 50, 600], [7, 80, 900], [10, 11, 12]], dtype=np.uint32)
    whole = [T.Piece(0, 4, 9, b"s")]
    assert T.format_table(T.CSV, 3, t, whole) == (b"s,9,0,0,1,0,0,20,0,0,300\n" b"s,10,0,1,4,0,20,50,0,300,600\n" b"s,11,1,4,7,20,50,80,300,600,900\n"
                                                 b"s,12,4,7,10,50,80,11,600,900,12\n")
    assert T.format_table(T.BED, 3, t, [T.Piece(1, 1, 10, b"s", 1)]) == b"s\t10\t0:1:4\t0:20:50\t0:300:600\n"
    cut = [T.Piece(0, 2, 9, b"s"), T.Piece(2, 2, 11, b"s", 2)]
    assert T.format_table(T.CSV, 3, t, cut) == T.format_table(T.CSV, 3, t, whole)
    assert T.format_table(T.CSV, 3, t, [T.Piece(0, 2, 9, b"s"), T.Piece(2, 2, 11, b"s", 0)]) != T.format_table(T.CSV, 3, t, whole)      # no history: no leak
    assert T.format_table(T.KWIG, 3, t, [T.Piece(2, 2, 5, b"chr", 0, True)]) == b"fixedStep chrom=chr start=5 step=1\n7,80,900\n10,11,12\n"


def test_triples_orientation():
    pb = np.zeros(5, dtype=np.dtype([("fw", "<u4"), ("bw", "<u4"), ("cov", "<u4"), ("isFw", "u1"), ("pad", "u1", 3)]))
    pb["fw"], pb["bw"], pb["cov"], pb["isFw"] = [1, 2, 3, 4, 5], [10, 20, 30, 40, 50], [7, 8, 9, 6, 5], [1, 0, 1, 0, 0]
    assert T.triples_of(pb, [(0, 2), (3, 2)]).tolist() == [[7, 1, 10], [8, 20, 2], [6, 40, 4], [5, 50, 5]]


def test_lookup_span_and_refusals():
    data = golden("decompressor1.bkwig")
    one = T.lookup(data, [(b"sequence1", 20, 30)], span=2)
    assert lines_of(one)[1] == "sequence1:18-32" and len(lines_of(one)) == 2 + 14
    for bad in ([(b"nobody", 1, 2)], [(b"sequence1", 10 ** 6, 10 ** 6 + 2)], [(b"sequence1", 0, 5)]):
        try:
            T.lookup(data, bad)
        except T.LookupError_:
            continue
        raise AssertionError(bad)
