"""kq_format_table / kq_format_table_dev / kq_per_base_triples_dev (kreeq_amd/csrc/kq_table.h) against tests/table_ref.py, byte
for byte: segment lengths around the tile (256 lines) and its multiples, every k the window code distinguishes, names of 1, 7
and 300 bytes, values and coordinates at every digit boundary, pieces at the window's edges, and the contract of the call
(size query, capacity, refusals)."""
import ctypes as C

import numpy as np
import pytest

from kreeq_amd import KreeqDB, capi
from tests import table_cases as TC
from tests import table_ref as T

pytestmark = pytest.mark.gpu

KS = (2, 21, 31, 32)
FORMATS = (T.KWIG, T.BED, T.CSV)
ERR_INVALID, ERR_CAPACITY = -1, -6
assert TC.TILE == 256 and all(n in TC.SEGMENT_LENGTHS for n in (TC.TILE - 1, TC.TILE, TC.TILE + 1))      # the tile's own edges are in the list


@pytest.fixture(scope="module")
def dbs():
    return {k: KreeqDB(k, 128, device=0, capacity_hint=1024) for k in KS}


def gpu_text(db, fmt, t, pieces):
    segs, names = T.pack_pieces(pieces)
    return db.format_table(fmt, t, segs, names)


def check(db, fmt, t, pieces):
    got = gpu_text(db, fmt, t, pieces)
    want = T.format_table(fmt, db.k, t, pieces)
    assert len(got) == len(want) and got == want, (fmt, db.k, len(t), len(pieces))
    return got


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_segment_lengths(dbs, fmt, k):
    for i, n in enumerate(TC.SEGMENT_LENGTHS):
        t, pieces = TC.one_segment(n, 100 * k + i, TC.NAMES[(1, 7, 300)[i % 3]], TC.ABS_EDGES[i % len(TC.ABS_EDGES)])
        check(dbs[k], fmt, t, pieces)


@pytest.mark.parametrize("fmt,k", [(T.KWIG, 21), (T.BED, 21), (T.CSV, 21), (T.CSV, 32)])
def test_long_segment(dbs, fmt, k):
    """70 001 positions: 274 tiles, in the expanded formats several LDS windows of text per tile"""
    t, pieces = TC.one_segment(70001, 9, TC.NAMES[7], 2 ** 32 - 40)
    check(dbs[k], fmt, t, pieces)


def test_more_tiles_than_one_scan_workgroup_takes(dbs):
    """2 x 16384 tiles is where the project's scan changes from one workgroup to chunk sums + apply: 8 388 908 one-digit
    lines (6 bytes each, so numpy can spell the expected text) under one header line"""
    n = 2 * 16384 * TC.TILE + 300
    t = np.random.default_rng(12).integers(0, 10, (n, 3), dtype=np.uint32)
    pieces = [T.Piece(0, n, 3, b"chr", 0, True)]
    got = gpu_text(dbs[21], T.KWIG, t, pieces)
    head = b"fixedStep chrom=chr start=3 step=1\n"
    assert got[:len(head)] == head and len(got) == len(head) + 6 * n
    want = np.empty((n, 6), dtype=np.uint8)
    want[:, 0::2] = t + 48
    want[:, 1], want[:, 3], want[:, 5] = 44, 44, 10
    assert np.array_equal(np.frombuffer(got, dtype=np.uint8)[len(head):].reshape(n, 6), want)
    assert got[len(head):len(head) + 6000] == T.format_table(T.KWIG, 21, t[:1000], [T.Piece(0, 1000, 3, b"chr")])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_coordinates_and_names(dbs, fmt, k):
    for i, abs_pos in enumerate(TC.ABS_EDGES):
        for name_len in (1, 7, 300):
            t, pieces = TC.one_segment(130, 7 * k + i, TC.NAMES[name_len], abs_pos)
            check(dbs[k], fmt, t, pieces)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fmt", (T.BED, T.CSV))
def test_segments_around_k(dbs, fmt, k):
    for n in (1, k - 1, k, k + 1):
        check(dbs[k], fmt, *TC.one_segment(n, n, header=False))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_no_leak_across_pieces(dbs, fmt, k):
    t, pieces = TC.big_then_one(k)
    got = check(dbs[k], fmt, t, pieces)
    last = got.rstrip(b"\n").split(b"\n")[-1]
    assert b"4294967295" not in last


@pytest.mark.parametrize("k", (2, 21, 32))
def test_cut_at_every_position(dbs, k):
    db = dbs[k]
    for fmt in (T.KWIG, T.CSV):
        t, whole, _ = TC.cut_in_two(k, 1)
        want = check(db, fmt, t, whole)
        for cut in range(1, 100):
            _, _, two = TC.cut_in_two(k, cut)
            assert gpu_text(db, fmt, t, two) == want, (fmt, k, cut)


@pytest.mark.parametrize("fmt", FORMATS)
def test_many_small_pieces(dbs, fmt):
    t, pieces = TC.many_pieces(3)
    assert len(pieces) == 300
    check(dbs[21], fmt, t, pieces)


def test_nothing_to_format(dbs):
    db = dbs[21]
    assert gpu_text(db, T.KWIG, np.zeros((0, 3), dtype=np.uint32), []) == b""
    t = TC.values(4, 1)
    empty = [T.Piece(0, 0, 5, b"a", 0, True), T.Piece(2, 0, 100000, b"bb", 0, True), T.Piece(4, 0, 0, b"c", 0, False)]
    assert check(db, T.KWIG, t, empty) == b"fixedStep chrom=a start=5 step=1\nfixedStep chrom=bb start=100000 step=1\n"
    assert check(db, T.CSV, t, empty) == b""


# ---- the device entry point: size query, capacity, alignment ---------------------------------------------------------------

def dev_call(db, fmt, d_triples, n_triples, pieces, out_ptr, cap):
    segs, names = T.pack_pieces(pieces)
    nb = np.frombuffer(names, dtype=np.uint8)
    return db.format_table_raw(fmt, C.c_void_p(d_triples), n_triples, segs.ctypes.data_as(C.c_void_p), len(segs), nb.ctypes.data_as(C.c_void_p), len(nb),
                               C.c_void_p(out_ptr) if out_ptr else None, cap, dev=True)


@pytest.mark.parametrize("fmt", FORMATS)
def test_size_query_capacity_and_alignment(dbs, fmt):
    import torch

    db = dbs[21]
    t, pieces = TC.one_segment(700, 4, TC.NAMES[7], 99990)
    want = T.format_table(fmt, 21, t, pieces)
    d_t = torch.from_numpy(t.view(np.int32)).cuda()
    rc, need = dev_call(db, fmt, d_t.data_ptr(), len(t), pieces, None, 0)
    assert rc == 0 and need == len(want)
    for lead in (0, 1, 7, 15):                                            # the output's first and last 16-byte word are partial
        buf = torch.full((lead + need + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        rc, n = dev_call(db, fmt, d_t.data_ptr(), len(t), pieces, buf.data_ptr() + lead, need)
        assert rc == 0 and n == need
        host = buf.cpu().numpy()
        assert host[lead:lead + need].tobytes() == want
        assert (host[:lead] == 0x5A).all() and (host[lead + need:] == 0x5A).all()
    buf = torch.full((need - 1 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, n = dev_call(db, fmt, d_t.data_ptr(), len(t), pieces, buf.data_ptr(), need - 1)
    assert rc == ERR_CAPACITY and n == need
    assert (buf.cpu().numpy()[need - 1:] == 0x5A).all()                   # the 64 guard bytes behind cap


def test_refusals(dbs):
    db = dbs[21]
    t = TC.values(50, 2)
    segs, names = T.pack_pieces([T.Piece(25, 20, 0, b"name", 5, True)])
    nb = np.frombuffer(names, dtype=np.uint8)
    tp, sp, np_ = t.ctypes.data_as(C.c_void_p), segs.ctypes.data_as(C.c_void_p), nb.ctypes.data_as(C.c_void_p)

    def rc_of(fmt=T.CSV, triples=tp, n_triples=50, s=sp, n_segs=1, names_ptr=np_, names_len=len(nb), n_out=True, handle=db):
        return handle.format_table_raw(fmt, triples, n_triples, s, n_segs, names_ptr, names_len, None, 0, n_out=n_out)[0]

    assert rc_of() == 0
    assert rc_of(n_out=False) == ERR_INVALID                              # null pointers
    assert rc_of(triples=None) == ERR_INVALID
    assert rc_of(s=None) == ERR_INVALID
    assert rc_of(names_ptr=None) == ERR_INVALID
    assert rc_of(fmt=0) == ERR_INVALID and rc_of(fmt=4) == ERR_INVALID    # an unknown format
    assert "format" in capi.load().kq_last_error().decode()

    def with_seg(**kw):
        s = segs.copy()
        for f, v in kw.items():
            s[0][f] = v
        return rc_of(s=s.ctypes.data_as(C.c_void_p))

    assert with_seg(n_ctx=20) == 0 and with_seg(n_ctx=21) == ERR_INVALID          # n_ctx > k - 1
    assert with_seg(first=10, n_ctx=11) == ERR_INVALID and with_seg(first=10, n_ctx=10) == 0      # n_ctx > first
    assert rc_of(handle=dbs[2]) == ERR_INVALID                                    # (k = 2: n_ctx 5 > 1)
    assert with_seg(n=25) == 0 and with_seg(n=26) == ERR_INVALID                  # a piece that runs past n_triples
    assert with_seg(first=51, n=0) == ERR_INVALID and with_seg(first=2 ** 64 - 1) == ERR_INVALID
    assert with_seg(name_off=1) == ERR_INVALID and with_seg(name_off=2 ** 32 - 1) == ERR_INVALID      # a name outside names
    assert with_seg(name_len=5) == ERR_INVALID and with_seg(name_off=4, name_len=0) == 0


def test_too_many_lines(dbs):
    """2^32 lines in one call are refused before any device work (the triples are never touched: the pointer is a dummy)"""
    db = dbs[21]
    segs, names = T.pack_pieces([T.Piece(0, 2 ** 31, 0, b"a"), T.Piece(0, 2 ** 31, 0, b"a")])
    dummy = np.zeros(4, dtype=np.uint32)
    rc, _ = db.format_table_raw(T.KWIG, dummy.ctypes.data_as(C.c_void_p), 2 ** 31, segs.ctypes.data_as(C.c_void_p), 2, np.frombuffer(names, dtype=np.uint8).ctypes.data_as(C.c_void_p),
                                len(names), None, 0)
    assert rc == ERR_INVALID and "2^32" in capi.load().kq_last_error().decode()


def test_per_base_triples(dbs):
    import torch

    db = dbs[21]
    rng = np.random.default_rng(8)
    n = 5000
    pb = np.zeros(n, dtype=capi.DBGBASE_DTYPE)
    pb["fw"], pb["bw"], pb["cov"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64), rng.integers(0, 1000, n), rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    pb["isFw"] = rng.integers(0, 2, n)
    segments = [(0, 1), (2, 255), (258, 257), (600, 0), (601, 1024), (1700, 3299), (4999, 1)]      # separators between them, an empty one, the array's last entry
    want = T.triples_of(pb, segments)
    total = sum(s[1] for s in segments)
    d_pb = torch.from_numpy(pb.view(np.uint8)).cuda()
    d_out = torch.full((total * 3 + 16,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    db.per_base_triples_dev(d_pb.data_ptr(), segments, d_out.data_ptr())
    db.sync()
    got = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:total * 3].reshape(-1, 3), want)
    assert (got[total * 3:] == 0xFFFFFFFF).all()
    assert {0, 1} <= set(pb["isFw"][:300].tolist())
