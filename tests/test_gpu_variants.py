"""kq_search_variants through the C ABI (ctypes binding) against `dbg_to_variants` of oracle/variants.py on the oracle's table
of the same reads.  Every comparison is exact: positions, order, types, refLen and sequences.  Inputs: tests/variant_cases.py,
tests/scan_inputs.py."""
import numpy as np
import pytest

from oracle import variants as V
from tests import bestfirst_cases as B
from tests import scan_inputs as S
from tests import variant_cases as C

pytestmark = pytest.mark.gpu

MAPS = 128
ERR_INVALID, ERR_CAPACITY = -1, -6


@pytest.fixture(scope="module")
def kq():
    from kreeq_amd import capi
    assert capi.device_available()
    return capi


def counted(kq, k, reads, hint=1 << 16):
    db = kq.KreeqDB(k, MAPS, 0, capacity_hint=hint)
    db.count_batch(reads if isinstance(reads, bytes) else reads.encode())
    return db


want_of = C.want_of


def check(db, g, text, depth, span, cutoff=0):
    text_b = text if isinstance(text, bytes) else text.encode()
    got = db.search_variants(text_b, depth, span, cutoff)
    want = want_of(g, text, depth, span)
    assert got == want
    return want


@pytest.fixture(scope="module")
def planted(kq):
    """the k = 21 planted-error text behind a second segment, a run shorter than k and a lower-case stretch: ~2 kb"""
    k = 21
    reads, asm, genome = C.planted(k, n=1400)
    text = asm[:700] + "N" + asm[700:710] + "NN" + asm[710:1000] + asm[1000:1200].lower() + asm[1200:] + "\n" + asm[90:160]
    return k, counted(kq, k, reads), C.graph_of(k, reads), text


def test_planted_errors(planted):
    k, db, g, text = planted
    want = check(db, g, text, 60, 32)
    assert {p[2] for p in want} == {0, 1, 2, 3}
    assert len({p[1] for p in want}) >= 2                              # sites in more than one segment
    for depth, span in ((0, 32), (1, 5), (k, 1), (60, 0), (60, 255), (253, 32)):
        check(db, g, text, depth, span)


def test_cutoff(kq, monkeypatch):
    k = 21
    reads, genome = C.thin(k)
    db, g = counted(kq, k, reads), C.graph_of(k, reads)
    results = []
    for cutoff in (0, 1, 3):
        with monkeypatch.context() as m:
            C.with_cutoff(m, cutoff)
            results.append(check(db, g, genome, 30, 32, cutoff))
    assert results[0] != results[2]


@pytest.mark.parametrize("k", [5, 31, 32])
def test_other_k(kq, k):
    """k = 5: a dense graph (more than 64 flagged positions: several waves, windows with repeated keys); k = 31 / 32: wide keys"""
    if k == 5:
        text = B.dense(k)[0].decode()
        db, g = counted(kq, k, text), C.graph_of(k, text)
        want = check(db, g, text, 40, 32)
        assert len({p[0] for p in want}) > 64
        check(db, g, text, 253, 255)
        return
    reads, asm, _ = C.planted(k, seed=k)
    db, g = counted(kq, k, reads), C.graph_of(k, reads)
    assert {p[2] for p in check(db, g, asm, 60, 32)} == {0, 1, 2, 3}


@pytest.mark.parametrize("lead", [0, 1])
def test_scanner_edges(kq, lead):
    """the texts of tests/scan_inputs.py (nine scanner tiles; run ends on and across tile edges; the text built for an odd
    lead) against the table of their reads: the pre-filter, the position list and the segment bounds across tiles"""
    k = 21
    ref = S.reference(k, lead)
    db = counted(kq, k, ref.reads, hint=1 << 18)
    g = V.Graph(ref.table, k)
    g.nodes = C.ZeroNodes(g.nodes)
    want = check(db, g, ref.text, 30, 16)
    assert len({p[0] for p in want}) > 64 and len({p[1] for p in want}) > 4
    assert max(p[0] for p in want) > 2 * S.T                            # sites behind a tile boundary


def test_batch_size_does_not_matter(planted):
    """variant_batch 0 (automatic), 1 and 7: byte-identical records and sequence bytes"""
    k, db, g, text = planted
    raw = []
    for batch in (0, 1, 7):
        db.set_option("variant_batch", batch)
        rc, n_paths, n_seq, paths, seq = db.search_variants_raw(text.encode(), 60, 32, 0, 1 << 12, 1 << 16)
        assert rc == 0 and n_paths > 4
        raw.append((n_paths, n_seq, paths[:n_paths].tobytes(), seq[:n_seq].tobytes()))
    db.set_option("variant_batch", 0)
    assert raw[0] == raw[1] == raw[2]


def test_capacity_protocol(planted):
    k, db, g, text = planted
    want = want_of(g, text, 60, 32)
    n_seq_want = sum(len(p[4]) for p in want)
    rc, n_paths, n_seq, _, _ = db.search_variants_raw(text.encode(), 60, 32)              # NULL query: the counts
    assert (rc, n_paths, n_seq) == (0, len(want), n_seq_want)
    for path_cap, seq_cap in ((n_paths - 1, n_seq), (n_paths, n_seq - 1), (1, 1)):
        rc, a, b, paths, seq = db.search_variants_raw(text.encode(), 60, 32, 0, path_cap, seq_cap)
        assert (rc, a, b) == (ERR_CAPACITY, n_paths, n_seq)
        assert not paths.tobytes().strip(b"\0") and not seq.tobytes().strip(b"\0")        # nothing written
    rc, a, b, paths, seq = db.search_variants_raw(text.encode(), 60, 32, 0, n_paths, n_seq)
    assert (rc, a, b) == (0, n_paths, n_seq)
    assert db.search_variants(text.encode(), 60, 32) == want          # and the handle is usable after the refusals
    rc, a, b, _, _ = db.search_variants_raw(text.encode()[:k - 1], 60, 32, 0, 4, 4)      # len < k
    assert (rc, a, b) == (0, 0, 0)


def test_invalid_arguments(kq, planted):
    import ctypes as ct

    k, db, g, text = planted
    lib = kq.load()
    buf = np.frombuffer(text.encode(), dtype=np.uint8)
    n = ct.c_uint64(0)
    for depth, span in ((-1, 32), (254, 32), (60, -1), (60, 256)):
        rc, _, _, _, _ = db.search_variants_raw(text.encode(), depth, span)
        assert rc == ERR_INVALID, (depth, span)
    p = buf.ctypes.data_as(ct.c_void_p)
    assert lib.kq_search_variants(db._h, p, len(buf), 60, 32, 0, None, 0, None, None, 0, ct.byref(n)) == ERR_INVALID      # null n_paths
    assert lib.kq_search_variants(db._h, p, len(buf), 60, 32, 0, None, 0, ct.byref(n), None, 0, None) == ERR_INVALID      # null n_seq
    assert lib.kq_search_variants(db._h, None, len(buf), 60, 32, 0, None, 0, ct.byref(n), None, 0, ct.byref(n)) == ERR_INVALID
    assert lib.kq_search_variants(db._h, p, 0xFFFFFFFF, 60, 32, 0, None, 0, ct.byref(n), None, 0, ct.byref(n)) == ERR_INVALID      # len >= 2^32 - 1 (refused before the text is read)
    win = kq.KreeqDB(k, MAPS, 0, capacity_hint=1 << 12)
    win.set_option("bucket_window", 0 | (128 << 16))
    rc, _, _, _, _ = win.search_variants_raw(text.encode(), 60, 32)
    assert rc == ERR_INVALID                                           # a windowed handle
    assert db.search_variants(text.encode(), 60, 32) == want_of(g, text, 60, 32)      # usable after the refusals
