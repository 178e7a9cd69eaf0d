"""kq_subgraph_gfa against the restatement tests/gfa_ref.py: segments, sequence, edges and counts must be equal, record by
record, in both modes -- on the subgraphs of tests/subgraph_inputs.py at k = 4, 8, 21, 31, 32, on three goldens and on the
hand-made graphs of tests/gfa_cases.py (cycles, hairpin, self-loop, palindrome, isolated k-mer, asymmetric and trimmed counters,
cov 300, a unitig of 5000 k-mers = 14 ranking rounds, a cycle of 3000).  Tables come in through kq_import."""
import numpy as np
import pytest

from tests import gfa_cases as GC
from tests import gfa_ref as G
from tests import subgraph_ref as R

pytestmark = pytest.mark.gpu

MAPS = 128
ERR_INVALID, ERR_CAPACITY = -1, -6


@pytest.fixture(scope="module")
def kq():
    from kreeq_amd import capi
    assert capi.device_available()
    return capi


def load(kq, table, k):
    db = kq.KreeqDB(k, MAPS, capacity_hint=max(len(table), 1 << 12))
    if table:
        db.import_entries(R.entries_of(table))
    return db


def as_tuples(segs, edges):
    return ([(int(s["seq_off"]), int(s["head_key"]), int(s["n_kmers"]), int(s["cov"]), int(s["head_rc"])) for s in segs],
            [(int(e["from"]), int(e["to"]), int(e["count"]), int(e["from_rc"]), int(e["to_rc"])) for e in edges])


def check(kq, table, k):
    db = load(kq, table, k)
    try:
        for no_collapse in (False, True):
            want = G.build(table, k, no_collapse)
            segs, seq, edges, counts = db.subgraph_gfa(no_collapse)
            assert counts == want.counts
            got_segs, got_edges = as_tuples(segs, edges)
            assert seq.decode() == want.seq
            assert got_segs == want.segs
            assert got_edges == want.edges
            assert not segs["pad"].any() and not edges["pad"].any()
    finally:
        db.close()


@pytest.mark.parametrize("k", GC.INPUT_KS)
def test_inputs(kq, k):
    check(kq, GC.input_table(k), k)


@pytest.mark.parametrize("idx", (37, 38, 43))
def test_goldens(kq, idx):
    check(kq, GC.golden_table(idx)[0], 21)


@pytest.mark.parametrize("name,k", GC.HAND_IDS)
def test_hand_cases(kq, name, k):
    check(kq, GC.hand_case(name, k), k)


def rank_rounds(db):
    return sum(name.startswith("gfa_rank_") for name in db.profile())


def test_ranking_rounds(kq):
    """5000 k-mers in one chain: 13 doubling rounds and the one that finds nothing to do; a cycle runs the round limit
    (1 + ceil(log2(2n))) before it is opened, and is ranked again"""
    for name, rounds in (("long_unitig", 14), ("long_cycle", 14 + 13)):
        table = GC.hand_case(name, 21)
        db = load(kq, table, 21)
        try:
            db.set_option("profile", 1)
            db.subgraph_gfa_raw()
            assert rank_rounds(db) == rounds, name
        finally:
            db.close()


def test_capacity_protocol(kq):
    table = GC.input_table(21)
    want = G.build(table, 21)
    db = load(kq, table, 21)
    try:
        rc, counts, segs, seq, edges = db.subgraph_gfa_raw()
        assert rc == 0 and counts == want.counts and segs is None             # counts only
        exact = (counts["n_segments"], counts["n_seq"], counts["n_edges"])
        assert min(exact) > 0
        for short in range(3):
            caps = tuple(c - (i == short) for i, c in enumerate(exact))
            rc, counts, segs, seq, edges = db.subgraph_gfa_raw(caps=caps)
            assert rc == ERR_CAPACITY and counts == want.counts
            assert not segs.view(np.uint8).any() and not seq.any() and not edges.view(np.uint8).any()      # nothing written
        rc, counts, segs, seq, edges = db.subgraph_gfa_raw(caps=exact)
        assert rc == 0 and counts == want.counts
        assert as_tuples(segs[:exact[0]], edges[:exact[2]]) == (want.segs, want.edges) and seq[:exact[1]].tobytes().decode() == want.seq
        assert not segs[exact[0]:].view(np.uint8).any() and not seq[exact[1]:].any() and not edges[exact[2]:].view(np.uint8).any()      # nor behind the end
    finally:
        db.close()


def test_empty_table(kq):
    db = load(kq, {}, 21)
    try:
        for no_collapse in (False, True):
            rc, counts, *_ = db.subgraph_gfa_raw(no_collapse, caps=(4, 4, 4))
            assert rc == 0 and set(counts.values()) == {0}
    finally:
        db.close()


def test_refusals(kq):
    import ctypes as C

    lib = kq.load()
    db = load(kq, GC.hand_case("isolated", 5), 5)
    try:
        cnt = kq.GfaCounts()
        assert lib.kq_subgraph_gfa(None, 0, None, 0, None, 0, None, 0, C.byref(cnt)) == ERR_INVALID
        assert lib.kq_subgraph_gfa(db.handle, 0, None, 0, None, 0, None, 0, None) == ERR_INVALID
        rc, counts, *_ = db.subgraph_gfa_raw(flags=2)
        assert rc == ERR_INVALID and b"flags" in lib.kq_last_error()
        rc, counts, *_ = db.subgraph_gfa_raw(flags=3)
        assert rc == ERR_INVALID
        rc, counts, *_ = db.subgraph_gfa_raw()                               # still usable
        assert rc == 0 and counts["n_segments"] == 2
    finally:
        db.close()
    win = kq.KreeqDB(21, MAPS, capacity_hint=1 << 12)
    try:
        win.set_option("bucket_window", 0 | (128 << 16))
        rc, counts, *_ = win.subgraph_gfa_raw()
        assert rc == ERR_INVALID and b"windowed" in lib.kq_last_error()
    finally:
        win.close()
