"""kq_export as a unit: the filter (k_export), the key order (sort_entries_dev: k_entry_keys, the radix sort over bits [0, 2k),
k_entry_gather -- or parallel_sort_entries on the host) and the way out (copy_out_bounced), against tables that came in through
kq_import and whose content is known: tests/export_cases.py constructs every entry from its key, and the reference of an export
is that numpy array, filtered by key % map_count and sorted by key.  No count path and no other device result is involved.

Every case runs in the modes of KQ_OPT_TEST_EXPORT its list names: device or host sort x one copy or 4096-byte chunks.  The sizes
sit on both sides of what selects another code path: 1024 and 1 048 576 entries (the sorting library's one-workgroup sort, its
merge sort, its multi-pass onesweep), k with 2k on both sides of every multiple of 8 (digit passes 1 to 8, both parities),
1 398 101 / 1 398 102 entries (one copy / bounce buffers, a last chunk of 32 bytes), 1 048 576 and 2 097 152 entries (whole
chunks), the whole key space of k = 11.  Then the capacity protocol with guard bytes, map ranges on 1, 3 and 128 maps, growth and
merge, and the two other callers of the sort above its small-input sizes (kq_export_map_images, kq_subgraph_gfa)."""
import ctypes as C

import numpy as np
import pytest

from tests import export_cases as EC
from tests import helpers as H

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_NOMEM, ERR_CAPACITY = 0, -1, -4, -6
FILL = 0x5A


@pytest.fixture(scope="module")
def kq():
    from kreeq_amd import capi
    assert capi.device_available()
    return capi


def table(kq, k, e, map_count=128, capacity_hint=None):
    db = kq.KreeqDB(k, map_count, capacity_hint=max(len(e), 1 << 12) if capacity_hint is None else capacity_hint)
    if len(e):
        db.import_entries(e)
    return db


def raw_export(kq, db, lo, hi, cap, null_out=False):
    """kq_export into a buffer of `cap` entries filled with 0x5A -> (return code, n_out, the buffer)"""
    out = np.empty(cap, dtype=EC.ENTRY_DTYPE)
    out.view(np.uint8)[:] = FILL
    n = C.c_uint64(0xDEAD)
    rc = kq.load().kq_export(db.handle, lo, hi, None if null_out else out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return rc, n.value, out


def untouched(a):
    return bool((a.view(np.uint8) == FILL).all())


def assert_export(kq, db, want, what, lo=0, hi=None):
    hi = db.map_count if hi is None else hi
    got = db.export(lo, hi)
    diff = EC.first_difference(got, want)
    assert diff is None, f"{what}: {diff}"


# ---- sizes and k: sort algorithm, pass count, copy path -----------------------------------------------------------------
@pytest.mark.parametrize("case", EC.cases(), ids=EC.case_id)
def test_sizes_and_k(kq, case):
    k, n, modes = case
    e = EC.entries(k, n)
    want = EC.expected(e)
    db = table(kq, k, e)
    try:
        assert db.info()["slots_used"] == n
        for mode in modes:
            db.set_option("test_export", EC.MODES[mode])
            assert_export(kq, db, want, f"k {k}, n {n}, {mode} ({EC.sort_algorithm(n)} sort, {EC.sort_passes(k)} passes, {EC.copy_plan(n, mode)[0]} copy)")
    finally:
        db.close()


def test_option_range(kq):
    db = table(kq, 21, EC.entries(21, 64))
    try:
        for bad in (-1, 4, 1 << 20):
            with pytest.raises(kq.KqError) as err:
                db.set_option("test_export", bad)
            assert err.value.code == ERR_INVALID
        for v in (3, 0):
            db.set_option("test_export", v)
    finally:
        db.close()


def test_tier_boundary_and_clamp(kq):
    e = EC.saturated_entries()
    db = table(kq, 21, e)
    try:
        for mode in EC.ALL_MODES:
            db.set_option("test_export", EC.MODES[mode])
            assert_export(kq, db, EC.expected(e), mode)
        db.set_option("test_export", 0)
        db.import_entries(e)                                # 254 + 254 crosses the tier; 2^32 - 1 stays
        assert_export(kq, db, EC.expected(EC.doubled(e)), "imported twice")
    finally:
        db.close()


# ---- capacity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", EC.ALL_MODES)
@pytest.mark.parametrize("n", [2, 257, 1025, 5000])
def test_capacity(kq, n, mode):
    e = EC.entries(21, n)
    want = EC.expected(e)
    db = table(kq, 21, e)
    try:
        db.set_option("test_export", EC.MODES[mode])
        rc, n_out, _ = raw_export(kq, db, 0, 128, 0, null_out=True)             # the size query
        assert (rc, n_out) == (OK, n)
        rc, n_out, out = raw_export(kq, db, 0, 128, n)
        assert (rc, n_out) == (OK, n) and EC.first_difference(out, want) is None
        rc, n_out, out = raw_export(kq, db, 0, 128, n + 7)                      # room to spare: the entries behind the end keep their fill
        assert (rc, n_out) == (OK, n) and EC.first_difference(out[:n], want) is None
        assert untouched(out[n:])
        for cap in sorted({n - 1, 1}):                                          # too small: the size, and nothing written
            rc, n_out, out = raw_export(kq, db, 0, 128, cap)
            assert (rc, n_out) == (ERR_CAPACITY, n), cap
            assert untouched(out), cap
            assert b"too small" in kq.load().kq_last_error()
            rc, n_out, _ = raw_export(kq, db, 0, 128, 0, null_out=True)         # the failed call changed nothing
            assert (rc, n_out) == (OK, n)
        rc, n_out, out = raw_export(kq, db, 0, 128, n)
        assert (rc, n_out) == (OK, n) and EC.first_difference(out, want) is None
        # a range of its own: cap against the range's count, not the table's
        m = e["key"] % np.uint64(128)
        n_r = int(((m >= 5) & (m < 60)).sum())
        rc, n_out, out = raw_export(kq, db, 5, 60, n_r + 7)
        assert (rc, n_out) == (OK, n_r) and EC.first_difference(out[:n_r], EC.expected(e, 128, 5, 60)) is None and untouched(out[n_r:])
        if n_r > 1:
            rc, n_out, out = raw_export(kq, db, 5, 60, n_r - 1)
            assert (rc, n_out) == (ERR_CAPACITY, n_r) and untouched(out)
    finally:
        db.close()


def test_null_arguments(kq):
    db = table(kq, 21, EC.entries(21, 64))
    try:
        L = kq.load()
        n = C.c_uint64(0)
        assert L.kq_export(None, 0, 128, None, 0, C.byref(n)) == ERR_INVALID
        assert L.kq_export(db.handle, 0, 128, None, 0, None) == ERR_INVALID
        rc, n_out, _ = raw_export(kq, db, 0, 128, 0)                            # a buffer of no entries is a size query as well
        assert (rc, n_out) == (ERR_CAPACITY, 64)
        rc, n_out, _ = raw_export(kq, db, 0, 128, 64, null_out=True)            # no buffer: cap is not looked at
        assert (rc, n_out) == (OK, 64)
    finally:
        db.close()


# ---- map ranges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "host_sort_bounced"])
@pytest.mark.parametrize("map_count", [1, 3, 128])
def test_map_ranges(kq, map_count, mode):
    k, n = 21, 20_000
    e = EC.entries(k, n)
    db = table(kq, k, e, map_count)                         # (3: kq_create takes any map count from 1 to 65535)
    try:
        db.set_option("test_export", EC.MODES[mode])
        rng = np.random.default_rng(map_count)
        partitions = [[0, map_count]] + [[0, c, map_count] for c in range(1, map_count)][:3]
        for _ in range(4):
            inner = np.sort(rng.choice(np.arange(0, map_count + 1), min(map_count + 1, int(rng.integers(1, 6))), replace=False)).tolist()
            partitions.append([0] + inner + [map_count])    # (a cut at 0 or map_count, or none: empty ranges among them)
        for cuts in partitions:
            total = 0
            for lo, hi in zip(cuts, cuts[1:]):
                want = EC.expected(e, map_count, lo, hi)
                assert_export(kq, db, want, f"maps [{lo}, {hi}) of {map_count}, {mode}", lo, hi)
                total += len(want)
            assert total == n
        for at in sorted({0, map_count // 2, map_count}):   # empty ranges
            rc, n_out, out = raw_export(kq, db, at, at, 4)
            assert (rc, n_out) == (OK, 0) and untouched(out), at
            rc, n_out, _ = raw_export(kq, db, at, at, 0, null_out=True)
            assert (rc, n_out) == (OK, 0)
        for lo, hi in ((0, map_count + 1), (map_count, map_count + 1), (map_count + 1, map_count + 1), (1, 0), (map_count, map_count - 1)):
            rc, n_out, out = raw_export(kq, db, lo, hi, 4)
            assert rc == ERR_INVALID and untouched(out), (lo, hi)
        assert_export(kq, db, EC.expected(e, map_count), "whole table after the refusals")
    finally:
        db.close()


def test_single_maps_of_128(kq):
    """every map on its own: each entry comes out exactly once, under its own map"""
    e = EC.entries(21, 5000)
    db = table(kq, 21, e)
    try:
        parts = [db.export(m, m + 1) for m in range(128)]
        for m, p in enumerate(parts):
            assert EC.first_difference(p, EC.expected(e, 128, m, m + 1)) is None, m
        assert sum(len(p) for p in parts) == len(e)
    finally:
        db.close()


# ---- growth and merge ---------------------------------------------------------------------------------------------------
def test_growth_between_imports(kq):
    """capacity_hint 0: the table (732 regions) takes the first two parts as it is and grows for the third; the side table of
    high-copy entries grows on the way.  The export after each part is the union so far"""
    k, part = 21, 450_000
    e = EC.entries(k, 3 * part)
    db = table(kq, k, e[:0], capacity_hint=0)
    try:
        slots = [db.info()["slots_total"]]
        for i in range(3):
            db.import_entries(e[i * part:(i + 1) * part])
            assert_export(kq, db, EC.expected(e[:(i + 1) * part]), f"after part {i + 1}")
            slots.append(db.info()["slots_total"])
        assert slots[0] == slots[2] < slots[3] and db.info()["slots_used"] == 3 * part
    finally:
        db.close()


@pytest.mark.parametrize("mode", ["default", "host_sort_bounced"])
def test_import_twice_doubles(kq, mode):
    e = EC.entries(21, 3000)
    db = table(kq, 21, e)
    try:
        db.set_option("test_export", EC.MODES[mode])
        db.import_entries(e[::-1])
        assert_export(kq, db, EC.expected(EC.doubled(e)), "imported twice")
        assert db.info()["slots_used"] == len(e)
    finally:
        db.close()


# ---- the other callers of the sort --------------------------------------------------------------------------------------
def test_map_images_above_the_small_sorts(kq, tmp_path):
    """kq_export_map_images over 300 000 entries (merge sort), high-copy ones among them: every image is the host writer's file.
    Without the device sort the call has nothing to fall back on: KQ_ERR_NOMEM, and the handle stays usable"""
    k, n = 21, 300_000
    e = EC.expected(EC.entries(k, n))
    assert (e["hc"] != 0).sum() > 1000
    db = table(kq, k, e)
    try:
        for lo, hi, mode in ((0, 128, "default"), (0, 128, "bounced"), (17, 90, "default")):
            db.set_option("test_export", EC.MODES[mode])
            want, want_hc = H.host_map_files(tmp_path, e, 128, lo, hi)
            offsets, n_hc = db.export_map_images(lo, hi, sizes_only=True)
            got, hc = db.export_map_images(lo, hi)
            assert [len(g) for g in got] == np.diff(offsets.astype(np.int64)).tolist() == [len(w) for w in want]
            for m, (g, w) in enumerate(zip(got, want), lo):
                assert g.tobytes() == w, f"map {m}, {mode}"
            assert n_hc == len(hc) == len(want_hc)
            assert EC.first_difference(hc, want_hc[np.argsort(want_hc["key"], kind="stable")]) is None
            in_range = EC.expected(e, 128, lo, hi)
            assert EC.first_difference(hc, in_range[in_range["hc"] != 0]) is None
        db.set_option("test_export", 1)
        with pytest.raises(kq.KqError) as err:
            db.export_map_images(0, 128)
        assert err.value.code == ERR_NOMEM and "sort" in str(err.value)
        offsets2, n_hc2 = db.export_map_images(17, 90, sizes_only=True)       # the size query does not sort
        assert np.array_equal(offsets2, offsets) and n_hc2 == n_hc
        db.set_option("test_export", 0)
        assert_export(kq, db, e, "after the refused call")
    finally:
        db.close()


@pytest.fixture(scope="module")
def gfa_table():
    """a table of more than 100 000 k-mers as a count gives it: one random sequence, and 40 windows of it with one base changed
    (bubbles: branching k-mers at both ends)"""
    from tests import gfa_cases as GC

    k = 15
    rng = np.random.default_rng(1500)
    genome = "".join("ACGT"[i] for i in rng.integers(0, 4, 101_000))
    seqs = [genome]
    for start in rng.integers(0, len(genome) - 200, 40).tolist():
        w = list(genome[start:start + 200])
        w[100] = "ACGT"[("ACGT".index(w[100]) + 1 + int(rng.integers(0, 3))) % 4]
        seqs.append("".join(w))
    return k, GC.count_table(k, seqs)


def test_gfa_above_the_small_sorts(kq, gfa_table):
    """kq_subgraph_gfa where its sort sees more than 100 000 entries: equal to tests/gfa_ref.py, record by record; the copies out
    through 4096-byte chunks as well.  Without the device sort: KQ_ERR_NOMEM, counts zero, and the handle stays usable"""
    from tests import gfa_ref as G
    from tests import subgraph_ref as R

    k, tab = gfa_table
    assert len(tab) >= 100_000
    want = G.build(tab, k)
    assert want.counts["n_segments"] > 40 and want.counts["n_edges"] > 40
    db = table(kq, k, R.entries_of(tab))
    try:
        for mode in ("default", "bounced"):
            db.set_option("test_export", EC.MODES[mode])
            segs, seq, edges, counts = db.subgraph_gfa()
            assert counts == want.counts, mode
            assert seq.decode() == want.seq, mode
            assert [(int(s["seq_off"]), int(s["head_key"]), int(s["n_kmers"]), int(s["cov"]), int(s["head_rc"])) for s in segs] == want.segs, mode
            assert [(int(x["from"]), int(x["to"]), int(x["count"]), int(x["from_rc"]), int(x["to_rc"])) for x in edges] == want.edges, mode
        db.set_option("test_export", 1)
        rc, counts, *_ = db.subgraph_gfa_raw()
        assert rc == ERR_NOMEM and set(counts.values()) == {0} and b"no device memory" in kq.load().kq_last_error()
        db.set_option("test_export", 0)
        rc, counts, *_ = db.subgraph_gfa_raw()
        assert rc == OK and counts == want.counts
    finally:
        db.close()
