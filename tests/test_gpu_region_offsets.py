"""The table pass of 4- and 5-byte records (k_count_regions_q4r) reads a region's share of every pending set from one
region-major offset matrix, transposed once per pass (k_p3_region_offsets).  KQ_OPT_KERNEL_SET bit 16 selects the pass that
reads the sets' own offset arrays instead.  Both must leave the oracle's table, exactly: the whole summary with its
histogram, and the entry of every distinct key.

Shapes: the smallest table of 5-byte records (2048 regions) and the smallest table of 4-byte records (2^16 regions); set
counts at the edges of the matrix pitch (a multiple of 16, at most 64); a pass that reuses the matrix with fewer sets;
sets that leave most regions -- and the first / last region in all sets but one -- without records; a skewed region; a
lazily cleared table; two map ranges."""
import numpy as np
import pytest

from tests import helpers as H
from tests import region_inputs as R

pytestmark = pytest.mark.gpu

K, MAP = 21, 128
MASKS = (0, 16)                          # 0: row pairs of the offset matrix (shipped); 16: the sets' own offset arrays
# capacity hints: slots = hint / 0.7, regions = slots / 2048 rounded up to a multiple of 256
FORMATS = {"narrow": (2_935_000, 2048),              # the smallest table that takes 5-byte records
           "tight": (93_585_409, 1 << 16)}           # the smallest hint that reaches TIGHT_MIN_REGIONS: 4-byte records
ARENA = 160 << 20                        # holds 65 sets of either table (a set: <= 5 B per record + 8 B per region)
SET_COUNTS = (1, 2, 16, 17, 63, 64, 65)  # 65: the 65th set triggers a pass over 64, the closing pass takes 1 (pitch 64 -> 16)


@pytest.fixture(scope="module")
def kq():
    import kreeq_amd
    if not kreeq_amd.device_available():
        pytest.fail("no gfx950 device: the product has no CPU fallback")
    return kreeq_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    O.build()
    return O


def handle(kq, fmt, pending=ARENA, **opts):
    hint, regions = FORMATS[fmt]
    db = kq.KreeqDB(K, MAP, capacity_hint=hint)
    assert db.info()["slots_total"] == regions * R.REGION_SLOTS
    db.set_option("count_path", "partitioned")
    db.set_option("trust_capacity", 1)                 # no read of the device state between batches: the sets stay pending
    db.set_option("pending_bytes", pending)
    for o, v in opts.items():
        db.set_option(o, v)
    return db


def reference(cpu, rng):
    """what a table must answer: the oracle's summary, its entries, and some keys it does not hold"""
    want = cpu.export()
    absent = rng.integers(0, 1 << (2 * K), 300, dtype=np.uint64)
    return {"summary": cpu.summary(with_hist=True), "export": want, "absent": absent[~np.isin(absent, want["key"])]}


def same_table(db, ref, tag):
    assert db.summary(with_hist=True) == ref["summary"], tag
    want = ref["export"]
    keys = np.concatenate([want["key"], ref["absent"]])
    perm = np.random.default_rng(len(keys)).permutation(len(keys))
    got = db.lookup_keys(keys[perm])[np.argsort(perm)]
    assert H.entries_equal(got[:len(want)], want), tag
    assert (got[len(want):]["cov"] == 0).all(), tag


def small_batch(i):
    # the same 30 kbp genome for every batch (the first draw of the seed), reads of 60 .. 150 bp
    return H.synth_reads(90 + 3 * i, 60 + (7 * i) % 91, 30_000, seed=4242, err=0.01, n_rate=0.002)[0]


@pytest.fixture(scope="module")
def counted_sets(O):
    """the oracle after 1, 2, 16, ... of the small batches: computed once, shared by both formats"""
    cpu, refs, rng = O.OracleDB(K, MAP), {}, np.random.default_rng(1)
    for i in range(max(SET_COUNTS)):
        cpu.count_batch(small_batch(i), threads=4)
        if i + 1 in SET_COUNTS:
            refs[i + 1] = reference(cpu, rng)
    cpu.close()
    return refs


@pytest.mark.parametrize("n_sets", SET_COUNTS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_set_counts_at_the_pitch_edges(kq, counted_sets, fmt, n_sets):
    """n_sets batches = n_sets pending sets, applied by one pass (pitch 16, 32 or 64 with 0, 1 or 15 unused columns); with 65
    the matrix of the first pass (64 columns in use) is rewritten for a second pass with one set and pitch 16"""
    for mask in MASKS:
        db = handle(kq, fmt, kernel_set=mask)
        for i in range(n_sets):
            db.count_batch(small_batch(i))
        same_table(db, counted_sets[n_sets], (fmt, n_sets, mask))
        assert db.info()["table_passes"] == (2 if n_sets > 64 else 1), mask      # all sets in one pass; 65 = 64 + 1
        db.close()


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_edge_regions_filled_by_one_set_only(kq, O, fmt, where):
    """five sets of a few short reads each: nearly every region is empty in every set, and region 0 and the last region
    (whose closing offset is the last row of the matrix) get records from the first / the last set alone"""
    n = FORMATS[fmt][1]
    rng = np.random.default_rng(n + len(where))
    edge = (0, n - 1)
    batches = []
    for i in range(5):
        special = i == (0 if where == "first" else 4)
        regs = edge if special else rng.integers(1, n - 1, 6)
        keys = np.concatenate([R.region_keys(int(r), n, K, 3, rng) for r in regs])
        batches.append(R.keys_to_reads(keys, rng.integers(1, 6, len(keys)), K, rng, n, avoid=edge))
        hit = np.isin(edge, R.region_of_keys(O.emit_records(K, batches[-1])[0], K, n))
        assert hit.all() if special else not hit.any()
    cpu = O.OracleDB(K, MAP)
    for b in batches:
        cpu.count_batch(b)
    ref = reference(cpu, rng)
    cpu.close()
    assert len(np.unique(R.region_of_keys(ref["export"]["key"], K, n))) < n // 4      # most regions hold nothing
    for mask in MASKS:
        db = handle(kq, fmt, kernel_set=mask)
        for b in batches:
            db.count_batch(b)
        same_table(db, ref, (fmt, where, mask))
        assert db.info()["table_passes"] == 1
        db.close()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_hot_region_behind_the_gate(kq, O, fmt):
    """poly-A reads: one k-mer with 4 x 600 x 130 instances, far beyond 32 x 2048 records in its region -- the region goes to the
    hot list and the folding launch, the k-mer to the high-copy tier -- between ordinary sets"""
    hot = b"\n".join([b"A" * 150] * 600)
    batches = [small_batch(0), hot, small_batch(1), hot, hot, small_batch(2), hot]
    cpu = O.OracleDB(K, MAP)
    for b in batches:
        cpu.count_batch(b, threads=4)
    ref = reference(cpu, np.random.default_rng(2))
    cpu.close()
    assert ref["export"]["cov"].max() == 4 * 600 * 130 > 32 * R.REGION_SLOTS
    for mask in MASKS:
        db = handle(kq, fmt, kernel_set=mask)
        for b in batches:
            db.count_batch(b)
        same_table(db, ref, (fmt, mask))
        assert db.info()["table_passes"] == 1
        db.close()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_lazily_cleared_table(kq, O, fmt):
    """after kq_clear the slot array still holds the first job: the next pass writes every region's image, also of the many
    regions its sets have no records for"""
    first = [small_batch(i) for i in range(3)]
    after = [H.synth_reads(4, 70 + 9 * i, 2_000, seed=77)[0] for i in range(3)]          # ~600 k-mers: most regions stay empty
    cpu = O.OracleDB(K, MAP)
    for b in after:
        cpu.count_batch(b)
    ref = reference(cpu, np.random.default_rng(3))
    cpu.close()
    for mask in MASKS:
        db = handle(kq, fmt, kernel_set=mask)
        for b in first:
            db.count_batch(b)
        db.sync()
        db.clear()
        for b in after:
            db.count_batch(b)
        same_table(db, ref, (fmt, mask))
        db.close()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_map_ranges(kq, O, fmt):
    """two map ranges over one small job, the way the flagship run calls the pass: each range's table = the oracle's entries
    of those maps"""
    batches = [small_batch(i) for i in range(4)]
    cpu = O.OracleDB(K, MAP)
    for b in batches:
        cpu.count_batch(b, threads=4)
    want = cpu.export()
    cpu.close()
    maps = want["key"] % np.uint64(MAP)
    for mask in MASKS:
        db = handle(kq, fmt, kernel_set=mask)
        for lo, hi in ((64, 128), (0, 64)):
            db.clear()
            db.set_option("count_map_range", (lo, hi))
            for b in batches:
                db.count_batch(b)
            part = want[(maps >= lo) & (maps < hi)]
            s = db.summary(with_hist=True)
            cov, cnt = np.unique(part["cov"], return_counts=True)
            assert s["distinct"] == len(part) and s["total"] == int(part["cov"].sum()), (fmt, mask, lo)
            assert s["hist"] == dict(zip(cov.tolist(), cnt.tolist())), (fmt, mask, lo)
            assert H.entries_equal(db.export(), part), (fmt, mask, lo)
            perm = np.random.default_rng(lo).permutation(len(want))
            got = db.lookup_keys(want["key"][perm])[np.argsort(perm)]
            inside = (maps >= lo) & (maps < hi)
            assert H.entries_equal(got[inside], part) and (got[~inside]["cov"] == 0).all(), (fmt, mask, lo)
        db.close()
