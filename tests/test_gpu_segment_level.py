"""The last split level of a plan with a middle level has two forms: the unit path (k_lv_hist, offsets, scans, k_lv_scatter_s) and
k_lv_segment_s, where one workgroup counts, offsets and splits a whole sub-bucket segment.  KQ_OPT_KERNEL_SET bit 32 = always the unit
path, bit 64 = the segment kernel wherever it applies; with neither, a filtered pass takes the segment kernel when the slice's 256
bucket sizes are even (kq_seg_gate_host.h) and every other pass the unit path.  All of them must leave the oracle's table, exactly: the
whole summary with its histogram, and the entry of every distinct key.

Shapes (tables of 4-byte records, KQ_OPT_NARROW_MID picks the fan-out of the last level):
  2^16 regions, 256 per bucket, narrow_mid 16   ->   2 bins, 32768 segments, 64 counters per bin
  2^16 regions, 256 per bucket, narrow_mid 256  ->  32 bins,  2048 segments,  8 counters per bin
  2^18 regions, 1024 per bucket, narrow_mid 1024 -> 128 bins,  2048 segments,  2 counters per bin (the smallest table with 128 bins)
Inputs: small read batches (nearly all segments hold a handful of records or none); a few keys of chosen regions; records in the first
and in the last segment only; a segment of exactly one round (4096 records) and of one more; a batch large enough for even buckets
under a map range, with and without one k-mer repeated 10^5 times; two pending sets in one table pass."""
import math

import numpy as np
import pytest

from tests import helpers as H
from tests import region_inputs as R

pytestmark = pytest.mark.gpu

K, MAP = 21, 128
UNIT, SEGMENT = 32, 64                   # KQ_OPT_KERNEL_SET: the unit path everywhere / the segment kernel wherever it applies
ROUND = 4096                             # records per round of either scatter


def hint_for(regions):
    """smallest capacity hint of a table of `regions` regions (kq_create: slots = hint / 0.7, regions = slots / 2048 rounded up to a
    multiple of 256)"""
    return math.ceil(((regions - 256) * R.REGION_SLOTS + 1) * 0.7)


# name -> (regions, narrow_mid, bins of the last level, segments)
SHAPES = {"b2": (1 << 16, 16, 2, 32768), "b32": (1 << 16, 256, 32, 2048), "b128": (1 << 18, 1024, 128, 2048)}
ARENA = 256 << 20


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


def test_hint_rule():
    assert hint_for(1 << 16) == 93_585_409               # the hint test_gpu_region_offsets.py uses for 2^16 regions


def handle(kq, shape, mask, profile=False):
    regions, mid, bins, segs = SHAPES[shape]
    assert regions == bins * segs
    db = kq.KreeqDB(K, MAP, capacity_hint=hint_for(regions))
    assert db.info()["slots_total"] == regions * R.REGION_SLOTS
    db.set_option("count_path", "partitioned")
    db.set_option("trust_capacity", 1)                 # no read of the device state between batches: the sets stay pending
    db.set_option("pending_bytes", ARENA)
    db.set_option("narrow_mid", mid)
    db.set_option("kernel_set", mask)
    if profile:
        db.set_option("profile", 1)
    return db


def took_segment_kernel(db):
    """the stage list of the last count names the segment kernel's launch"""
    return "segment_level" in db.profile()


def reference(cpu, rng):
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


def same_part(db, want, lo, hi, tag):
    """the table of a map-range pass = the oracle's entries of the maps [lo, hi)"""
    maps = want["key"] % np.uint64(MAP)
    inside = (maps >= lo) & (maps < hi)
    part = want[inside]
    s = db.summary(with_hist=True)
    cov, cnt = np.unique(part["cov"], return_counts=True)
    assert s["distinct"] == len(part) and s["total"] == int(part["cov"].sum()), tag
    assert s["hist"] == dict(zip(cov.tolist(), cnt.tolist())), tag
    assert H.entries_equal(db.export(), part), tag
    perm = np.random.default_rng(lo).permutation(len(want))
    got = db.lookup_keys(want["key"][perm])[np.argsort(perm)]
    assert H.entries_equal(got[inside], part) and (got[~inside]["cov"] == 0).all(), tag


def run(kq, shape, batches, ref, masks=(UNIT, SEGMENT), passes=1):
    for mask in masks:
        db = handle(kq, shape, mask)
        for b in batches:
            db.count_batch(b)
        same_table(db, ref, (shape, mask))
        assert db.info()["table_passes"] == passes, (shape, mask)
        db.close()


def oracle_of(O, batches, seed):
    cpu = O.OracleDB(K, MAP)
    for b in batches:
        cpu.count_batch(b, threads=4)
    ref = reference(cpu, np.random.default_rng(seed))
    cpu.close()
    return ref


def small_batch(i):
    # the small read batches of test_gpu_region_offsets.py: one 30 kbp genome, reads of 60 .. 150 bp
    return H.synth_reads(90 + 3 * i, 60 + (7 * i) % 91, 30_000, seed=4242, err=0.01, n_rate=0.002)[0]


def bare_reads(keys):
    """one read of exactly k bases per key: one record each, no neighbouring k-mers"""
    rows = np.full((len(keys), K + 1), ord("\n"), dtype=np.uint8)
    rows[:, :K] = R.ACGT[R.key_codes(keys, K)]
    return rows.tobytes()[:-1]


@pytest.fixture(scope="module")
def small_refs(O):
    """the oracle after one and after two of the small batches, shared by the shapes"""
    cpu, refs, rng = O.OracleDB(K, MAP), {}, np.random.default_rng(1)
    for i in range(2):
        cpu.count_batch(small_batch(i), threads=4)
        refs[i + 1] = reference(cpu, rng)
    cpu.close()
    return refs


@pytest.mark.parametrize("n_sets", [1, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_small_batches(kq, small_refs, shape, n_sets):
    """~10^4 records over thousands of segments: most hold a few records, many none.  Two batches = two pending sets written by the
    same kernel, which meet in the offset matrix of one table pass"""
    run(kq, shape, [small_batch(i) for i in range(n_sets)], small_refs[n_sets])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_most_segments_empty(kq, O, shape):
    """five sets of a few short reads around two keys of four regions each: at most 40 x 11 k-mers, the flanks' included"""
    n, _, bins, segs = SHAPES[shape]
    rng = np.random.default_rng(n + 5)
    batches = []
    for _ in range(5):
        keys = np.concatenate([R.region_keys(int(r), n, K, 2, rng) for r in rng.integers(0, n, 4)])
        batches.append(R.keys_to_reads(keys, rng.integers(1, 6, len(keys)), K, rng))
    ref = oracle_of(O, batches, 2)
    assert len(np.unique(R.region_of_keys(ref["export"]["key"], K, n) // bins)) < segs // 4
    run(kq, shape, batches, ref)


@pytest.mark.parametrize("where", ["first", "last", "both"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_only_the_edge_segments(kq, O, shape, where):
    """records in the first segment only, in the last only (its closing offset is the set's record count), in both: every other
    segment is empty"""
    n, _, bins, segs = SHAPES[shape]
    rng = np.random.default_rng(segs + len(where))
    regs = {"first": range(bins), "last": range(n - bins, n), "both": list(range(bins)) + list(range(n - bins, n))}[where]
    regs = list(regs)[:: max(1, len(regs) // 8)] + [list(regs)[-1]]                  # a few regions of the segment(s), the last one included
    keys = np.unique(np.concatenate([R.region_keys(int(r), n, K, 5, rng) for r in regs]))
    batch = bare_reads(np.repeat(keys, rng.integers(1, 4, len(keys))))
    ref = oracle_of(O, [batch], 3)
    seg = np.unique(R.region_of_keys(ref["export"]["key"], K, n) // bins)
    assert set(seg.tolist()) == {"first": {0}, "last": {segs - 1}, "both": {0, segs - 1}}[where]
    run(kq, shape, [batch], ref)


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("shape", ["b2", "b32"])
def test_segment_of_one_round(kq, O, shape, extra):
    """a segment of exactly 4096 records (one full round, nothing behind it) and of 4097 (a round of one record), its neighbours
    empty, a few records elsewhere"""
    n, _, bins, segs = SHAPES[shape]
    rng = np.random.default_rng(bins + extra)
    seg = segs // 3
    keys = np.unique(np.concatenate([R.region_keys(seg * bins + r, n, K, 512 // bins, rng) for r in range(bins)]))
    assert len(keys) == 512
    copies = np.full(512, ROUND // 512)
    copies[17] += extra
    other = np.concatenate([R.region_keys(int(r), n, K, 2, rng) for r in (5, n // 2, n - 7)])
    batch = bare_reads(rng.permutation(np.concatenate([np.repeat(keys, copies), other])))
    ref = oracle_of(O, [batch], 4)
    regions = R.region_of_keys(ref["export"]["key"], K, n)
    assert int(ref["export"]["cov"][regions // bins == seg].sum()) == ROUND + extra
    run(kq, shape, [batch], ref)


# ---- batches large enough for the gate: under a map range of half the maps ~1.7 M records, ~6800 per bucket (sigma ~1.3 %)
BIG = dict(n_reads=27_000, read_len=150, genome_len=12_000_000, seed=99, err=0.01)
HOT_COPIES = 770                          # reads of 150 A: 130 k-mers each, 100 100 instances of one k-mer (key 0, map 0)


@pytest.fixture(scope="module")
def big(O):
    """one large batch, and the same with a hot k-mer: the oracle's entries of both, counted in one go"""
    reads = H.synth_reads(**BIG)[0]
    hot = b"\n".join([b"A" * 150] * HOT_COPIES)
    cpu = O.OracleDB(K, MAP)
    cpu.count_batch(reads, threads=4)
    plain = reference(cpu, np.random.default_rng(5))
    cpu.count_batch(hot, threads=4)
    with_hot = cpu.export()
    cpu.close()
    assert int(with_hot["cov"].max()) >= HOT_COPIES * 130
    return {"reads": reads, "plain": plain, "hot_batch": reads + b"\n" + hot, "hot": with_hot}


@pytest.mark.parametrize("shape", ["b2", "b32"])
def test_map_range_takes_the_segment_kernel(kq, big, shape):
    """a map-range pass reads the bucket offsets back: even buckets take the segment kernel by default, bit 32 keeps the unit path"""
    for mask, segment in ((0, True), (UNIT, False), (SEGMENT, True)):
        db = handle(kq, shape, mask, profile=True)
        db.set_option("count_map_range", (32, 96))
        db.count_batch(big["reads"])
        assert took_segment_kernel(db) == segment, (shape, mask)
        same_part(db, big["plain"]["export"], 32, 96, (shape, mask))
        db.close()


@pytest.mark.parametrize("shape", ["b2", "b32"])
def test_full_range(kq, big, shape):
    """without a map range nothing is read back: the unit path by default, the segment kernel with bit 64"""
    for mask, segment in ((0, False), (SEGMENT, True)):
        db = handle(kq, shape, mask, profile=True)
        db.count_batch(big["reads"])
        assert took_segment_kernel(db) == segment, (shape, mask)
        same_table(db, big["plain"], (shape, mask))
        db.close()


@pytest.mark.parametrize("shape", ["b2", "b32"])
def test_hot_sub_bucket(kq, big, shape):
    """one k-mer 10^5 times among ordinary reads: its bucket stands far above the mean, so the default keeps the unit path (which cuts
    the hot segment into units); bit 64 gives the whole segment to one workgroup.  Same table either way"""
    for mask, segment in ((0, False), (UNIT, False), (SEGMENT, True)):
        db = handle(kq, shape, mask, profile=True)
        db.set_option("count_map_range", (0, 64))
        db.count_batch(big["hot_batch"])
        assert took_segment_kernel(db) == segment, (shape, mask)
        same_part(db, big["hot"], 0, 64, (shape, mask))
        db.close()
