"""Full table regions and a crowded high-copy tier, exact against the CPU oracle.

A table region holds 2048 keys, probed linearly from a home quad and wrapping from slot 2047 to 0; the region kernels
queue records that miss their home quad, sum the edges of the first 64 k-mers per region and pass that move past 254
instances in LDS (the rest go to the side table directly), hand regions with more than 32 x 2048 records of a pass to the
folding kernel, and the side table is rehashed as it grows.  Uniform inputs reach none of these limits.  Here keys are
made for chosen regions through the numpy restatement of the table geometry (tests/region_inputs.py), which is pinned to
the device first: the hash bits of packed records, and a region that takes exactly 2048 keys but not a 2049th.  Each
case asserts the occupancy it was designed for (the oracle's k-mer walk of its reads, regions by the restatement), the
table class, and that the table did not grow, before it compares export and summary with the oracle.
Table classes as in test_gpu_kmatrix.py: S (hint 0, < 2048 regions), B (hint 5 M), T (hint 100 M, >= 2^16 regions)."""
import functools
import types

import numpy as np
import pytest

from tests import helpers as H
from tests import region_inputs as R

pytestmark = pytest.mark.gpu

MAP = 128
HINT = {"S": 0, "B": 5_000_000, "T": 100_000_000}
FULL = R.REGION_SLOTS
LOW = 254                          # instances the 8-bit tier holds
BIG = 32 * FULL                    # records of one region and pass above which the folding kernel takes the region


@pytest.fixture(scope="module")
def kq():
    import kreeq_amd

    if not kreeq_amd.device_available():
        pytest.fail("no gfx950 device: the product path has no CPU fallback")
    return kreeq_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def n_regions_of(k, cls):
    """region count kq_create gives the class (kq_plan_host.h initial_regions / round_regions: load 0.7 at the hint, whole
    multiples of 256 regions from 2048 on and for k >= 29); asserted against info() on every handle"""
    r = max(16, -(-int((HINT[cls] or 1 << 20) / 0.7) // FULL))
    return -(-r // 256) * 256 if r >= 2048 or k >= 29 else r


def handle(kq, k, cls, trust=True, **opts):
    db = kq.KreeqDB(k, MAP, capacity_hint=HINT[cls])
    assert db.info()["slots_total"] == n_regions_of(k, cls) * FULL
    if trust:
        db.set_option("trust_capacity", 1)
    for o, v in opts.items():
        db.set_option(o, v)
    return db


def unchanged(db, k, cls):
    assert db.info()["slots_total"] == n_regions_of(k, cls) * FULL, "the table grew"


def same_table(db, ref, what=""):
    assert H.entries_equal(db.export(), ref.export), what
    assert db.summary(with_hist=True) == ref.summary, what


def oracle_of(O, k, batches):
    cpu = O.OracleDB(k, MAP)
    for b in batches:
        cpu.count_batch(b, threads=8)
    r = types.SimpleNamespace(export=cpu.export(), summary=cpu.summary(with_hist=True), cpu=cpu)
    return r


def bare_reads(keys, k):
    """each key alone in a read: exactly its own k-mer"""
    return b"\n".join(R.ACGT[R.key_codes(keys, k)].view(f"S{k}").ravel().tolist()) if len(keys) else b""


def roomy_regions(k, n, count, need, rng):
    """`count` distinct regions that hold at least `need` canonical keys, none adjacent to another (a neighbour region
    stays free for the boundary cases), or [] when the key space leaves every region smaller"""
    lo, hi = R.value_range(0, n, k)
    small = hi - lo <= R.ENUM_MAX // 4                     # small key space: measure the regions
    out = []
    for r in rng.permutation(n)[:400].tolist():
        if r + 1 < n and all(abs(r - q) > 1 for q in out) and (not small or len(R.all_region_keys(r, n, k)) >= need):
            out.append(r)
        if len(out) == count:
            break
    return out if len(out) == count else []


def skip_unless_room(k, n, regions):
    if not regions:
        per = H.n_canonical(k) / n
        assert per < FULL, "regions were not found although the key space allows them"
        pytest.skip(f"k = {k}: {n} regions hold ~{per:.0f} canonical keys each, fewer than {FULL}")


# ---------------------------------------------------------------------------------- pin the restatement to the device
@pytest.mark.parametrize("k", [10, 12, 17, 21, 24, 25, 28])
def test_packed_records_carry_the_restated_hash(kq, O, k):
    """the 56 hash bits of kq_emit_packed_dev records == the restated table hash of the oracle's keys, as multisets"""
    import torch

    batch, _ = H.synth_reads(3000, 150, 40000, seed=900 + k, err=0.01, n_rate=0.002)
    ok, _ = O.emit_records(k, batch)
    t = torch.frombuffer(bytearray(batch), dtype=torch.uint8).cuda()
    recs = torch.empty(len(batch), dtype=torch.int64, device="cuda")
    db = kq.KreeqDB(k, MAP)
    counts = db.emit_packed_dev(t.data_ptr(), len(batch), 1, recs.data_ptr(), len(batch))
    assert int(counts.sum()) == len(ok)
    got = recs[:len(ok)].cpu().numpy().astype(np.uint64) & np.uint64((1 << 56) - 1)
    want = R.table_hash(ok, k) >> np.uint64(8)
    assert np.array_equal(np.sort(got), np.sort(want))
    db.close()


BOUNDARY = [(12, "S"), (12, "B"), (17, "B"), (17, "T"), (21, "B"), (21, "T"), (24, "S"), (25, "B"), (28, "S"), (29, "B"),
            (32, "S"), (32, "B"), (10, "B")]


@pytest.mark.parametrize("path", ["direct", "partitioned"])
@pytest.mark.parametrize("k,cls", BOUNDARY, ids=[f"k{k}-{c}" for k, c in BOUNDARY])
def test_region_boundary(kq, O, k, cls, path):
    """2048 keys aimed at one region count exactly on a trusted table that does not grow; a 2049th key aimed at it fails
    the next synchronising call with KQ_ERR_TABLE_FULL (test_gpu_parity.py test_trusted_capacity_overflow_fails_loudly);
    the same key aimed at the neighbouring region instead does not"""
    n = n_regions_of(k, cls)
    rng = np.random.default_rng(1000 + k)
    regs = roomy_regions(k, n, 1, FULL + 1, rng)
    skip_unless_room(k, n, regs)
    r = regs[0]
    keys = R.region_keys(r, n, k, FULL + 1, rng)
    assert len(keys) == FULL + 1 and (R.region_of_keys(keys, k, n) == r).all()
    extra, keys = keys[:1], keys[1:]
    nb = R.region_keys(r + 1, n, k, 1, rng)
    assert len(nb) == 1 and R.region_of_keys(nb, k, n)[0] == r + 1
    db = handle(kq, k, cls, count_path=path)
    db.count_batch(bare_reads(keys, k))
    e = db.export()
    assert np.array_equal(e["key"], keys) and (e["cov"] == 1).all()
    assert db.info()["slots_used"] == FULL
    db.count_batch(bare_reads(nb, k))
    e = db.export()
    assert len(e) == FULL + 1 and nb[0] in e["key"]
    unchanged(db, k, cls)
    db.close()
    db = handle(kq, k, cls, count_path=path)
    with pytest.raises(kq.KqError) as err:
        db.count_batch(bare_reads(np.concatenate([keys, extra]), k))
        db.summary()
    assert err.value.code == -5
    db.close()


# ---------------------------------------------------------------------------------- 1.-2. exactly full regions
FULL_CASES = [(10, "B"), (12, "B"), (12, "S"), (17, "B"), (17, "T"), (21, "B"), (21, "T"), (24, "S"), (25, "B"), (28, "S"),
              (29, "B"), (32, "S"), (32, "B")]
LAYOUTS = ("quad", "wrap", "random")
HC_PER_REGION = 40                 # keys per region of each high-copy kind


@functools.lru_cache(maxsize=None)
def full_reference(k, cls):
    from oracle import oracle as O

    n = n_regions_of(k, cls)
    rng = np.random.default_rng(2000 + k)
    regs = roomy_regions(k, n, len(LAYOUTS), FULL + 300, rng)
    if not regs:
        return types.SimpleNamespace(regions=[], n=n)
    keys, shared = [], []
    for r, lay in zip(regs, LAYOUTS):
        kk, same = R.full_region_keys(r, n, k, rng, lay)
        assert len(kk) == FULL
        keys.append(kk)
        shared.append(same)
    # instances: 1 (in one of the batches), already past 254 from batch 1, crossing 254 in batch 2 (from batch 1's 100),
    # crossing 254 inside batch 2
    c1, c2 = [], []
    for kk in keys:
        kind = rng.permutation(np.arange(FULL) % (FULL // HC_PER_REGION)).clip(max=4)     # 0..3: HC_PER_REGION each
        a = np.select([kind == 0, kind == 1, kind == 2], [300, 100, 0], 1)
        b = np.select([kind == 0, kind == 1, kind == 2], [3, 200, 260], 0)
        single = kind == 4
        a[single] = rng.random(single.sum()) < 0.5
        b[single] = 1 - a[single]
        c1.append(a), c2.append(b)
    allk, c1, c2 = np.concatenate(keys), np.concatenate(c1), np.concatenate(c2)
    b1 = R.keys_to_reads(allk[c1 > 0], c1[c1 > 0], k, rng, n, regs)
    b2 = R.keys_to_reads(allk[c2 > 0], c2[c2 > 0], k, rng, n, regs)
    ref = oracle_of(O, k, [b1, b2])
    ref.n, ref.regions, ref.keys, ref.shared, ref.batches = n, regs, keys, shared, [b1, b2]
    ref.occ = R.region_occupancy(O, ref.batches, k, n)
    ref.recs_per_region = np.bincount(R.region_of_keys(np.concatenate([O.emit_records(k, b)[0] for b in ref.batches]), k, n), minlength=n)
    # lookups: every target key with random flanks, and absent keys whose home quad lies in a full region
    absent = np.concatenate([R.region_keys(r, n, k, 200, rng, exclude=kk) for r, kk in zip(regs, keys)])
    segs = np.concatenate([allk, absent])
    fl = R.ACGT[rng.integers(0, 4, (len(segs), 2))]
    rows = np.concatenate([fl[:, :1], R.ACGT[R.key_codes(segs, k)], fl[:, 1:]], axis=1)
    rows = rows[rng.permutation(len(rows))]
    ref.asm = b"N".join(rows.view(f"S{k + 2}").ravel().tolist())
    ref.absent = absent
    ref.validate = {(cut, lo, hi): ref.cpu.validate_sequence(ref.asm, cov_cutoff=cut, map_lo=lo, map_hi=hi, per_base=True, threads=8)
                    for cut, lo, hi in ((0, 0, MAP), (2, 0, MAP), (0, 17, 90))}
    ref.cpu.close()
    return ref


def full_or_skip(k, cls):
    ref = full_reference(k, cls)
    skip_unless_room(k, ref.n, ref.regions)
    for r in ref.regions:                                  # the designed occupancy: exactly full
        assert ref.occ[r] == FULL, (r, ref.occ[r])
    assert ref.recs_per_region.max() <= BIG                 # the ordinary region kernels, not the folding one
    if k >= 22 or (k >= 17 and cls == "B"):                 # enough hash values per quad: one chain of 2048 keys
        assert ref.shared[0] == FULL and ref.shared[1] == FULL
    assert ref.shared[1] > 0
    return ref


def count_variants(k, cls):
    v = [("direct", {}), ("partitioned", {}), ("pending 0", {"pending_bytes": 0}), ("slices", {"slice_kmers": 20000})]
    if cls != "S":
        v += [("kernel_set 1", {"kernel_set": 1}), ("kernel_set 2", {"kernel_set": 2}), ("kernel_set 4", {"kernel_set": 4})]
    return v


@pytest.mark.parametrize("k,cls", FULL_CASES, ids=[f"k{k}-{c}" for k, c in FULL_CASES])
def test_full_regions_count(kq, O, k, cls):
    import torch

    ref = full_or_skip(k, cls)
    for name, opts in count_variants(k, cls):
        path = "direct" if name == "direct" else "partitioned"
        db = handle(kq, k, cls, count_path=path, **opts)
        for b in ref.batches:
            db.count_batch(b)
        same_table(db, ref, name)
        unchanged(db, k, cls)
        db.close()
    # map-range passes over resident batches
    dev = [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() for b in ref.batches]
    maps = ref.export["key"] % np.uint64(MAP)
    db = handle(kq, k, cls, count_path="partitioned", count_map_passes=2)
    for lo, hi in ((64, 128), (0, 64)):
        db.clear()
        db.set_option("count_map_range", (lo, hi))
        for t in dev:
            db.count_batch_dev(t.data_ptr(), t.numel())
        assert H.entries_equal(db.export(), ref.export[(maps >= lo) & (maps < hi)]), (lo, hi)
    unchanged(db, k, cls)
    db.close()
    # records and entries made elsewhere
    db = handle(kq, k, cls)
    for b in ref.batches:
        keys, edges = O.emit_records(k, b)
        db.insert_records(keys, edges)
    same_table(db, ref, "insert_records")
    db.close()
    db = handle(kq, k, cls)
    db.import_entries(ref.export)
    same_table(db, ref, "import_entries")
    unchanged(db, k, cls)
    db.close()
    if k <= 28:
        src = kq.KreeqDB(k, MAP)
        db = handle(kq, k, cls)
        for t in dev:
            recs = torch.empty(t.numel(), dtype=torch.int64, device="cuda")
            counts = src.emit_packed_dev(t.data_ptr(), t.numel(), 1, recs.data_ptr(), t.numel())
            db.insert_packed_dev(recs.data_ptr(), int(counts[0]))
        same_table(db, ref, "insert_packed_dev")
        db.close(), src.close()
    if k <= 21 and cls != "S":
        src = kq.KreeqDB(k, MAP)
        db = handle(kq, k, cls)
        for t in dev:
            recs = torch.empty(t.numel(), dtype=torch.int32, device="cuda")
            aux = torch.empty(t.numel(), dtype=torch.uint8, device="cuda")
            meta = torch.empty((1, 256), dtype=torch.int64, device="cuda")
            counts = src.emit_sharded_dev(t.data_ptr(), t.numel(), 1, recs.data_ptr(), aux.data_ptr(), recs.numel(), meta.data_ptr())
            n = int(counts[0])
            db.insert_sharded_dev(recs.data_ptr(), aux.data_ptr(), n, 1, meta.data_ptr())
        same_table(db, ref, "insert_sharded_dev")
        db.close(), src.close()


@pytest.mark.parametrize("k,cls", FULL_CASES, ids=[f"k{k}-{c}" for k, c in FULL_CASES])
def test_full_regions_lookup(kq, O, k, cls):
    ref = full_or_skip(k, cls)
    db = handle(kq, k, cls, count_path="partitioned")
    for b in ref.batches:
        db.count_batch(b)
    for (cut, lo, hi), (cc, pc) in ref.validate.items():
        if (cut, lo, hi) == (0, 0, MAP):
            assert cc[0] >= len(ref.absent)                # the absent keys count as missing
        for path in ("direct", "partitioned"):
            db.set_option("lookup_path", path)
            cg, pg = db.lookup_sequence(ref.asm, cov_cutoff=cut, map_lo=lo, map_hi=hi, per_base=True)
            assert np.array_equal(cg, cc), (path, cut, lo, hi, cg, cc)
            for f in ("fw", "bw", "cov", "isFw"):
                assert np.array_equal(pg[f], pc[f]), (path, cut, f)
            cr, _ = db.lookup_sequence(ref.asm, cov_cutoff=cut, map_lo=lo, map_hi=hi)
            assert np.array_equal(cr, cc), (path, cut, lo, hi, cr, cc)
    keys = np.concatenate([ref.export["key"], ref.absent])
    perm = np.random.default_rng(k).permutation(len(keys))
    got = db.lookup_keys(keys[perm])[np.argsort(perm)]
    assert H.entries_equal(got[:len(ref.export)], ref.export)
    miss = got[len(ref.export):]
    assert np.array_equal(miss["key"], ref.absent) and (miss["cov"] == 0).all()
    # branch_scan: (present, a continuation other than the next base) per position, from the oracle's table
    seq = ref.asm[:6000 * (k + 3) // 8]
    flags = db.branch_scan(seq)
    assert np.array_equal(flags, H.branch_flags(ref.export, k, seq))
    db.close()


# ---------------------------------------------------------------------------------- 3. merge into full regions
def entries_for(O, keys, cov, rng):
    e = np.zeros(len(keys), dtype=O.ENTRY_DTYPE)
    e["key"] = keys
    e["cov"] = cov
    e["hc"] = e["cov"] > LOW
    edges = (rng.random((len(keys), 8)) * e["cov"][:, None]).astype(np.uint32)
    e["fw"], e["bw"] = edges[:, :4], edges[:, 4:]
    return e


def merged_oracle(O, k, a, b):
    x, y = O.OracleDB(k, MAP), O.OracleDB(k, MAP)
    x.import_entries(a)
    y.import_entries(b)
    x.merge(y)
    r = types.SimpleNamespace(export=x.export(), summary=x.summary(with_hist=True))
    x.close(), y.close()
    return r


MERGE_CASES = [(12, "B"), (17, "T"), (21, "B"), (25, "S"), (29, "B"), (32, "S")]


@pytest.mark.parametrize("path", ["direct", "partitioned"])
@pytest.mark.parametrize("k,cls", MERGE_CASES, ids=[f"k{k}-{c}" for k, c in MERGE_CASES])
def test_merge_into_full_regions(kq, O, k, cls, path):
    n = n_regions_of(k, cls)
    rng = np.random.default_rng(3000 + k)
    regs = roomy_regions(k, n, 2, FULL + 1, rng)
    skip_unless_room(k, n, regs)
    keys = [R.region_keys(r, n, k, FULL + 1, rng) for r in regs]
    full = np.sort(np.concatenate([kk[:FULL] for kk in keys]))
    cov8 = rng.integers(1, 200, len(full))
    covhc = rng.integers(255, 5000, len(full))
    side = rng.random(len(full)) < 0.5                      # which side holds the high-copy count
    cases = {
        "same keys": (entries_for(O, full, cov8, rng), entries_for(O, full, np.where(side, covhc, cov8[::-1]), rng)),
        "high-copy on one side, 8-bit on the other": (entries_for(O, full, np.where(side, covhc, cov8), rng),
                                                       entries_for(O, full, np.where(side, cov8, covhc), rng)),
    }
    half = np.zeros(len(full), dtype=bool)
    half[rng.permutation(len(full))[:len(full) // 2]] = True
    e = entries_for(O, full, np.where(side, covhc, cov8), rng)
    cases["disjoint, union exactly full"] = (e[half], e[~half])
    for name, (a, b) in cases.items():
        want = merged_oracle(O, k, a, b)
        assert np.bincount(R.region_of_keys(want.export["key"], k, n), minlength=n)[regs].tolist() == [FULL] * len(regs)
        dst, src = handle(kq, k, cls, merge_path=path), handle(kq, k, cls)
        dst.import_entries(a)
        src.import_entries(b)
        dst.merge(src)
        same_table(dst, want, name)
        unchanged(dst, k, cls)
        dst.close(), src.close()
    # one key more than a region holds
    extra = entries_for(O, keys[0][FULL:], [7], rng)
    dst, src = handle(kq, k, cls, merge_path=path), handle(kq, k, cls)
    dst.import_entries(e[half])
    src.import_entries(np.concatenate([e[~half], extra]))
    with pytest.raises(kq.KqError) as err:
        dst.merge(src)
        dst.summary()
    assert err.value.code == -5
    dst.close(), src.close()


# ---------------------------------------------------------------------------------- 4. a crowded high-copy tier
@functools.lru_cache(maxsize=None)
def deep_reference(k):
    from oracle import oracle as O

    reads, _ = H.synth_reads(60_000 * 262 // (151 - k), 150, 60_000, seed=4000 + k, err=0.0)      # ~262 instances per k-mer
    half = reads.find(b"\n", len(reads) // 2)
    ref = oracle_of(O, k, [reads[:half], reads[half + 1:]])
    ref.batches = [reads[:half], reads[half + 1:]]
    ref.cpu.close()
    return ref


@pytest.mark.parametrize("k,cls", [(17, "B"), (21, "S"), (21, "B"), (21, "T"), (31, "B")])
def test_deep_coverage_high_copy_tier(kq, k, cls):
    """300x of a 60 kb genome without errors: tens of thousands of k-mers in the side table, many just around 254 / 255"""
    ref = deep_reference(k)
    e = ref.export
    assert (e["hc"] == 1).sum() >= 20000 and ((e["cov"] >= 240) & (e["cov"] <= 270)).sum() >= 1000
    assert ref.summary["hist"].get(LOW, 0) > 0 and ref.summary["hist"].get(LOW + 1, 0) > 0
    for path in ("direct", "partitioned"):
        db = handle(kq, k, cls, count_path=path)
        for b in ref.batches:
            db.count_batch(b)
        same_table(db, ref, path)
        unchanged(db, k, cls)
        db.close()


AIMED = [(10, "B"), (12, "B"), (17, "B"), (21, "B"), (21, "T"), (21, "S"), (25, "S"), (31, "B")]
AIMED_KEYS = 100                   # distinct k-mers per region that pass 254 together: more than the 64 LDS entries


@functools.lru_cache(maxsize=None)
def aimed_reference(k, cls):
    from oracle import oracle as O

    n = n_regions_of(k, cls)
    rng = np.random.default_rng(5000 + k)
    regs = roomy_regions(k, n, 3, AIMED_KEYS, rng)
    keys = np.concatenate([R.region_keys(r, n, k, AIMED_KEYS, rng) for r in regs])
    ref = types.SimpleNamespace(n=n, regions=regs, keys=keys)
    # five batches of 60 copies (crossing 254 in the fifth), a sixth (already past); then 700 copies in one batch, twice
    ref.steps = [R.keys_to_reads(keys, np.full(len(keys), 60), k, rng, n, regs) for _ in range(6)]
    ref.folds = [R.keys_to_reads(keys, np.full(len(keys), 700), k, rng, n, regs) for _ in range(2)]
    ref.step = oracle_of(O, k, ref.steps)
    ref.fold = oracle_of(O, k, ref.folds)
    ref.step.cpu.close(), ref.fold.cpu.close()
    ref.occ = R.region_occupancy(O, ref.steps + ref.folds, k, n)
    ref.fold_recs = np.bincount(R.region_of_keys(O.emit_records(k, ref.folds[0])[0], k, n), minlength=n)
    ref.step_recs = np.bincount(R.region_of_keys(np.concatenate([O.emit_records(k, b)[0] for b in ref.steps]), k, n), minlength=n)
    return ref


@pytest.mark.parametrize("k,cls", AIMED, ids=[f"k{k}-{c}" for k, c in AIMED])
def test_many_kmers_cross_254_in_one_region(kq, k, cls):
    """more than 64 distinct k-mers of one region move past 254 instances in one table pass (the global side-table path
    of the region kernels' LDS sums), with the region under 32 x 2048 records of a pass and, separately, above it (the
    folding kernel); then again with those k-mers already in the side table"""
    ref = aimed_reference(k, cls)
    for r in ref.regions:
        assert ref.occ[r] == AIMED_KEYS > 64
        assert ref.step_recs[r] <= BIG < ref.fold_recs[r]
    assert (ref.step.export["cov"][np.isin(ref.step.export["key"], ref.keys)] == 360).all()
    for pending in (0, -1):
        db = handle(kq, k, cls, count_path="partitioned", pending_bytes=pending)
        for i, b in enumerate(ref.steps):
            db.count_batch(b)
            if pending == 0 and i == 3:
                assert db.info()["hc_used"] == 0          # 240 instances each: nothing in the side table yet
        same_table(db, ref.step, f"steps, pending {pending}")
        assert db.info()["hc_used"] == (ref.step.export["hc"] == 1).sum()
        unchanged(db, k, cls)
        db.close()
        db = handle(kq, k, cls, count_path="partitioned", pending_bytes=pending)
        for b in ref.folds:
            db.count_batch(b)
        same_table(db, ref.fold, f"folding, pending {pending}")
        unchanged(db, k, cls)
        db.close()
    db = handle(kq, k, cls, count_path="direct")
    for b in ref.steps:
        db.count_batch(b)
    same_table(db, ref.step, "direct")
    db.close()


# ---------------------------------------------------------------------------------- 5. side-table growth with live entries
@pytest.mark.parametrize("k,cls,path", [(21, "B", "partitioned"), (21, "S", "direct"), (31, "B", "partitioned")])
def test_side_table_grows_with_live_entries(kq, O, k, cls, path):
    # 31 000 reads of a 22 kb genome: ~21 000 k-mers at ~300 instances in 7.8 M bases, under the bound of the 2^16-entry
    # side table (2^15 x 255 instances); the same reads again double that
    b1, _ = H.synth_reads(31_000, 250, 22_000, seed=6000 + k, err=0.0)
    b2 = b1
    assert len(b1) < (1 << 15) * 255
    one = oracle_of(O, k, [b1])
    both = oracle_of(O, k, [b1, b2])
    one.cpu.close(), both.cpu.close()
    n_hc = (one.export["hc"] == 1).sum()
    assert n_hc >= 20000
    db = handle(kq, k, cls, trust=False, count_path=path)
    db.count_batch(b1)
    db.sync()
    i = db.info()
    assert i["hc_total"] == 1 << 16 and i["hc_used"] == n_hc, i
    same_table(db, one, "before growth")
    db.count_batch(b2)
    i = db.info()
    assert i["hc_total"] > 1 << 16 and i["hc_used"] == (both.export["hc"] == 1).sum(), i
    same_table(db, both, "after growth")
    db.close()
    # the same growth through merge
    dst = handle(kq, k, cls, trust=False, count_path=path)
    src = handle(kq, k, cls, trust=False, count_path=path)
    dst.count_batch(b1)
    src.count_batch(b2)
    assert dst.info()["hc_total"] == 1 << 16 and dst.info()["hc_used"] == n_hc
    dst.merge(src)
    assert dst.info()["hc_total"] > 1 << 16
    same_table(dst, both, "merge")
    dst.close(), src.close()


# ---------------------------------------------------------------------------------- 6. histogram past HIST_SMALL
@pytest.mark.parametrize("k,cls", [(21, "B"), (31, "S")])
def test_histogram_past_4096(kq, O, k, cls):
    rng = np.random.default_rng(7000 + k)
    keys = np.unique(R.canonical(np.frombuffer(rng.bytes(8 * 40000), dtype=np.uint64) & np.uint64((1 << (2 * k)) - 1), k))
    keys = rng.permutation(keys)[:30000]
    cov = rng.integers(4096, 30000, len(keys))
    special = [LOW, LOW + 1, 4095, 4096, 4097, (1 << 32) - 1, 1, 2]
    cov[:len(special)] = special
    cov[len(special):15000] = rng.integers(1, 4096, 15000 - len(special))
    a = entries_for(O, keys[:20000], cov[:20000], rng)
    b = entries_for(O, keys[10000:], cov[10000:], rng)
    want = merged_oracle(O, k, a, b)
    alone = merged_oracle(O, k, a, a[:0])
    big = sum(c for v, c in want.summary["hist"].items() if v >= 4096)
    assert big >= 10000 and all(want.summary["hist"].get(v, 0) > 0 for v in (LOW, LOW + 1, 4095, 4096, (1 << 32) - 1))
    for path in ("direct", "partitioned"):
        dst, src = handle(kq, k, cls, merge_path=path), handle(kq, k, cls)
        dst.import_entries(a)
        same_table(dst, alone, "import")
        src.import_entries(b)
        dst.merge(src)
        same_table(dst, want, path)
        dst.close(), src.close()
