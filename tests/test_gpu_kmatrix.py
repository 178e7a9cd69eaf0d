"""Every k from 2 to 32 on every table class against the CPU oracle, exactly.

The count, lookup, merge and export paths change with k (Feistel table hash up to k = 24, xorshift-multiply above; 5-byte
narrow records up to k = 21, packed 8-byte records up to 28, hash-remainder records from 29, where the region implies the
top 8 hash bits) and with the table's region count, which the capacity hint chooses:
  S  hint 0            < 2048 regions       FMT_PACK8 / FMT_WIDE records
  B  hint 5 M          >= 2048 regions      bucketed: FMT_NARROW / packed / FMT_TOP8
  T  hint 100 M        >= 2^16 regions      FMT_TIGHT for k <= 21 (about 2.3 GB of HBM: a few k only, one handle at a time)
Each case asserts the class it names, before and after counting.  Inputs: synthetic reads with errors, N and lower case,
a high-copy k-mer for every k and, for even k, min(60, 4^(k/2)) planted palindromic k-mers (forward == reverse complement:
never "forward", which decides their edge bytes and per-base isFw), one of them in the high-copy tier.  For k <= 11 every canonical key goes into the table (de Bruijn
sequences), and export must return exactly the canonical keys computed in numpy: the table hash is a bijection and
key_of_hash its inverse over the whole key space.  For larger k a hand-built key set makes the import / export /
lookup_keys round trip.  The oracle's result of each k is computed once and shared by the cases of that k."""
import functools
import types

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

MAP = 128
HINT = {"S": 0, "B": 5_000_000, "T": 100_000_000}
T_KS = (2, 8, 12, 16, 18, 20, 21, 22, 24, 25, 29, 30, 32)
CASES = [(k, c) for k in range(2, 33) for c in ("S", "B", "T") if c != "T" or k in T_KS]
CASE_IDS = [f"k{k}-{c}" for k, c in CASES]
LOOKUPS = [(lo, hi, cut) for lo, hi in ((0, MAP), (17, 90)) for cut in (0, 2)]
SLICE_KMERS = 200_000          # the partitioned count of class S cuts each batch into several slices


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


def assert_class(db, cls):
    regions = db.info()["slots_total"] // 2048
    if cls == "S":
        assert regions < 2048, (cls, regions)
    elif cls == "B":
        assert 2048 <= regions < (1 << 16), (cls, regions)
    else:
        assert regions >= (1 << 16), (cls, regions)


def counted(kq, k, cls, batches, path, slice_kmers=None, map_ranges=((0, MAP),), hint=None, trust=False):
    db = kq.KreeqDB(k, MAP, capacity_hint=HINT[cls] if hint is None else hint)
    assert_class(db, cls)
    db.set_option("count_path", path)
    if trust:
        db.set_option("trust_capacity", 1)
    if slice_kmers:
        db.set_option("slice_kmers", slice_kmers)
    for r in map_ranges:
        db.set_option("count_map_range", r)
        for b in batches:
            db.count_batch(b)
    assert_class(db, cls)                                 # counting did not grow the table out of its class
    return db


def oracle_self_merge(O, k, table):
    twice = O.OracleDB(k, MAP)
    twice.import_entries(table)
    once = O.OracleDB(k, MAP)
    once.import_entries(table)
    twice.merge(once)
    out = twice.summary(with_hist=True), twice.export()
    twice.close(), once.close()
    return out


# ---------------------------------------------------------------------------------- per-k reads, assembly and oracle tables
@functools.lru_cache(maxsize=1)
def reference(k):
    from oracle import oracle as O

    reads, genome = H.synth_reads(20000, 150, 60000, seed=7000 + k, err=0.005, n_rate=0.002)
    pals = H.palindromes(k, 60, seed=7100 + k) if k % 2 == 0 else []
    hot, hot_reads = H.hot_kmer_reads(k, seed=7200 + k)
    planted = H.plant_palindromes(k, pals, seed=7300 + k)
    # four batches (later ones add to existing entries; an S table takes each without outgrowing its class)
    cuts = [0] + [reads.find(b"\n", len(reads) * i // 4) + 1 for i in (1, 2, 3)] + [len(reads) + 1]
    batches = [reads[a:b - 1] for a, b in zip(cuts, cuts[1:])]
    batches[-1] += b"\n" + b"\n".join(planted + hot_reads)
    # assembly: the genome with errors, an N run, every planted palindrome in its flanks, the high-copy k-mer
    rng = np.random.default_rng(7400 + k)
    g = bytearray(genome)
    for pos in rng.integers(0, len(g), 150):
        g[pos] = b"ACGT"[rng.integers(0, 4)]
    pal_segments = b"N".join(dict.fromkeys(r.upper() for r in planted))
    asm = bytes(g) + b"NNNNNNN" + pal_segments + b"N" + b"G" + hot + b"T" + b"NNN" + H.ACGT[rng.integers(0, 4, 3000)].tobytes()

    cpu = O.OracleDB(k, MAP)
    for b in batches:
        cpu.count_batch(b, threads=8)
    r = types.SimpleNamespace(k=k, batches=batches, asm=asm)
    r.summary = cpu.summary(with_hist=True)
    r.export = cpu.export()
    r.validate = {q: cpu.validate_sequence(asm, cov_cutoff=q[2], map_lo=q[0], map_hi=q[1], per_base=True, threads=8) for q in LOOKUPS}
    cpu.close()
    r.summary2, r.export2 = oracle_self_merge(O, k, r.export)
    cand = H.canonical_keys_of(rng.integers(0, np.iinfo(np.uint64).max, 3000, dtype=np.uint64, endpoint=True)
                               & np.uint64((1 << (2 * k)) - 1), k)
    r.absent = np.unique(cand[~np.isin(cand, r.export["key"])])
    # the inputs are what this file claims
    codes = {c: i for i, c in enumerate(b"ACGT")}
    pal_keys = np.array([H.key_of_codes([codes[c] for c in p]) for p in pals], dtype=np.uint64)
    assert np.isin(pal_keys, r.export["key"]).all()
    assert (r.export["hc"] == 1).any() and r.export["cov"].max() > 255
    return r


# ---------------------------------------------------------------------------------- one case per (k, class)
@pytest.mark.parametrize("k,cls", CASES, ids=CASE_IDS)
def test_kmatrix(kq, O, k, cls):
    """count (both paths), lookups (sequence and keys), merge into the other geometry; the cases of one k run together and
    share the oracle's result"""
    ref = reference(k)
    if cls == "S":
        check_emit(kq, O, ref)
    check_count(kq, ref, cls)
    check_lookup(kq, ref, cls)
    check_merge(kq, ref, cls)


# ---------------------------------------------------------------------------------- 1. count (+ emit once per k)
def check_emit(kq, O, ref):
    k = ref.k
    db = kq.KreeqDB(k, MAP)
    for b in ref.batches:
        keys, edges = db.emit_records(b)
        ok, oe = O.emit_records(k, b)
        assert np.array_equal(keys, ok) and np.array_equal(edges, oe), "emit_records"
    db.close()


def check_count(kq, ref, cls):
    k = ref.k
    for path in ("direct", "partitioned"):
        db = counted(kq, k, cls, ref.batches, path, slice_kmers=SLICE_KMERS if path == "partitioned" and cls == "S" else None)
        assert db.summary(with_hist=True) == ref.summary, path
        assert H.entries_equal(db.export(), ref.export), path
        assert db.info()["slots_used"] == ref.summary["distinct"], path
        db.close()
    if cls != "B":
        return
    # map-range passes: [17, 90) on one handle, the two ranges of its complement one after the other on another
    m = ref.export["key"] % MAP
    inside = (m >= 17) & (m < 90)
    piece = counted(kq, k, cls, ref.batches, "partitioned", map_ranges=((17, 90),))
    rest = counted(kq, k, cls, ref.batches, "direct", map_ranges=((0, 17), (90, MAP)))
    assert H.entries_equal(piece.export(), ref.export[inside])
    assert H.entries_equal(rest.export(), ref.export[~inside])
    piece.merge(rest)
    assert H.entries_equal(piece.export(), ref.export)
    assert piece.summary(with_hist=True) == ref.summary
    piece.close(), rest.close()


# ---------------------------------------------------------------------------------- 2. + 3. lookups
def check_lookup(kq, ref, cls):
    k = ref.k
    db = counted(kq, k, cls, ref.batches, "direct")
    for (lo, hi, cut), (cc, pc) in ref.validate.items():
        for path in ("direct", "partitioned"):
            db.set_option("lookup_path", path)
            cg, pg = db.lookup_sequence(ref.asm, cov_cutoff=cut, map_lo=lo, map_hi=hi, per_base=True)
            assert np.array_equal(cg, cc), (path, lo, hi, cut, cg, cc)
            for f in ("fw", "bw", "cov", "isFw"):
                bad = np.flatnonzero(pg[f] != pc[f])
                assert len(bad) == 0, (path, lo, hi, cut, f, bad[:10], ref.asm[bad[0]:bad[0] + k] if len(bad) else None)
            cr, _ = db.lookup_sequence(ref.asm, cov_cutoff=cut, map_lo=lo, map_hi=hi)
            assert np.array_equal(cr, cc), (path, lo, hi, cut, cr, cc)
    want = ref.export
    keys = np.concatenate([want["key"], ref.absent])
    perm = np.random.default_rng(k).permutation(len(keys))
    got = db.lookup_keys(keys[perm])[np.argsort(perm)]
    assert H.entries_equal(got[:len(want)], want)
    miss = got[len(want):]
    assert np.array_equal(miss["key"], ref.absent) and (miss["cov"] == 0).all()
    db.close()


# ---------------------------------------------------------------------------------- 4. merge into the other geometry
def check_merge(kq, ref, cls):
    k = ref.k
    src = counted(kq, k, cls, ref.batches, "direct")
    other = "B" if cls == "S" else "S"
    for path in ("partitioned", "direct"):
        dst = kq.KreeqDB(k, MAP, capacity_hint=HINT[other])
        assert_class(dst, other)
        dst.set_option("merge_path", path)
        dst.merge(src)
        assert dst.summary(with_hist=True) == ref.summary, path
        assert H.entries_equal(dst.export(), ref.export), path
        dst.merge(src)                                      # every key present: counters double, saturating
        assert dst.summary(with_hist=True) == ref.summary2, path
        assert H.entries_equal(dst.export(), ref.export2), path
        dst.close()
    src.close()


# ---------------------------------------------------------------------------------- whole key space, k = 2..11
KEYSPACE = [(k, c, p) for k in range(2, 12) for c in ("S", "B", "T") if c != "T" or k in (2, 8) for p in ("direct", "partitioned")]


@functools.lru_cache(maxsize=1)
def keyspace_reference(k):
    from oracle import oracle as O

    seq = H.de_bruijn_linear(k)
    n_kmers = len(seq) - k + 1
    rng = np.random.default_rng(7500 + k)
    cuts = np.sort(rng.choice(np.arange(1, n_kmers), min(2000, n_kmers // 3), replace=False)).tolist()
    # pieces that overlap by k - 1 bases: each k-mer lies in exactly one piece
    pieces = b"\n".join(seq[a:b + k - 1] for a, b in zip([0] + cuts, cuts + [n_kmers]))
    batches = [seq, H.revcomp_bases(seq), pieces]
    cpu = O.OracleDB(k, MAP)
    for b in batches:
        cpu.count_batch(b, threads=8)
    r = types.SimpleNamespace(batches=batches, summary=cpu.summary(with_hist=True), export=cpu.export(), keys=H.all_canonical_keys(k))
    cpu.close()
    return r


@pytest.mark.parametrize("k,cls,path", KEYSPACE, ids=[f"k{k}-{c}-{p}" for k, c, p in KEYSPACE])
def test_whole_key_space(kq, k, cls, path):
    ref = keyspace_reference(k)
    # k = 11 holds 2.1 M keys: the hint of an S table is then an honest bound (a batch would otherwise pre-grow the table by
    # its 4^11 k-mers into the B class)
    big = cls == "S" and k == 11
    db = counted(kq, k, cls, ref.batches, path, hint=2_800_000 if big else None, trust=big)
    s = db.summary(with_hist=True)
    assert s["distinct"] == H.n_canonical(k) and s["missing"] == 4 ** k - H.n_canonical(k), s
    e = db.export()
    assert np.array_equal(e["key"], ref.keys)
    assert s == ref.summary
    assert H.entries_equal(e, ref.export)


# ---------------------------------------------------------------------------------- hand-built keys, k = 12..32
def boundary_keys(k, rng):
    """canonical keys at the edges of the key space and of the hash halves, plus 10 000 random ones"""
    full = (1 << (2 * k)) - 1
    cand = [0, full, H.max_canonical_key(k)]
    if k <= 24:                                           # the Feistel halves: low k bits | high k bits << k
        ones = (1 << k) - 1
        rnd = [int(v) for v in rng.integers(0, 1 << k, 8)]
        for lo in [0, ones] + rnd[:4]:
            for hi in [0, ones] + rnd[4:]:
                if lo in (0, ones) or hi in (0, ones):
                    cand.append(lo | (hi << k))
    mid = 1 << (2 * k - 1)
    cand += list(range(mid - 64, mid + 64))
    if k == 32:
        cand += [(1 << 63) + i for i in range(64)] + [full - i for i in range(64)]
        cand += [int(v) | (1 << 63) for v in rng.integers(0, 1 << 63, 500, dtype=np.uint64)]
    cand = np.array(cand, dtype=np.uint64)
    special = cand[cand <= H.revcomp_keys(cand, k)]        # the canonical ones among them
    rand = H.canonical_keys_of(np.frombuffer(rng.bytes(8 * 10000), dtype=np.uint64) & np.uint64(full), k)
    return np.unique(np.concatenate([special, rand]))


IMPORT_CASES = [(k, c) for k in range(12, 33) for c in ("S", "B")]


@pytest.mark.parametrize("k,cls", IMPORT_CASES, ids=[f"k{k}-{c}" for k, c in IMPORT_CASES])
def test_import_round_trip(kq, O, k, cls):
    rng = np.random.default_rng(7600 + k)
    keys = boundary_keys(k, rng)
    mid = 1 << (2 * k - 1)
    assert keys[0] == 0 and int(keys[-1]) == H.max_canonical_key(k)
    assert ((keys >= mid - 64) & (keys < mid)).any() and ((keys >= mid) & (keys < mid + 64)).any()
    e = np.zeros(len(keys), dtype=O.ENTRY_DTYPE)
    e["key"] = keys
    hc = rng.random(len(keys)) < 0.2
    hc[:2] = (False, True)
    e["cov"] = np.where(hc, rng.integers(255, 1 << 20, len(keys)), rng.integers(1, 255, len(keys)))
    e["cov"][2:4] = (254, 255)                               # both sides of the 8-bit tier
    hc[2:4] = (False, True)
    e["hc"] = hc
    frac = rng.random((len(keys), 8))
    edges = (frac * e["cov"][:, None]).astype(np.uint32)
    e["fw"], e["bw"] = edges[:, :4], edges[:, 4:]
    e["fw"][2], e["bw"][3] = 254, 255
    db = kq.KreeqDB(k, MAP, capacity_hint=HINT[cls])
    assert_class(db, cls)
    db.import_entries(e)
    assert_class(db, cls)
    got = db.export()
    assert np.array_equal(got["key"], keys)
    assert H.entries_equal(got, e)
    cpu = O.OracleDB(k, MAP)
    cpu.import_entries(e)
    assert H.entries_equal(got, cpu.export())
    assert db.summary(with_hist=True) == cpu.summary(with_hist=True)
    perm = rng.permutation(len(keys))
    assert H.entries_equal(db.lookup_keys(keys[perm])[np.argsort(perm)], e)
