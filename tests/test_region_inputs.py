"""CPU checks of tests/region_inputs.py, the numpy restatement of the table geometry and the region-crowding inputs that
tests/test_gpu_regions.py builds with it: the hash is a bijection with key_of_hash its inverse, generated keys are what
they claim (canonical, distinct, in the region and home quad asked for), and the occupancy counter agrees with a
brute-force walk of the reads."""
import numpy as np
import pytest

from tests import region_inputs as R

# region counts of the table classes of test_gpu_regions.py (S, B, T at k <= 28; S at k >= 29 is a multiple of 256)
N_REGIONS = (732, 768, 3584, 69888)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.mark.parametrize("k", range(2, 33))
def test_key_of_hash_inverts_table_hash(k):
    rng = np.random.default_rng(k)
    full = (1 << (2 * k)) - 1
    x = np.frombuffer(rng.bytes(8 * 20000), dtype=np.uint64) & np.uint64(full)
    x = np.concatenate([x, np.array([0, full, full >> 1, (full >> 1) + 1], dtype=np.uint64)])
    h = R.table_hash(x, k)
    assert not (h & np.uint64((1 << (64 - 2 * k)) - 1)).any()      # left-aligned: the low 64 - 2k bits are zero
    assert np.array_equal(R.key_of_hash(h, k), x)
    assert np.array_equal(R.table_hash(R.key_of_hash(h, k), k), h)


@pytest.mark.parametrize("k", range(2, 12))
def test_table_hash_is_a_bijection(k):
    x = np.arange(4 ** k, dtype=np.uint64)
    v = R.table_hash(x, k) >> np.uint64(64 - 2 * k)
    assert np.array_equal(np.sort(v), x)


def test_hash_families_differ_at_the_split():
    """k = 24 is the last Feistel k, k = 25 the first multiply k: both must mix (no identity on either side)"""
    for k in (24, 25):
        x = np.arange(1, 1000, dtype=np.uint64)
        v = R.table_hash(x, k) >> np.uint64(64 - 2 * k)
        assert (v != x).all() and len(np.unique(v)) == len(x)


@pytest.mark.parametrize("k", [2, 7, 12, 16, 21, 29, 32])
@pytest.mark.parametrize("n", N_REGIONS)
def test_value_range_is_the_region(k, n):
    """the hash values value_range() gives for a region map to it; the values just outside map to other regions"""
    rng = np.random.default_rng(k * n)
    for r in [0, n - 1] + [int(x) for x in rng.integers(0, n, 5)]:
        lo, hi = R.value_range(r, n, k)
        if hi == lo:                       # a small key space leaves some regions without any value
            continue
        pad = 64 - 2 * k
        inside = [lo, hi - 1, (lo + hi) // 2]
        got = R.hash_region(np.array([v << pad for v in inside], dtype=np.uint64), n)
        assert (got == r).all(), (r, got)
        if lo > 0:
            assert int(R.hash_region(np.array([(lo - 1) << pad], dtype=np.uint64), n)[0]) < r
        if hi < 1 << (2 * k):
            assert int(R.hash_region(np.array([hi << pad], dtype=np.uint64), n)[0]) > r


@pytest.mark.parametrize("k,n", [(6, 16), (8, 732), (10, 732), (11, 3584), (12, 3584), (12, 69888)])
def test_region_keys_exhaustive(k, n):
    """small key spaces: the enumeration of a region's canonical keys is complete and exact"""
    keys = np.arange(4 ** k, dtype=np.uint64)
    keys = keys[R.is_canonical(keys, k)]
    reg = R.region_of_keys(keys, k, n)
    for r in (0, n // 2, n - 1):
        assert np.array_equal(R.all_region_keys(r, n, k), keys[reg == r])
        total, per_quad = R.region_capacity(r, n, k)
        assert total == (reg == r).sum() and sum(per_quad.values()) == total


@pytest.mark.parametrize("k", [10, 12, 17, 21, 24, 25, 28, 29, 32])
@pytest.mark.parametrize("n", N_REGIONS)
def test_generated_keys(k, n):
    rng = np.random.default_rng(100 * k + n % 97)
    r = int(rng.integers(0, n))
    for layout in ("quad", "wrap", "random"):
        keys, same = R.full_region_keys(r, n, k, rng, layout)
        if k <= 12:
            avail = len(R.all_region_keys(r, n, k))
            assert len(keys) == min(avail, R.REGION_SLOTS)
        else:
            assert len(keys) == R.REGION_SLOTS
        assert len(np.unique(keys)) == len(keys)
        assert R.is_canonical(keys, k).all()
        if k < 32:
            assert (keys < np.uint64(1 << (2 * k))).all()
        assert (R.region_of_keys(keys, k, n) == r).all()
        homes = R.home_of_keys(keys, k)
        if layout == "wrap":
            assert (homes == R.QUAD_MASK).sum() == same
        if layout != "random":
            assert np.bincount(homes // 4).max() >= same
            if k >= 22 or (k >= 17 and n <= 3584):         # enough hash values per home quad: every key shares it
                assert same == R.REGION_SLOTS, (layout, same)


def walk_kmers(batch: bytes, k):
    """brute force: canonical key of every k-base window of ACGT bases"""
    code = {ord(c): i for i, c in enumerate("ACGT")}
    out = []
    for read in batch.split(b"\n"):
        for i in range(len(read) - k + 1):
            w = read[i:i + k]
            if all(c in code for c in w):
                fw = sum(code[c] << (2 * j) for j, c in enumerate(w))
                rv = sum((3 - code[c]) << (2 * (k - 1 - j)) for j, c in enumerate(w))
                out.append(min(fw, rv))
    return out


@pytest.mark.parametrize("k,n", [(11, 732), (21, 3584), (25, 768), (32, 3584)])
def test_reads_and_occupancy(O, k, n):
    rng = np.random.default_rng(k)
    targets = [int(x) for x in rng.choice(n, 3, replace=False)]
    keys = np.concatenate([R.region_keys(r, n, k, 40, rng) for r in targets])
    copies = rng.integers(1, 12, len(keys))
    batch = R.keys_to_reads(keys, copies, k, rng, n_regions=n, avoid=targets)
    # the oracle's k-mer walk == a brute-force walk; every copy is one read with its key
    walked = walk_kmers(batch, k)
    assert np.array_equal(np.sort(O.emit_records(k, batch)[0]), np.sort(np.array(walked, dtype=np.uint64)))
    reads = [r for r in batch.split(b"\n") if r]           # a missing flank is a read end: an empty piece beside the read
    assert len(reads) == copies.sum()
    occ = R.region_occupancy(O, [batch], k, n)
    brute = np.bincount(R.region_of_keys(np.unique(np.array(walked, dtype=np.uint64)), k, n), minlength=n)
    assert np.array_equal(occ, brute)
    for r in targets:                                      # flanks never reach the target regions
        assert occ[r] == 40
    # every flank base and the read end occur on both sides, over both strands
    assert {len(r) for r in reads} == {k, k + 1, k + 2}
    assert {r[:1] for r in reads if len(r) == k + 2} == {b"A", b"C", b"G", b"T"}
    assert {r[-1:] for r in reads if len(r) == k + 2} == {b"A", b"C", b"G", b"T"}
    assert {int(x) for x in keys} <= set(walked)


def test_neighbours_avoided_exactly():
    """a key whose every flank would hit a target region still gets reads: bare copies only"""
    k, n = 12, 16
    rng = np.random.default_rng(1)
    keys = R.region_keys(3, n, k, 200, rng)
    avoid = list(range(n))                                  # every region: no flank is allowed
    batch = R.keys_to_reads(keys, np.full(len(keys), 3), k, rng, n_regions=n, avoid=avoid)
    reads = [r for r in batch.split(b"\n") if r]
    assert len(reads) == 3 * len(keys) and all(len(r) == k for r in reads)
