"""kq_subgraph_seed / kq_subgraph_expand / kq_subgraph_trim through the C ABI (ctypes binding) against the Python restatement
of the reference's subgraph mode (tests/subgraph_ref.py, itself pinned by the reference's goldens in
tests/test_subgraph_ref.py).  Every comparison is the whole exported table, entry by entry, and exact."""
import numpy as np
import pytest

from oracle.variants import hash_kmer
from tests import helpers as H
from tests import subgraph_ref as R

pytestmark = pytest.mark.gpu

MAPS = 128


@pytest.fixture(scope="module")
def kq():
    from kreeq_amd import capi
    assert capi.device_available()
    return capi


def rand_bases(rng, n):
    return H.ACGT[rng.integers(0, 4, n)].tobytes()


def counted(kq, k, reads, hint=1 << 16):
    db = kq.KreeqDB(k, MAPS, 0, capacity_hint=hint)
    db.count_batch(reads)
    return db, R.table_of(db.export())


def new_sub(kq, k, hint=1 << 12):
    return kq.KreeqDB(k, MAPS, 0, capacity_hint=hint)


def same(sub_handle, want_table):
    return H.entries_equal(sub_handle.export(), R.entries_of(want_table))


# ------------------------------------------------------------------------------------------------------------------ seed
def seed_batch(k, genome, rng):
    """>= 4 segments that share k-mers; about half of the bases are absent from the reads; a constructed k-mer twice in
    one segment with different neighbours; segments of k - 1 and of exactly k bases; lower case; an N run"""
    absent = rand_bases(rng, 120)
    w = rand_bases(rng, k)                                               # absent k-mer, twice in one segment
    return b"".join([genome[100:200], b"N", genome[150:260].lower(), b"NNNN", absent, b"\n",
                     genome[100:180] + rand_bases(rng, 60), b"N",
                     b"A" + w + b"C" + rand_bases(rng, 10) + b"G" + w + b"T", b"n",
                     absent[10:80], b"N", genome[300:300 + k - 1], b"N", genome[400:400 + k], b"NN",
                     genome[100:200], b"N", absent.lower()])


@pytest.fixture(scope="module", params=[21, 31])
def seed_case(request, kq):
    k = request.param
    reads, genome = H.synth_reads(400, 100, 1500, seed=100 + k, err=0.004, n_rate=0.001)
    db, table = counted(kq, k, reads)
    return k, db, table, seed_batch(k, genome, np.random.default_rng(k))


@pytest.mark.parametrize("no_reference", [False, True])
def test_seed(kq, seed_case, no_reference):
    k, db, table, batch = seed_case
    sub = new_sub(kq, k)
    db.subgraph_seed(sub, batch, no_reference)
    want = R.seed(table, [batch], k, no_reference)
    assert any(v[2] > table[key][2] for key, v in want.items() if key in table)      # a k-mer of several segments
    assert no_reference or any(key not in table for key in want)                     # constructed k-mers
    assert same(sub, want)
    # seeding adds up over calls like over segments
    db.subgraph_seed(sub, batch[:300], no_reference)
    want2 = R.seed(table, [batch, batch[:300]], k, no_reference)
    assert same(sub, want2)
    assert sub.summary() == R.summary(want2, k)


def test_seed_first_occurrence_decides(kq, seed_case):
    """the constructed k-mer that occurs twice in one segment carries the neighbours of its first position only"""
    k, db, table, _ = seed_case
    rng = np.random.default_rng(7)
    w = rand_bases(rng, k)
    seg = b"A" + w + b"C" + rand_bases(rng, 5) + b"G" + w + b"T"
    sub = new_sub(kq, k)
    db.subgraph_seed(sub, seg)
    want = R.seed(table, [seg], k)
    key, _ = hash_kmer([R.CTOI[chr(c)] for c in w], k)
    assert key not in table and want[key][2] == 1 and sum(want[key][0]) + sum(want[key][1]) == 2
    assert same(sub, want)


@pytest.mark.parametrize("no_reference", [False, True])
def test_seed_expand_trim_k4_de_bruijn(kq, no_reference):
    """k = 4 on B(4, 4): palindromic k-mers, self-loops, every edge present"""
    k = 4
    text = H.de_bruijn_linear(k)
    db, table = counted(kq, k, text + b"\n" + text[:40])
    batch = text[:60] + b"N" + text[30:120].lower() + b"NN" + text[200:203] + b"N" + text[210:214]
    sub = new_sub(kq, k)
    db.subgraph_seed(sub, batch, no_reference)
    want = R.seed(table, [batch], k, no_reference)
    assert same(sub, want)
    for depth in (1, 2):
        added = db.subgraph_expand(sub, depth)
        assert added == R.traversal(table, want, k, depth)
        assert same(sub, want)
    sub.subgraph_trim(0)
    R.trim(want, k, 0)
    assert same(sub, want)
    assert sub.summary() == R.summary(want, k)


# ------------------------------------------------------------------------------------------------------------- high copy
@pytest.mark.parametrize("k", [21, 31])
def test_high_copy(kq, k):
    """cov >= 255: one k-mer in the seed, one reached only by expansion, one seeded from 3 segments"""
    hot_a, reads_a = H.hot_kmer_reads(k, seed=1)
    hot_b, reads_b = H.hot_kmer_reads(k, seed=2)
    hot_c, reads_c = H.hot_kmer_reads(k, seed=3)
    bg, genome = H.synth_reads(200, 100, 800, seed=9, err=0.0)
    db, table = counted(kq, k, b"\n".join(reads_a + reads_b + reads_c) + b"\n" + bg)
    assert sum(v[2] >= 255 for v in table.values()) >= 3
    near_b = reads_b[0][:k]                                              # a flank k-mer next to hot_b: hot_b is one step away
    batch = b"N".join([hot_a, near_b, hot_c, hot_c, hot_c, genome[50:120]])
    sub = new_sub(kq, k)
    db.subgraph_seed(sub, batch)
    want = R.seed(table, [batch], k)
    assert max(v[2] for v in want.values()) >= 3 * 320
    assert same(sub, want)
    n_hc_seed = sum(v[2] >= 255 for v in want.values())
    assert db.subgraph_expand(sub, 1) == R.traversal(table, want, k, 1)
    assert sum(v[2] >= 255 for v in want.values()) == n_hc_seed + 1      # hot_b came in by expansion
    assert same(sub, want)
    sub.subgraph_trim(0)                                                 # clears counters of the high-copy tier too
    R.trim(want, k, 0)
    assert same(sub, want)
    assert sub.summary() == R.summary(want, k)


# ------------------------------------------------------------------------------------------------------------- traversal
def bubble_genome(k):
    """reads of a 400-base genome + a second haplotype with one SNP (a bubble) + a tandem repeat (a cycle);
    -> (reads, seed sequence): the seed ends 2 k-mers before the bubble opens, so that both branches arrive at the k-mer
    behind the bubble in the same round"""
    reads, genome = H.synth_reads(150, 100, 400, seed=5, err=0.002)
    s = 230                                                              # SNP position
    alt = genome[:s] + bytes([H.ACGT[(list(b"ACGT").index(genome[s]) + 1) & 3]]) + genome[s + 1:]
    alt_reads = [alt[i:i + 80] for i in range(s - 79, s + 1, 3)]
    unit = b"ACGGTCA"
    rep = genome[320:350] + unit * 8 + genome[350:380]                   # joins the genome's graph on both sides
    rep_reads = [rep[i:i + 70] for i in range(0, len(rep) - 69, 2)]
    seed_seq = genome[s - 23 - 50:s - 2] + b"N" + unit * 4               # ... and a seed inside the repeat's cycle
    return reads + b"\n" + b"\n".join(alt_reads + rep_reads), seed_seq


@pytest.fixture(scope="module")
def bubble_case(kq):
    k = 21
    reads, seed_seq = bubble_genome(k)
    db, table = counted(kq, k, reads)
    return k, db, table, seed_seq


@pytest.mark.parametrize("depth", [0, 1, 2, 11, 30])
def test_traversal_depths(kq, bubble_case, depth):
    k, db, table, seed_seq = bubble_case
    sub = new_sub(kq, k)
    db.subgraph_seed(sub, seed_seq)
    want = R.seed(table, [seed_seq], k)
    added = db.subgraph_expand(sub, depth)
    assert added == R.traversal(table, want, k, depth)
    assert (added == 0) == (depth == 0)
    assert same(sub, want)
    assert sub.summary() == R.summary(want, k)


def test_traversal_closure(kq, bubble_case):
    """the graph of the 400-base genome closes within 255 rounds: a larger depth adds nothing, and n_added says so"""
    k, db, table, seed_seq = bubble_case
    subs = []
    for depth in (250, 255):
        sub = new_sub(kq, k)
        db.subgraph_seed(sub, seed_seq)
        want = R.seed(table, [seed_seq], k)
        assert db.subgraph_expand(sub, depth) == R.traversal(table, want, k, depth)
        assert same(sub, want)
        subs.append(sub)
    assert H.entries_equal(subs[0].export(), subs[1].export())
    assert db.subgraph_expand(subs[1], 5) == 0
    assert H.entries_equal(subs[0].export(), subs[1].export())


@pytest.fixture(scope="module")
def wide_case(kq):
    """>= 20 000 seed k-mers: the frontier spans many workgroups"""
    k = 21
    reads, genome = H.synth_reads(3000, 150, 30000, seed=77, err=0.01, n_rate=0.0005)
    db, table = counted(kq, k, reads, hint=1 << 20)
    seed_seq = genome[:12000] + b"N" + genome[13000:26000]
    want = R.seed(table, [seed_seq], k)
    assert len(want) >= 20000
    added = R.traversal(table, want, k, 3)
    assert added > 1000
    R.trim(want, k, 0)
    return k, db, seed_seq, R.entries_of(want), added


def run_wide(kq, wide_case):
    k, db, seed_seq, _, added = wide_case
    sub = new_sub(kq, k)
    db.subgraph_seed(sub, seed_seq)
    assert db.subgraph_expand(sub, 3) == added
    sub.subgraph_trim(0)
    return sub.export()


def test_traversal_wide_frontier(kq, wide_case):
    assert H.entries_equal(run_wide(kq, wide_case), wide_case[3])


def test_determinism(kq, wide_case):
    a, b = run_wide(kq, wide_case), run_wide(kq, wide_case)
    assert a.tobytes() == b.tobytes()


def test_convenience_method(kq, bubble_case):
    k, db, table, seed_seq = bubble_case
    sub = db.subgraph(seed_seq, 4)
    want = R.subgraph(table, [seed_seq], k, 4, "traversal")
    assert same(sub, want)
    with pytest.raises(ValueError):
        db.subgraph(seed_seq, 4, algorithm="best-first")


# ------------------------------------------------------------------------------------------------------------------ trim
@pytest.fixture(scope="module")
def trim_case(kq):
    """a seed whose k-mer at position 9 has forward edges of count 1, 2 and 3 that leave the subgraph, one of count 4
    that stays inside, and whose last k-mer has one of count 4 that leaves"""
    k = 21
    rng = np.random.default_rng(42)
    core = rand_bases(rng, 60)
    others = [b for b in b"ACGT" if b != core[30]]
    reads = [core] * 4
    for copies, b in zip((1, 2, 3), others):
        reads += [core[5:30] + bytes([b])] * copies
    bg, _ = H.synth_reads(100, 100, 500, seed=3, err=0.0)
    db, table = counted(kq, k, b"\n".join(reads) + b"\n" + bg)
    return k, db, table, core[:40]


@pytest.mark.parametrize("cutoff", [0, 2])
def test_trim(kq, trim_case, cutoff):
    k, db, table, seed_seq = trim_case
    sub = new_sub(kq, k)
    db.subgraph_seed(sub, seed_seq)
    want = R.seed(table, [seed_seq], k)
    before = {key: (list(v[0]), list(v[1]), v[2]) for key, v in want.items()}
    outside = sorted(c for key, (f, b, _) in before.items() for fw, cs in ((True, f), (False, b)) for i, c in enumerate(cs)
                     if c and R.next_key(key, i, fw, k)[0] not in before)
    assert outside == [1, 2, 3, 4]
    sub.subgraph_trim(cutoff)
    R.trim(want, k, cutoff)
    left = sorted(c for key, (f, b, _) in want.items() for fw, cs in ((True, f), (False, b)) for i, c in enumerate(cs)
                  if c and R.next_key(key, i, fw, k)[0] not in want)
    assert left == ([] if cutoff == 0 else [1, 2])                       # counts <= cutoff stay, counts > cutoff go
    for key, (f, b, _) in before.items():                                # edges that lead inside are never touched
        for fw, cs in ((True, f), (False, b)):
            for i, c in enumerate(cs):
                if c and R.next_key(key, i, fw, k)[0] in before:
                    assert want[key][0 if fw else 1][i] == c
    assert same(sub, want)
    assert sub.summary() == R.summary(want, k)


# -------------------------------------------------------------------------------------------------------------- refusals
def code_of(kq, call):
    with pytest.raises(kq.KqError) as e:
        call()
    return e.value.code


def test_refusals(kq, bubble_case):
    k, db, table, seed_seq = bubble_case
    INVALID, MISMATCH = -1, -7
    sub = new_sub(kq, k)
    windowed = new_sub(kq, k)
    windowed.set_option("bucket_window", 0 | (128 << 16))
    shard = new_sub(kq, k)
    shard.set_option("shard_window", 64 | (128 << 16))
    other_k = kq.KreeqDB(k - 2, MAPS, 0, capacity_hint=1 << 12)
    other_maps = kq.KreeqDB(k, 64, 0, capacity_hint=1 << 12)
    assert code_of(kq, lambda: db.subgraph_seed(windowed, seed_seq)) == INVALID
    assert code_of(kq, lambda: windowed.subgraph_seed(sub, seed_seq)) == INVALID
    assert code_of(kq, lambda: db.subgraph_expand(shard, 1)) == INVALID
    assert code_of(kq, lambda: windowed.subgraph_trim(0)) == INVALID
    assert code_of(kq, lambda: db.subgraph_seed(other_k, seed_seq)) == MISMATCH
    assert code_of(kq, lambda: db.subgraph_expand(other_maps, 1)) == MISMATCH
    assert code_of(kq, lambda: db.subgraph_seed(db, seed_seq)) == INVALID
    assert code_of(kq, lambda: db.subgraph_expand(db, 1)) == INVALID
    assert code_of(kq, lambda: db.subgraph_expand(sub, 256)) == INVALID
    assert code_of(kq, lambda: db.subgraph_expand(sub, -1)) == INVALID
    lib = kq.load()
    assert lib.kq_subgraph_seed(None, sub.handle, None, 0, 0) == INVALID
    assert lib.kq_subgraph_seed(db.handle, sub.handle, None, 5, 0) == INVALID
    assert lib.kq_subgraph_seed(db.handle, sub.handle, None, 0, 2) == INVALID      # unknown flag bit
    assert lib.kq_subgraph_expand(db.handle, sub.handle, 1, None) == INVALID
    assert lib.kq_subgraph_trim(None, 0) == INVALID
    # both handles are as they were, and work
    assert R.table_of(db.export()) == table
    assert len(sub.export()) == 0 and len(windowed.export()) == 0
    db.subgraph_seed(sub, seed_seq)
    want = R.seed(table, [seed_seq], k)
    assert same(sub, want)
    windowed.set_option("bucket_window", 0 | (256 << 16))                # an ordinary table again
    db.subgraph_seed(windowed, seed_seq)
    assert same(windowed, want)
