"""kq_subgraph_best_first through the C ABI (ctypes binding) against `best_first` of tests/subgraph_ref.py (itself pinned by the
reference's goldens in tests/test_subgraph_ref.py).  Every comparison is exact: the count of k-mers added, the whole exported
table entry by entry, the summary, and the export after the trim.  Inputs and the numbers the restatement gives on them:
tests/bestfirst_cases.py."""
import pytest

from tests import bestfirst_cases as B
from tests import helpers as H
from tests import subgraph_ref as R
from tests.test_gpu_subgraph import bubble_genome

pytestmark = pytest.mark.gpu

MAPS = 128


@pytest.fixture(scope="module")
def kq():
    from kreeq_amd import capi
    assert capi.device_available()
    return capi


def counted(kq, k, reads, hint=1 << 16):
    db = kq.KreeqDB(k, MAPS, 0, capacity_hint=hint)
    db.count_batch(reads)
    return db, R.table_of(db.export())


def new_sub(kq, k, hint=1 << 12):
    return kq.KreeqDB(k, MAPS, 0, capacity_hint=hint)


def same(sub_handle, want_table):
    return H.entries_equal(sub_handle.export(), R.entries_of(want_table))


def check(kq, db, table, k, seed_seq, depth, cutoff):
    """seed + best-first + trim on the device and in the restatement -> (k-mers added, the subgraph handle)"""
    sub = new_sub(kq, k)
    db.subgraph_seed(sub, seed_seq)
    want = R.seed(table, [seed_seq], k)
    want_added = R.best_first(table, want, k, depth, cutoff)
    assert db.subgraph_best_first(sub, depth, cutoff) == want_added
    assert same(sub, want)
    assert sub.summary() == R.summary(want, k)
    sub.subgraph_trim(cutoff)
    assert same(sub, R.subgraph(table, [seed_seq], k, depth, "best-first", cov_cutoff=cutoff))
    return want_added, sub


# ------------------------------------------------------------------------------------------------------------ dense graphs
@pytest.fixture(scope="module", params=[4, 5])
def dense_case(request, kq):
    k = request.param
    g, seed_seq = B.dense(k)
    db, table = counted(kq, k, g)
    return k, db, table, seed_seq


@pytest.mark.parametrize("cutoff", B.DENSE_CUTOFFS)
def test_dense_graphs(kq, dense_case, cutoff):
    """consolidation links several degrees; depth 255: the state block at its limit"""
    k, db, table, seed_seq = dense_case
    added = {depth: check(kq, db, table, k, seed_seq, depth, cutoff)[0] for depth in B.dense_depths(k)}
    if cutoff == 0:
        assert added == B.DENSE_ADDED[k]


# ------------------------------------------------------------------------------------------------------------------ bubble
@pytest.fixture(scope="module")
def bubble_case(kq):
    k = 21
    reads, seed_seq = bubble_genome(k)
    db, table = counted(kq, k, reads)
    assert len(R.seed(table, [seed_seq], k)) == B.BUBBLE_SEEDS
    return k, db, table, seed_seq


@pytest.mark.parametrize("cutoff", [0, 2])
def test_bubble(kq, bubble_case, cutoff):
    k, db, table, seed_seq = bubble_case
    for depth in B.BUBBLE_DEPTHS:
        added, _ = check(kq, db, table, k, seed_seq, depth, cutoff)
        if (depth, cutoff) in B.BUBBLE_ADDED:
            assert added == B.BUBBLE_ADDED[(depth, cutoff)]


def test_depth_0_empty_sub_and_second_call(kq, bubble_case):
    k, db, table, seed_seq = bubble_case
    sub = new_sub(kq, k)
    assert db.subgraph_best_first(sub, 21) == 0                          # an empty subgraph
    assert len(sub.export()) == 0
    db.subgraph_seed(sub, seed_seq)
    want = R.seed(table, [seed_seq], k)
    assert db.subgraph_best_first(sub, 0) == 0 and same(sub, want)       # depth 0
    first = R.best_first(table, want, k, 21)
    assert first == B.BUBBLE_ADDED[(21, 0)] and db.subgraph_best_first(sub, 21) == first
    assert same(sub, want)
    second = R.best_first(table, want, k, 255, 2)                        # the result is the seed set of a second call
    assert second == 163
    assert db.subgraph_best_first(sub, 255, 2) == second
    assert same(sub, want)


def test_batches_of_one_search(kq, bubble_case):
    k, db, table, seed_seq = bubble_case
    db.set_option("subgraph_batch", 1)
    try:
        added, one = check(kq, db, table, k, seed_seq, 21, 0)
    finally:
        db.set_option("subgraph_batch", 0)
    assert added == B.BUBBLE_ADDED[(21, 0)]
    assert one.export().tobytes() == check(kq, db, table, k, seed_seq, 21, 0)[1].export().tobytes()


# ------------------------------------------------------------------------------------------------------- saturated dist, k = 31
@pytest.mark.parametrize("s", [1, 3])
def test_saturated_dist(kq, s):
    """a linear path of more than 254 k-mers between two seeds: dist saturates, one node has no prev"""
    k, got = 21, []
    for gap in B.SATURATED_GAPS:
        genome, seed_seq = B.saturated(s, gap)
        db, table = counted(kq, k, genome, hint=1 << 12)
        got.append(check(kq, db, table, k, seed_seq, 255, 0)[0])
    assert got == B.SATURATED_ADDED[s]


def test_k31(kq):
    k = 31
    reads, seed_seq = B.two_stretches(k, seed=31)
    db, table = counted(kq, k, reads)
    assert check(kq, db, table, k, seed_seq, 31, 0)[0] > 0


# ------------------------------------------------------------------------------------------------------------------- high copy
def test_high_copy_on_the_search_path(kq):
    """every counter on the path is 320 and the cutoff 300: the path is followed only if counters come from the logical
    entry (8-bit tier + high-copy tier).  The two seeds are 39 k-mers apart, so depth 21 cannot join them (the restatement
    adds nothing, and neither may the device); depth 40 adds the 38 interior k-mers."""
    k = 21
    reads, seed_seq = B.high_copy_path(k)
    db, table = counted(kq, k, reads)
    assert min(v[2] for v in table.values()) >= 255 and len(table) == 40
    assert check(kq, db, table, k, seed_seq, 21, 300)[0] == 0
    assert check(kq, db, table, k, seed_seq, 40, 300)[0] == 38
    assert check(kq, db, table, k, seed_seq, 40, 320)[0] == 0             # counters == cutoff are not followed


# ------------------------------------------------------------------------------------------------------------------------ wide
@pytest.fixture(scope="module")
def wide_case(kq):
    """24 960 seed k-mers of the wide case of tests/test_gpu_subgraph.py: many workgroups, many batches"""
    k = 21
    reads, genome = H.synth_reads(3000, 150, 30000, seed=77, err=0.01, n_rate=0.0005)
    db, table = counted(kq, k, reads, hint=1 << 20)
    seed_seq = genome[:12000] + b"N" + genome[13000:26000]
    seeds = R.seed(table, [seed_seq], k)
    assert len(seeds) == 24960
    want = {key: (list(v[0]), list(v[1]), v[2]) for key, v in seeds.items()}
    added = R.best_first(table, want, k, 21, 0)
    assert added == 33789
    summary = R.summary(want, k)
    before = R.entries_of(want)
    R.trim(want, k, 0)
    return k, db, table, seed_seq, seeds, added, before, summary, R.entries_of(want)


def run_wide(kq, wide_case, batch):
    k, db, _, seed_seq, _, added, before, summary, after = wide_case
    sub = new_sub(kq, k, hint=1 << 16)
    db.subgraph_seed(sub, seed_seq)
    db.set_option("subgraph_batch", batch)
    try:
        assert db.subgraph_best_first(sub, 21, 0) == added
    finally:
        db.set_option("subgraph_batch", 0)
    assert H.entries_equal(sub.export(), before)
    assert sub.summary() == summary
    sub.subgraph_trim(0)
    out = sub.export()
    assert H.entries_equal(out, after)
    return out.tobytes()


@pytest.fixture(scope="module")
def wide_auto(kq, wide_case):
    return run_wide(kq, wide_case, 0)


@pytest.mark.parametrize("batch", [7, 64, 1000, 0])
def test_wide_batch_sizes(kq, wide_case, wide_auto, batch):
    """3566 batches of 7 (the found list and the visited set grow between batches), 390 of 64, a remainder batch behind 24 of
    1000, and the automatic size a second time: byte-identical exports"""
    assert run_wide(kq, wide_case, batch) == wide_auto


def test_wide_cutoff_1(kq, wide_case):
    k, db, table, seed_seq, seeds = wide_case[:5]
    want = {key: (list(v[0]), list(v[1]), v[2]) for key, v in seeds.items()}
    added = R.best_first(table, want, k, 21, 1)
    assert added == 546
    sub = new_sub(kq, k, hint=1 << 16)
    db.subgraph_seed(sub, seed_seq)
    assert db.subgraph_best_first(sub, 21, 1) == added
    assert same(sub, want)
    sub.subgraph_trim(1)
    R.trim(want, k, 1)
    assert same(sub, want)


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(kq, bubble_case):
    k, db, table, seed_seq = bubble_case
    INVALID, MISMATCH = -1, -7
    sub = new_sub(kq, k)
    db.subgraph_seed(sub, seed_seq)
    want = R.seed(table, [seed_seq], k)
    other_k = kq.KreeqDB(k - 2, MAPS, 0, capacity_hint=1 << 12)
    windowed = new_sub(kq, k)
    windowed.set_option("bucket_window", 0 | (128 << 16))

    def code_of(call):
        with pytest.raises(kq.KqError) as e:
            call()
        return e.value.code

    assert code_of(lambda: db.subgraph_best_first(sub, -1)) == INVALID
    assert code_of(lambda: db.subgraph_best_first(sub, 256)) == INVALID
    assert code_of(lambda: db.subgraph_best_first(db, 5)) == INVALID
    assert code_of(lambda: db.subgraph_best_first(windowed, 5)) == INVALID
    assert code_of(lambda: db.subgraph_best_first(other_k, 5)) == MISMATCH
    assert code_of(lambda: db.set_option("subgraph_batch", -1)) == INVALID
    lib = kq.load()
    assert lib.kq_subgraph_best_first(db.handle, sub.handle, 5, 0, None) == INVALID
    assert lib.kq_subgraph_best_first(None, sub.handle, 5, 0, None) == INVALID
    # both handles are as they were, and a correct call works
    assert R.table_of(db.export()) == table and same(sub, want)
    assert db.subgraph_best_first(sub, 21) == R.best_first(table, want, k, 21) == B.BUBBLE_ADDED[(21, 0)]
    assert same(sub, want)
