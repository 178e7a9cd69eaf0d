"""kq_subgraph_seed / _expand / _best_first / _trim at every k from 2 to 32 against the restatement tests/subgraph_ref.py, on the
inputs of tests/subgraph_inputs.py (tests/test_subgraph_inputs.py holds them to their design: k = 32 keys >= 2^63, both sides of
the hash forms at k = 24 / 25 and 28 / 29, a low-tier entry that crosses 254 inside the subgraph, a high-copy one that comes in
by expansion, counters on both sides of every cutoff used).  Every comparison is exact: the whole export entry by entry,
n_added and summary() after every step.

Table classes: S = the hints of the other subgraph tests (database 2^16, subgraph 2^12: 256 regions at k >= 29, where the slot's
hash is rebuilt from region / rps with rps = 1); B, for k = 21, 29, 31 and 32 = both handles at hint 5 000 000: >= 2048 regions,
rps >= 8.  Saturation at 2^32 - 1: k = 21 and 31."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import subgraph_inputs as G
from tests import subgraph_ref as R

pytestmark = pytest.mark.gpu

MAPS = 128
REGION_SLOTS = 2048
HINTS = {"S": (1 << 16, 1 << 12), "B": (5_000_000, 5_000_000)}
CASES = [(k, "S") for k in range(2, 33)] + [(k, "B") for k in (21, 29, 31, 32)]
DEPTHS = (1, 3)
TRIM_CUTOFFS = (0, 2)
BATCHES = (0, 1, 7)                 # subgraph_batch: automatic, one search per batch, 7


@pytest.fixture(scope="module")
def kq():
    from kreeq_amd import capi
    assert capi.device_available()
    return capi


@functools.lru_cache(maxsize=None)
def table_of(k):
    """the database of graph_case(k) by the CPU oracle"""
    from oracle import oracle as O

    cpu = O.OracleDB(k, MAPS)
    cpu.count_batch(G.graph_case(k).reads)
    entries = cpu.export()
    cpu.close()
    return entries, R.table_of(entries)


@functools.lru_cache(maxsize=None)
def want(k, *steps):
    """the restatement after `steps` -> (entries, summary, what the last step returned); steps are ("seed", batch, no_reference),
    ("expand", depth), ("best_first", depth, cutoff), ("trim", cutoff); every prefix is computed once and never changed"""
    table = table_of(k)[1]
    if not steps:
        return {}, None
    sub = G.copy_of(want(k, *steps[:-1])[0])
    op, ret = steps[-1], None
    if op[0] == "seed":                                                  # seeding adds up over calls like over sequences
        assert all(s[0] == "seed" and s[2] == op[2] for s in steps)
        sub = R.seed(table, [s[1] for s in steps], k, op[2])
    elif op[0] == "expand":
        ret = R.traversal(table, sub, k, op[1])
    elif op[0] == "best_first":
        ret = R.best_first(table, sub, k, op[1], op[2])
    else:
        R.trim(sub, k, op[1])
    return sub, ret


@functools.lru_cache(maxsize=None)
def want_entries(k, *steps):
    sub, ret = want(k, *steps)
    return R.entries_of(sub), R.summary(sub, k), ret


@pytest.fixture(scope="module", params=CASES, ids=[f"k{k}-{cls}" for k, cls in CASES])
def case(request, kq):
    k, cls = request.param
    c = G.graph_case(k)
    db = kq.KreeqDB(k, MAPS, 0, capacity_hint=HINTS[cls][0])
    db.count_batch(c.reads)
    assert H.entries_equal(db.export(), table_of(k)[0])
    if cls == "B":
        assert db.info()["slots_total"] // REGION_SLOTS >= 2048
    yield k, cls, c, db
    db.close()


def new_sub(kq, k, cls):
    sub = kq.KreeqDB(k, MAPS, 0, capacity_hint=HINTS[cls][1])
    if cls == "B":
        assert sub.info()["slots_total"] // REGION_SLOTS >= 2048        # k >= 29: rps = regions / 256 >= 8
    return sub


def same(sub, k, *steps):
    entries, summary, _ = want_entries(k, *steps)
    got = sub.export()
    assert H.entries_equal(got, entries), steps[-1]
    assert sub.summary() == summary, steps[-1]
    return got


@pytest.mark.parametrize("no_reference", [False, True])
def test_seed(kq, case, no_reference):
    k, cls, c, db = case
    sub = new_sub(kq, k, cls)
    steps = (("seed", c.batch, no_reference),)
    db.subgraph_seed(sub, c.batch, no_reference)
    same(sub, k, *steps)
    again = c.batch[:len(c.batch) // 2]                                  # a second call adds up
    steps += (("seed", again, no_reference),)
    db.subgraph_seed(sub, again, no_reference)
    same(sub, k, *steps)
    sub.close()


@pytest.mark.parametrize("cutoff", TRIM_CUTOFFS)
def test_seed_trim(kq, case, cutoff):
    """the trim straight behind the seed: entries that three segments took across 254 lose counters"""
    k, cls, c, db = case
    sub = new_sub(kq, k, cls)
    steps = (("seed", c.batch, False), ("trim", cutoff))
    db.subgraph_seed(sub, c.batch)
    sub.subgraph_trim(cutoff)
    same(sub, k, *steps)
    sub.close()


@pytest.mark.parametrize("cutoff", TRIM_CUTOFFS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_expand_trim(kq, case, depth, cutoff):
    k, cls, c, db = case
    sub = new_sub(kq, k, cls)
    steps = (("seed", c.batch, False),)
    db.subgraph_seed(sub, c.batch)
    same(sub, k, *steps)
    steps += (("expand", depth),)
    assert db.subgraph_expand(sub, depth) == want_entries(k, *steps)[2] > 0
    same(sub, k, *steps)
    steps += (("trim", cutoff),)
    sub.subgraph_trim(cutoff)
    same(sub, k, *steps)
    sub.close()


@pytest.mark.parametrize("which", ["cutoff0", "cutoff_of_case"])
def test_best_first_trim(kq, case, which):
    """depth k; the batch size changes nothing, down to the bytes of the export"""
    k, cls, c, db = case
    cutoff = 0 if which == "cutoff0" else c.cutoff
    exports = []
    for batch in BATCHES:
        sub = new_sub(kq, k, cls)
        steps = (("seed", c.batch, False),)
        db.subgraph_seed(sub, c.batch)
        same(sub, k, *steps)
        steps += (("best_first", k, cutoff),)
        db.set_option("subgraph_batch", batch)
        try:
            added = db.subgraph_best_first(sub, k, cutoff)
        finally:
            db.set_option("subgraph_batch", 0)
        assert added == want_entries(k, *steps)[2] > 0
        before = same(sub, k, *steps)
        steps += (("trim", cutoff),)
        sub.subgraph_trim(cutoff)
        exports.append((before.tobytes(), same(sub, k, *steps).tobytes()))
        sub.close()
    assert exports[1] == exports[0] and exports[2] == exports[0]


# -------------------------------------------------------------------------------------------------------------- saturation
@pytest.fixture(scope="module", params=[21, 31])
def saturated(request, kq):
    """the database of saturation_case(k): reads counted, then one entry with cov and two counters at 2^32 - 6 imported"""
    from kreeq_amd import capi
    from oracle import oracle as O

    k = request.param
    c = G.saturation_case(k)
    cpu = O.OracleDB(k, MAPS)
    cpu.count_batch(c.reads)
    table = R.table_of(cpu.export())
    cpu.close()
    assert c.key not in table
    table[c.key] = (list(c.entry[1]), list(c.entry[2]), c.entry[3])
    db = kq.KreeqDB(k, MAPS, 0, capacity_hint=1 << 16)
    db.count_batch(c.reads)
    entry = np.zeros(1, dtype=capi.ENTRY_DTYPE)
    entry["key"], entry["fw"], entry["bw"], entry["cov"], entry["hc"] = c.key, c.entry[1], c.entry[2], c.entry[3], 1
    db.import_entries(entry)
    assert H.entries_equal(db.export(), R.entries_of(table))
    yield k, c, table, db
    db.close()


def seeded(kq, saturated):
    k, c, table, db = saturated
    sub = kq.KreeqDB(k, MAPS, 0, capacity_hint=1 << 12)
    db.subgraph_seed(sub, c.batch)
    want_sub = R.seed(table, [c.batch], k)
    return sub, want_sub


def same_as(sub, want_sub, k):
    assert H.entries_equal(sub.export(), R.entries_of(want_sub))
    assert sub.summary() == R.summary(want_sub, k)


def test_saturation_seed(kq, saturated):
    """NEAR + NEAR from two segments: exactly 2^32 - 1 in the export, in the lookup and in the summary's total"""
    k, c, table, db = saturated
    sub, want_sub = seeded(kq, saturated)
    f, b, cov = want_sub[c.key]
    assert cov == G.LARGEST and sorted(f + b) == [0] * 5 + [14, G.LARGEST, G.LARGEST]
    same_as(sub, want_sub, k)
    got = sub.lookup_keys([c.key])[0]
    assert got["key"] == c.key and got["fw"].tolist() == f and got["bw"].tolist() == b and got["cov"] == G.LARGEST
    assert sub.summary()["total"] == sum(v[2] for v in want_sub.values()) == G.LARGEST + sum(v[2] for key, v in want_sub.items() if key != c.key)
    sub.close()


@pytest.mark.parametrize("cutoff", [0, G.LARGEST - 1, G.LARGEST])
def test_saturation_best_first_trim(kq, saturated, cutoff):
    """cutoff 2^32 - 2: of the source X only the two saturated counters pass (they are its subgraph entry's; the database has
    2^32 - 6), and the trim clears them; cutoff 2^32 - 1: nothing passes, nothing is cleared"""
    k, c, table, db = saturated
    sub, want_sub = seeded(kq, saturated)
    before = G.n_counters(want_sub)
    assert db.subgraph_best_first(sub, k, cutoff) == R.best_first(table, want_sub, k, k, cutoff) == (19 if cutoff == 0 else 0)
    same_as(sub, want_sub, k)
    sub.subgraph_trim(cutoff)
    R.trim(want_sub, k, cutoff)
    assert cutoff == 0 or before - G.n_counters(want_sub) == (2 if cutoff == G.LARGEST - 1 else 0)
    same_as(sub, want_sub, k)
    got = sub.lookup_keys([c.key])[0]
    assert got["fw"].tolist() == want_sub[c.key][0] and got["bw"].tolist() == want_sub[c.key][1] and got["cov"] == G.LARGEST
    sub.close()
