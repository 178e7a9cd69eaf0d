"""tests/fuzz_inputs.py held to its design, without a GPU: every expected value of the fuzz chain comes from the oracle and the
restatements alone, for the whole seed list, and the list must reach what the chain is there to compare -- variant paths at
every k, paths that the second counter tier decides, key 0, windows with repeated keys, cutoffs that matter, cycles, dropped
edges, palindromes.  These are conditions on the inputs: when one fails the generator is tuned, never the condition."""
import time

import pytest

from oracle import variants as V
from tests import fuzz_inputs as F
from tests import gfa_ref as G
from tests import variant_cases as C


def row_of(seed):
    t0 = time.perf_counter()
    e = F.expected(seed)
    seconds = time.perf_counter() - t0
    c, k = e.case, e.case.k
    hot = bool((e.entries["cov"] > F.HIGH).any())
    row = dict(seed=seed, k=k, flavour=c.flavour, seconds=seconds, n_entries=len(e.entries), n_paths=len(e.paths),
               types={p[2] for p in e.paths}, hot=hot, key0=bool(len(e.entries)) and int(e.entries["key"][0]) == 0,
               counts=e.gfa[False].counts, n_sub=len(e.sub_trimmed), n_added=e.n_added,
               palindrome=k % 2 == 0 and any(G._palindrome(key, k) for key in e.sub_trimmed))
    row["tier_decides"] = row["clamp_decides"] = row["cutoff_decides"] = False
    if hot and e.paths:
        args = (c.asm, c.var_depth, c.var_span, c.var_cutoff)
        row["tier_decides"] = F.variant_paths(F.graph_of_entries(F.first_tier_only(e.entries), k), *args) != e.paths
        row["clamp_decides"] = F.variant_paths(F.graph_of_entries(F.clamped(e.entries), k), *args) != e.paths
    if c.var_cutoff:
        row["cutoff_decides"] = F.variant_paths(e.graph, c.asm, c.var_depth, c.var_span, 0) != e.paths
    stats = [C.window_stats(k, seg, c.var_span) for _, seg in V.segments_of(c.asm.decode("latin-1")) if len(seg) >= k]
    row["twice"], row["erased"] = sum(s[0] for s in stats), sum(s[1] for s in stats)
    return row


@pytest.fixture(scope="module")
def rows():
    out = [row_of(seed) for seed in F.SEEDS]
    for r in out:
        print({f: v for f, v in r.items() if f != "types"}, sorted(r["types"]))
    return out


def seeds_with(rows, cond):
    return [r["seed"] for r in rows if cond(r)]


def test_seed_list():
    assert len(F.SEEDS) == 124
    for k in range(2, 33):
        assert sum(F.k_of(s) == k for s in F.SEEDS) == 4
    assert 8 * sum(F.is_circular(s) for s in F.SEEDS) >= len(F.SEEDS)
    for seed in (0, 3, 77):                                              # a pure function of the seed
        a, b = F.case(seed), F.case(seed)
        assert vars(a) == vars(b)
    for seed in F.SEEDS:
        c = F.case(seed)
        assert c.k == F.k_of(seed) and len(c.asm) < 500 and 1 <= len(c.edits) <= 5
        assert c.sub_depth <= min(c.k, 8) and c.copies in (1, 3, 130, 300)


def test_references_are_total_and_cheap(rows):
    """no restatement raised (the fixture would have failed), no table is empty, the whole list costs less than two minutes"""
    assert len(rows) == len(F.SEEDS)
    assert all(r["n_entries"] > 0 for r in rows)
    total = sum(r["seconds"] for r in rows)
    print("references: %.1f s in all, slowest seed %.2f s" % (total, max(r["seconds"] for r in rows)))
    assert total < 120


def test_every_k_has_a_variant_path(rows):
    for k in range(2, 33):
        assert seeds_with(rows, lambda r: r["k"] == k and r["n_paths"] > 0), k


def test_every_k_has_a_branching_subgraph(rows):
    for k in range(2, 33):
        assert seeds_with(rows, lambda r: r["k"] == k and r["counts"]["n_segments"] >= 2 and r["counts"]["n_edges"] >= 1), k


def test_variant_paths_are_common(rows):
    assert 3 * len(seeds_with(rows, lambda r: r["n_paths"] > 0)) >= len(rows)
    types = set().union(*(r["types"] for r in rows))
    assert types == {0, 1, 2, 3}


def test_second_tier_decides_paths(rows):
    """Paths on tables with entries above 254, and at least five path sets that change when the high-copy entries are read
    as the first tier holds them (a tombstone: cov 255, no edge counters).  Cutting their counters down to 254 instead can
    change no path here and never will: the search tests an edge counter with `!= 0` and with `> cov_cutoff`
    (oracle/variants.py:255), the cutoffs of the list are at most 5, and a counter of a high-copy entry that is clamped was
    above 254 before.  clamp_decides is computed all the same and must stay empty; what a kernel that ignored the second
    tier would read is the tombstone."""
    assert 8 * len(seeds_with(rows, lambda r: r["hot"] and r["n_paths"] > 0)) >= len(rows)
    assert len(seeds_with(rows, lambda r: r["tier_decides"])) >= 5
    assert not seeds_with(rows, lambda r: r["clamp_decides"])


def test_key_zero_with_paths(rows):
    assert len(seeds_with(rows, lambda r: r["key0"] and r["n_paths"] > 0)) >= 5


def test_graph_shapes(rows):
    assert len(seeds_with(rows, lambda r: r["counts"]["n_cycles"] > 0)) >= 5
    assert len(seeds_with(rows, lambda r: r["counts"]["n_dropped_edges"] > 0)) >= 10
    assert len(seeds_with(rows, lambda r: r["palindrome"])) >= 5


def test_windows_with_repeated_keys(rows):
    assert len(seeds_with(rows, lambda r: r["twice"] > 0 and r["erased"] > 0)) >= 5


def test_cutoff_decides_paths(rows):
    assert len(seeds_with(rows, lambda r: r["cutoff_decides"])) >= 10
