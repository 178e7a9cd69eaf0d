"""The inputs of tests/subgraph_inputs.py held to their design, from the restatement tests/subgraph_ref.py alone (CPU oracle for the
database table), so that no case of tests/test_gpu_subgraph_kmatrix.py can pass vacuously; and subgraph_ref.next_key against a
construction on strings at the k where the key arithmetic changes form."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import subgraph_inputs as G
from tests import subgraph_ref as R

MAPS = 128
ALL_K = list(range(2, 33))


@functools.lru_cache(maxsize=None)
def table_of(k):
    from oracle import oracle as O

    cpu = O.OracleDB(k, MAPS)
    cpu.count_batch(G.graph_case(k).reads)
    table = R.table_of(cpu.export())
    cpu.close()
    return table


@functools.lru_cache(maxsize=None)
def seeds_of(k):
    return R.seed(table_of(k), [G.graph_case(k).batch], k)


constructed = G.constructed


def test_every_k_has_a_case():
    assert ALL_K == list(range(2, 33))
    for k in ALL_K:
        c = G.graph_case(k)
        assert c.k == k and len(c.batch) < 1000 and c is G.graph_case(k)
        assert len(c.reads) < (1 << 20)


@pytest.mark.parametrize("k", ALL_K)
def test_seed_design(k):
    c, table, seeds = G.graph_case(k), table_of(k), seeds_of(k)
    segs = R.segments_of(c.batch)
    assert len(segs) >= 4
    if k >= 8:
        assert any(len(s) == k for s in segs) and any(len(s) == k - 1 for s in segs)
    assert any(key in table for key in seeds) and any(key not in table for key in seeds)          # both sources of a seed entry
    assert len(R.seed(table, [c.batch], k, no_reference=True)) < len(seeds)
    assert any(key not in seeds for key in table)                                                 # part of the graph stays outside
    # a low-tier database entry that the sums over three segments take across 254 inside the subgraph
    assert any(key in table and table[key][2] <= 254 < v[2] for key, v in seeds.items())
    absent = G.key_of(c.w)
    assert absent not in table and absent in seeds
    if k >= 8:
        assert any(key in table and table[key][2] == G.CENTURY and v[2] == 3 * G.CENTURY for key, v in seeds.items())
        # the reverse-complement repeats: both occurrences of A w C ... G rc(w) T construct the same edges, those of
        # C w2 A ... C rc(w2) A differ, and the first occurrence decides
        for w, (p1, n1), (p2, n2), differ in ((c.w, b"AC", b"GT", False), (c.w2, b"CA", b"CA", True)):
            key, f, b = constructed(bytes([p1]), w, bytes([n1]))
            assert key not in table and seeds[key] == (f, b, 1)
            assert constructed(bytes([p2]), H.revcomp_bases(w), bytes([n2]))[0] == key
            assert (constructed(bytes([p2]), H.revcomp_bases(w), bytes([n2])) != (key, f, b)) == differ
        if k % 2 == 0:
            pal = G.key_of(c.pal)
            assert pal in seeds and pal in table
    if k == 32:
        assert any(key >= 1 << 63 for key in seeds)
    # a trim straight behind the seed clears a counter of such an entry (its 8-bit lane and its high-copy counter)
    for cutoff in (0, 2):
        sub = G.copy_of(seeds)
        R.trim(sub, k, cutoff)
        assert G.crossed_and_trimmed(table, seeds, sub)
        assert G.n_counters(sub) < G.n_counters(seeds)


@pytest.mark.parametrize("k", ALL_K)
def test_traversal_design(k):
    c, table = G.graph_case(k), table_of(k)
    added, subs = {}, {}
    for depth in (1, 3):
        subs[depth] = G.copy_of(seeds_of(k))
        added[depth] = R.traversal(table, subs[depth], k, depth)
    assert added[1] > 0 and added[3] > 0
    if k >= 8:
        assert added[3] > added[1]
    hot = G.key_of(c.hot)
    assert hot not in seeds_of(k) and subs[1][hot][2] >= 255                   # a high-copy entry that comes in by expansion
    if k == 32:
        assert any(key >= 1 << 63 for key in subs[1] if key not in seeds_of(k))
    # trim after either depth, at both cutoffs: it removes counters; at cutoff 2, counters <= 2 that point outside stay (at
    # cutoff 0 none can: every counter that points outside is > 0).  k = 2 and 3: three rounds reach the whole key space, and
    # nothing points outside
    for depth in (1, 3):
        for cutoff in (0, 2):
            sub = G.copy_of(subs[depth])
            before, out_before = G.n_counters(sub), G.outside_counters(sub, k)
            if k < 4 and depth == 3:
                assert not out_before and len(sub) == len(table) + 1
                continue
            R.trim(sub, k, cutoff)
            left = G.outside_counters(sub, k)
            assert G.n_counters(sub) == before - sum(x > cutoff for x in out_before) < before
            assert left == [x for x in out_before if x <= cutoff]
            if cutoff == 2:
                assert len(left) >= 1
            assert G.n_counters(sub) > 0


@pytest.mark.parametrize("k", ALL_K)
def test_best_first_design(k):
    c, table = G.graph_case(k), table_of(k)
    full = G.copy_of(seeds_of(k))
    n_full = R.best_first(table, full, k, k, 0)
    assert n_full > 0                                                          # k = 2, 3: by the choice of SMALL_K
    cut = G.copy_of(seeds_of(k))
    n_cut = R.best_first(table, cut, k, k, c.cutoff)
    assert 0 < n_cut < n_full
    assert any(v[2] >= 255 for key, v in full.items() if key not in seeds_of(k))
    if k == 32:
        assert any(key >= 1 << 63 for key in full if key not in seeds_of(k))
    for sub, cutoff in ((full, 0), (cut, c.cutoff)):
        before, out_before, untrimmed = G.n_counters(sub), G.outside_counters(sub, k), G.copy_of(sub)
        R.trim(sub, k, cutoff)
        assert G.n_counters(sub) < before and any(x > cutoff for x in out_before)
        assert k < 8 or G.crossed_and_trimmed(table, untrimmed, sub)
        if cutoff:
            assert len(G.outside_counters(sub, k)) >= 1


# -------------------------------------------------------------------------------------------------------------- saturation
def saturation_table(k):
    """the database of saturation_case(k) as the restatement sees it: the reads counted, then the entry imported"""
    from oracle import oracle as O

    c = G.saturation_case(k)
    cpu = O.OracleDB(k, MAPS)
    cpu.count_batch(c.reads)
    table = R.table_of(cpu.export())
    cpu.close()
    assert c.key not in table
    table[c.key] = (list(c.entry[1]), list(c.entry[2]), c.entry[3])
    return c, table


@pytest.mark.parametrize("k", [21, 31])
def test_saturation_design(k):
    c, table = saturation_table(k)
    assert sorted(c.entry[1] + c.entry[2]) == [0] * 5 + [7, G.NEAR, G.NEAR] and len(c.along) == 2
    seeds = R.seed(table, [c.batch], k)
    f, b, cov = seeds[c.key]
    assert cov == G.LARGEST and sorted(f + b) == [0] * 5 + [14, G.LARGEST, G.LARGEST]
    assert all((f if fw else b)[i] == G.LARGEST for fw, i in c.along)
    added = {}
    for cutoff in (0, G.LARGEST - 1, G.LARGEST):
        sub = G.copy_of(seeds)
        added[cutoff] = R.best_first(table, sub, k, k, cutoff)
        before = G.n_counters(sub)
        R.trim(sub, k, cutoff)
        if cutoff == G.LARGEST - 1:                                           # the two saturated counters, and nothing else
            assert G.n_counters(sub) == before - 2 and sorted(sub[c.key][0] + sub[c.key][1]) == [0] * 7 + [14]
        if cutoff == G.LARGEST:
            assert G.n_counters(sub) == before
    # the 6 + 6 k-mers between X and the two ends of S and the 7 of the branch; no counter of the database passes the other
    # two cutoffs, so the two edges the first of them follows from X end at once
    assert added == {0: 19, G.LARGEST - 1: 0, G.LARGEST: 0}


# ----------------------------------------------------------------------------------------------- the repeat across a tile edge
@pytest.mark.parametrize("k", [21, 32])
@pytest.mark.parametrize("lead", [0, 1, 8, 15])
def test_tile_repeat_text(k, lead):
    text, plants = G.tile_repeat_text(k, lead)
    assert len(R.segments_of(text)) == 1 and len(plants) == 2
    seeds = R.seed({}, [text], k)
    for s, (w, a, b, at) in zip((1, 2), plants):
        first, second = lead + at, lead + at + G.PERIOD                       # window positions
        assert s * G.TILE - 16 <= first < s * G.TILE <= second < s * G.TILE + 16
        one = constructed(a, w, text[at + k:at + k + 1])
        two = constructed(text[at + G.PERIOD - 1:at + G.PERIOD], w, b)
        assert one[0] == two[0] and one[1:] != two[1:] and sum(one[1]) == sum(one[2]) == 1
        assert seeds[one[0]] == (one[1], one[2], 1)


# ---------------------------------------------------------------------------------------------------------------- next_key
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def string_next(key, base, fw, k):
    """the neighbour of the canonical string of `key`, built on strings.  Keys hold the first base in the low bits, so the order
    of the keys is the order of the REVERSED strings: that is the comparison taken here"""
    s = H.ACGT[[(key >> (2 * i)) & 3 for i in range(k)]].tobytes()
    nxt = s[1:] + b"ACGT"[base:base + 1] if fw else b"ACGT"[base:base + 1] + s[:-1]
    rc = nxt.translate(COMP)[::-1]
    is_fw = nxt[::-1] < rc[::-1]
    return H.key_of_codes([b"ACGT".index(x) for x in (nxt if is_fw else rc)]), is_fw


@pytest.mark.parametrize("k", [2, 3, 16, 24, 25, 28, 29, 31, 32])
def test_next_key_on_strings(k):
    rng = np.random.default_rng(k)
    keys = [int(x) for x in H.canonical_keys_of(rng.integers(0, 1 << 63, 300, dtype=np.uint64) >> np.uint64(max(0, 63 - 2 * k)), k)]
    if k == 32:
        keys += [int(x) for x in H.canonical_keys_of(rng.integers(0, 1 << 63, 100, dtype=np.uint64) * np.uint64(2) + np.uint64(1), k)]
    pals = set()
    if k % 2 == 0:                                                             # palindromes, and k-mers one step in front of one
        for p in H.palindromes(k, 20, seed=k):
            pk = H.key_of_codes([b"ACGT".index(x) for x in p])
            pals.add(pk)
            keys += [pk, int(H.canonical_keys_of([H.key_of_codes([b"ACGT".index(x) for x in b"A" + p[:-1]])], k)[0])]
    keys += [0, H.max_canonical_key(k)]
    n_pal = n_rev = n_top = 0
    for key in keys:
        assert key < 4 ** k
        for fw in (True, False):
            for base in range(4):
                got = R.next_key(key, base, fw, k)
                assert got == string_next(key, base, fw, k), (key, base, fw)
                n_rev += not got[1]
                n_pal += got[0] in pals
                n_top += got[0] >= 1 << 63
    assert n_rev > 0 and (k % 2 or n_pal > 0) and (k < 32 or n_top > 0)
