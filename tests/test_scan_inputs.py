"""The inputs of tests/test_gpu_scan_edges.py have the properties they were built for (tests/scan_inputs.py), by the CPU
oracle alone: these are conditions on the inputs -- a (k, lead) whose seed misses one gets another seed in
scan_inputs.SEED_OVERRIDE, the condition stays."""
import numpy as np
import pytest

from tests import helpers as H
from tests import scan_inputs as S

T = S.T
IDS = [f"k{k}-lead{lead}" for k, lead in S.CASES]


def test_cases_cover_the_issue_grid():
    assert S.K_EDGES == [2, 3, 15, 16, 17, 21, 24, 25, 28, 29, 31, 32] and S.LEADS == [0, 1, 8, 15]
    for k in S.K_EDGES:
        want = list(range(16)) if k in (21, 32) else S.LEADS
        assert [l for kk, l in S.CASES if kk == k] == want
    # over the grid every window length, every rotation of the separator offsets and both kinds of first byte occur
    seeds = [S.seed_for(k, lead) for k, lead in S.CASES]
    assert {s % 7 for s in seeds} == set(range(7)) and {s % 3 for s in seeds} == {0, 1, 2} and {s % 2 for s in seeds} == {0, 1}
    for k in S.K_EDGES:
        ks = [S.seed_for(kk, lead) for kk, lead in S.CASES if kk == k]
        assert {s % 3 for s in ks} == {0, 1, 2} and {s % 2 for s in ks} == {0, 1}, k
    assert {S.seed_for(k, lead) % 7 for k, lead in S.CASES if k in (21, 32)} == set(range(7))


@pytest.mark.parametrize("k,lead", S.CASES, ids=IDS)
def test_edge_text_layout(k, lead):
    """window coordinates: where the separators and runs sit relative to tile and lane edges"""
    seed = S.seed_for(k, lead)
    text, events = S.edge_text(k, lead, seed)
    assert (text, events) == S.edge_text(k, lead, seed)                        # deterministic
    assert len(text) < 40 * 1024 and lead + len(text) == S.N_TILES * T + S.tail_of(k, seed) and lead + len(text) >= 8 * T
    assert S.CODE[text[-1]] < 4 and (S.CODE[text[0]] == 4) == bool(seed % 2)
    is_base = np.array([S.CODE[c] < 4 for c in text])
    seps = {e["at"] + lead for e in events if e["kind"] == "sep"}
    assert seps == set((np.flatnonzero(~is_base) + lead).tolist())              # nothing but the recorded separators
    assert {text[w - lead] for w in seps} == {ord("\n"), ord("N")}
    assert abs(sum(text[w - lead] == ord("N") for w in seps) - len(seps) / 2) <= 1
    # every offset -1, 0, +1 at an odd and at an even tile edge, as a lone separator (edges 1..3) and at a run of k (4..6)
    for edges in ((1, 2, 3), (4, 5, 6), (1, 3, 5), (2, 4, 6)):
        offs = set()
        for s in edges:
            near = [w - s * T for w in seps if abs(w - s * T) <= 1]
            assert len(near) == 1, (s, near)
            offs.add(near[0])
        assert offs == {-1, 0, 1}, edges
    for s in (1, 2, 3):                                                        # long runs on both sides
        (w,) = [w for w in seps if abs(w - s * T) <= 1]
        assert is_base[w - lead - 100:w - lead].all() and is_base[w - lead + 1:w - lead + 100].all()
    runs_k = sorted(e["at"] + lead for e in events if e["kind"] == "run_k")
    runs_k1 = sorted(e["at"] + lead for e in events if e["kind"] == "run_k1")
    ends = {w + k - 1 for w in runs_k}
    assert any(w % T == 0 for w in runs_k), "a run of k that starts at a tile edge"
    assert any(w % T == T - 1 for w in ends), "a run of k that ends in front of a tile edge"
    assert any(w % T == T - 1 for w in runs_k), "one base before the edge"
    assert any(w % T == T - (k - 1) for w in runs_k), "k - 1 bases before the edge"
    assert any(0 < w % T < T - 100 and w % 16 == 0 for w in runs_k) and any(100 < w % T < T - 100 and w % 16 == 15 for w in ends)
    ends1 = {w + k - 2 for w in runs_k1}
    assert any(w // T < (w + k - 2) // T or (k == 2 and w % T == T - 1) for w in runs_k1), "k - 1 bases across a tile edge"
    assert any(100 < w % T < T - 100 and w % 16 == 0 for w in runs_k1) and any(100 < w % T < T - 100 and w % 16 == 15 for w in ends1)
    lower = [i + lead for i, c in enumerate(text) if c >= 0x61]
    assert lower and min(lower) < 2 * T <= max(lower)
    for e in events:
        if e["kind"] in ("run_k", "run_k1"):
            a, n = e["at"], e["n"]
            assert n == (k if e["kind"] == "run_k" else k - 1)
            assert is_base[a:a + n].all() and not is_base[a - 1] and not is_base[a + n], e


@pytest.mark.parametrize("k,lead", S.CASES, ids=IDS)
def test_oracle_records_of_the_text(k, lead):
    r = S.reference(k, lead)
    text = r.text
    # a plain run-length walk: a run of n >= k bases has n - k + 1 k-mers
    count, run = 0, 0
    for c in text + b"\n":
        if S.CODE[c] < 4:
            run += 1
        else:
            count += max(0, run - k + 1)
            run = 0
    assert len(r.keys) == count > 8 * T - 40 * k
    keys, edges = S.walk_records(k, text)
    assert np.array_equal(r.keys, keys) and np.array_equal(r.edges, edges)
    starts = [w[0] for w in S.walk(k, text)]
    index = {s: i for i, s in enumerate(starts)}
    lut = bytes.maketrans(b"ACGTacgt", bytes([0, 1, 2, 3, 0, 1, 2, 3]))
    for e in r.events:
        a, n = e["at"], e["n"]
        if e["kind"] == "run_k":                                              # one k-mer, no neighbour on either side
            key, fw = O_hash(text[a:a + k].translate(lut), k)
            assert a in index and a - 1 not in index and a + 1 not in index, e
            assert r.keys[index[a]] == key and r.edges[index[a]] == 0, e
        elif e["kind"] == "run_k1":
            assert not any(s in index for s in range(a - 1, a + n + 1)), e
        elif e["kind"] == "sep":
            assert not any(s in index for s in range(max(0, a - k + 1), a + 1)), e
            if a - k in index:                                                # the k-mer that ends in front of it: no next
                i = index[a - k]
                key, fw = O_hash(text[a - k:a].translate(lut), k)
                assert r.keys[i] == key and r.edges[i] & (0xF0 if fw else 0x0F) == 0, e
                if a - k - 1 in index:                                        # but a prev
                    assert r.edges[i] & (0x0F if fw else 0xF0) != 0, e
            if a + 1 in index:                                                # the k-mer that starts behind it: no prev
                i = index[a + 1]
                key, fw = O_hash(text[a + 1:a + 1 + k].translate(lut), k)
                assert r.keys[i] == key and r.edges[i] & (0x0F if fw else 0xF0) == 0, e
                if a + 2 in index:
                    assert r.edges[i] & (0xF0 if fw else 0x0F) != 0, e
    # the counted text: every record once
    assert int(r.export["cov"].sum()) == count and r.summary["total"] == count


def O_hash(codes, k):
    from oracle import oracle as O

    return O.hash_kmer(list(codes), k)


@pytest.mark.parametrize("k,lead", S.CASES, ids=IDS)
def test_lookup_inputs(k, lead):
    r = S.reference(k, lead)
    c0, pb0 = r.validate[(0, S.MAP, 0)]
    c3, _ = r.validate[(0, S.MAP, 3)]
    missing, evaluated, edge_missing = (int(x) for x in c0)
    assert missing > 0 and edge_missing > 0 and evaluated > missing
    assert evaluated == len(r.keys)
    assert c0.tolist() != c3.tolist()
    for cut in S.CUTOFFS:                                                     # the half ranges split the work
        lo, hi = r.validate[(0, 64, cut)][0], r.validate[(64, S.MAP, cut)][0]
        assert lo[1] > 0 and (lo + hi).tolist() == r.validate[(0, S.MAP, cut)][0].tolist()
        assert hi[1] > 0 or 4 ** k <= 64                                      # (every key of k <= 3 is below 64)
    assert (pb0["cov"] == 0).any() and (pb0["cov"] > 0).any()
    assert max(pb0["fw"].max(), pb0["bw"].max()) > 254, "an edge count out of the high-copy tier"
    assert r.table["cov"].max() > 254 and (r.table["cov"] < 3).any()
    assert len(r.reads) < 100_000


@pytest.mark.parametrize("k,lead", S.BRANCH_CASES, ids=[f"k{k}-lead{lead}" for k, lead in S.BRANCH_CASES])
def test_branch_scan_inputs(k, lead):
    r = S.reference(k, lead)
    f0, f2, f300 = (H.branch_flags(r.table, k, r.text, c) for c in S.BRANCH_CUTOFFS)
    assert not np.array_equal(f0, f2) and not np.array_equal(f2, f300) and not np.array_equal(f0, f300)
    assert ((f0 & 1) == (f300 & 1)).all() and (f0 & 1).any() and not (f0 & 1).all()
    row = {key: i for i, key in enumerate(r.table["key"].tolist())}
    strand = {w[0]: (w[1], w[2]) for w in S.walk(k, r.text)}
    quirk = lost = lost300 = 0
    for pos in np.flatnonzero(f0 & 2).tolist():
        key, fw = strand[pos]
        e = r.table[row[key]]
        if fw and f300[pos] & 2 and e["fw"].max() <= 300:
            quirk += 1                                      # the cut-off does not apply to the forward strand
        if not fw and not f2[pos] & 2:
            lost += 1
        if not fw and f2[pos] & 2 and not f300[pos] & 2 and e["bw"].max() > 254:
            lost300 += 1                                    # an edge count of the high-copy tier against the cut-off
    assert quirk > 0 and lost > 0 and lost300 > 0
    assert not any(strand[pos][1] for pos in np.flatnonzero((f0 ^ f300) & 2).tolist()), "only the reverse strand has a cut-off"


def test_branch_flags_cutoff_semantics():
    """H.branch_flags on a table written by hand: the cut-off is a strict `>` and applies to the reverse strand only"""
    from oracle import oracle as O

    k = 5
    fwd, rev = b"AACCA", b"TGGTT"                           # forward-strand k-mer; the same k-mer read on the reverse strand
    key, is_fw = O.hash_kmer(list(fwd.translate(bytes.maketrans(b"ACGT", bytes(range(4))))), k)
    assert is_fw and O.hash_kmer(list(rev.translate(bytes.maketrans(b"ACGT", bytes(range(4))))), k) == (key, False)
    e = np.zeros(1, dtype=O.ENTRY_DTYPE)
    e["key"], e["cov"] = key, 10
    e["fw"][0] = [0, 1, 0, 0]                               # fw[C] = 1
    e["bw"][0] = [0, 0, 3, 0]                               # bw[G] = 3: read on the reverse strand it continues with 3 - G = C
    for cut, want_rev in ((0, 3), (2, 3), (3, 1), (300, 1)):
        assert H.branch_flags(e, k, fwd + b"A", cut).tolist()[0] == 3          # fw[C] != 0, the sequence goes on with A
        assert H.branch_flags(e, k, fwd + b"C", cut).tolist()[0] == 1          # the only edge is the sequence's own
        assert H.branch_flags(e, k, rev + b"A", cut).tolist()[0] == want_rev, cut
        assert H.branch_flags(e, k, rev + b"C", cut).tolist()[0] == 1
    assert H.branch_flags(e, k, b"AACGA", 0).tolist() == [0] * 5
