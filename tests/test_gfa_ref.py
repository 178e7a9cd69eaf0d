"""The graph rules of tests/gfa_ref.py against the reference's own goldens (validateFiles/test.36.tst .. test.47.tst): every
line of the "+++Assembly summary+++" block this build prints, and invariants of the graph on every input.  No GPU."""
import pytest

from tests import gfa_cases as GC
from tests import gfa_ref as G
from tests import subgraph_inputs as SI
from tests import subgraph_ref as R
from tests.test_subgraph_ref import K


@pytest.mark.parametrize("idx", GC.SUBGRAPH_TESTS)
def test_block_matches_golden(idx):
    """the gate: all printed lines, in the golden's order; only `# separated components` and `# bubbles` are absent"""
    table, no_collapse, expected = GC.golden_table(idx)
    got = G.block_lines(G.build(table, K, no_collapse))
    want = G.golden_block(expected)
    assert len(want) == len(got) == 42
    assert got == want


def test_goldens_cover_both_modes():
    modes = [GC.golden_table(idx)[1] for idx in GC.SUBGRAPH_TESTS]
    assert modes.count(True) == 4 and modes.count(False) == 8


def check_invariants(table, k):
    """-> (collapsed graph, uncollapsed graph)"""
    rank = {x: r for r, x in enumerate(sorted(table))}
    out = []
    for no_collapse in (False, True):
        g = G.build(table, k, no_collapse)
        strings = G.segment_strings(g)
        assert g.counts["n_segments"] == len(g.segs) and g.counts["n_edges"] == len(g.edges) and g.counts["n_seq"] == len(g.seq)
        seen = []
        for s, seg in zip(strings, g.segs):
            assert len(s) == seg[2] + k - 1
            for i in range(seg[2]):
                key = GC.key_of(s[i:i + k])
                assert key in table                                      # every window is a subgraph k-mer
                seen.append(key)
            assert GC.key_of(s[:k]) == seg[1] and (s[:k] != G.kmer_string(seg[1], k)) == bool(seg[4]) and seg[3] == table[seg[1]][2]
        assert sorted(seen) == sorted(table)                             # every k-mer lies in exactly one segment
        for a, b, c, arc, brc in g.edges:
            sa = G.revcomp(strings[a]) if arc else strings[a]
            sb = G.revcomp(strings[b]) if brc else strings[b]
            assert sa[-(k - 1):] == sb[:k - 1] and c > 0
        if no_collapse:
            assert len(g.edges) == sum(c != 0 and R.next_key(key, i, fw, k)[0] in table for key, (f, b, _) in table.items()
                                       for fw, cs in ((True, f), (False, b)) for i, c in enumerate(cs))
            assert [s[1] for s in g.segs] == sorted(table) and g.counts["n_dropped_edges"] == g.counts["n_cycles"] == 0
        else:
            links = [(a, arc, b, brc) for a, b, _, arc, brc in g.edges]
            mirrored = [(b, 1 - brc, a, 1 - arc) for a, arc, b, brc in links]
            assert len(set(links)) == len(links)                         # no link twice,
            assert all(m == l or m not in links for l, m in zip(links, mirrored))      # and not as its own mirror either
        assert len(rank) == len(table)
        out.append(g)
    return out


@pytest.mark.parametrize("idx", GC.SUBGRAPH_TESTS)
def test_invariants_goldens(idx):
    check_invariants(GC.golden_table(idx)[0], K)


@pytest.mark.parametrize("k", GC.INPUT_KS)
def test_invariants_inputs(k):
    table = GC.input_table(k)
    assert len(table) > 10
    check_invariants(table, k)


@pytest.mark.parametrize("name,k", GC.HAND_IDS)
def test_invariants_hand_cases(name, k):
    table = GC.hand_case(name, k)
    g, nc = check_invariants(table, k)
    c = g.counts
    if name == "pure_cycle":      # one segment of n + k - 1 bases, closed by one link: + -> + or its mirror - -> -, whichever id pair is smaller
        assert c["n_segments"] == 1 and c["n_cycles"] == 1 and len(g.edges) == 1 and g.segs[0][2] == len(table)
        assert g.edges[0][:2] == (0, 0) and g.edges[0][3] == g.edges[0][4]
        assert G.stats(g)["circular"] == 1
    if name == "long_cycle":
        assert c["n_segments"] == 1 and c["n_cycles"] == 1 and g.segs[0][2] == 3000 and len(g.edges) == 1
    if name == "cycle_with_tail":
        assert c["n_cycles"] == 0 and c["n_segments"] == 2 and len(g.edges) == 2
    if name == "long_unitig":
        assert c["n_segments"] == 1 and g.segs[0][2] == 5000 and not g.edges
    if name == "hairpin":                                                # the path folds back on itself: one segment, a link + -> -
        assert c["n_segments"] == 1 and [(e[0], e[1], e[3], e[4]) for e in g.edges] == [(0, 0, 0, 1)] or c["n_segments"] == 1 and [(e[3], e[4]) for e in g.edges] == [(1, 0)]
    if name == "homopolymer":
        assert any(a == b and arc == brc for a, b, _, arc, brc in g.edges)      # the self-loop survives as a link of its own segment
    if name == "palindrome":
        pal = [key for key in table if G.kmer_string(key, k) == G.revcomp(G.kmer_string(key, k))]
        assert pal and all(seg[2] == 1 for seg in g.segs if seg[1] in pal)      # a palindrome takes no link: a segment of its own
    if name == "isolated":
        assert G.stats(g)["disconnected"] >= 1 and c["n_segments"] == 2
    if name == "two_kmer_unitig":
        assert 2 in [seg[2] for seg in g.segs] and c["n_segments"] == 5
    if name == "asymmetric":
        assert c["n_dropped_edges"] == 1
    if name == "trimmed_counter":
        assert c["n_segments"] == 2 and not g.edges and SI.outside_counters(table, k)
    if name == "cov300":
        assert [seg[3] for seg in g.segs] == [300] and "DP:f:300" in G.gfa_text(g)


def test_text_layout():
    g = G.build(GC.hand_case("two_kmer_unitig", 5), 5)
    lines = G.gfa_text(g).split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == ""
    kinds = [l[0] for l in lines[1:-1]]
    assert kinds == ["S"] * len(g.segs) + ["L"] * len(g.edges)           # all segments first, then all links
    assert all(l.split("\t")[5] == "4M" and l.split("\t")[6].startswith("KC:i:") for l in lines[1 + len(g.segs):-1])


def test_empty_graph():
    g = G.build({}, 21)
    assert g.counts == {"n_segments": 0, "n_seq": 0, "n_edges": 0, "n_dropped_edges": 0, "n_cycles": 0}
    assert G.gfa_text(g) == "H\tVN:Z:1.0\n"
    b = G.block_lines(g)
    assert "# segments: 0" in b and "Average segment length: nan" in b and "Average degree: nan" in b
