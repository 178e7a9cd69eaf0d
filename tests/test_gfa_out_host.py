"""kreeq_amd/host/gfa_out.h (GFA text, the block's numbers and its printer) as a stand-alone host program under
-fsanitize=address,undefined (tests/native/gfa_out_main.cpp), against the Python output of tests/gfa_ref.py: hand-written arrays
(the empty graph, one isolated segment, a cycle, two components, a hairpin link and a segment reached from both sides), the
arrays of goldens 38 and 43, records that point outside their arrays.  No GPU."""
import os
import shutil
import subprocess
import types

import pytest

from tests import gfa_cases as GC
from tests import gfa_ref as G
from tests.helpers import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("gfa_out") / "gfa_out")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "kreeq_amd", "host"), "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "gfa_out_main.cpp")])
    return out


def graph(k, seq, segs, edges):
    return types.SimpleNamespace(k=k, seq=seq, segs=segs, edges=edges)


def run(exe, tmp_path, g):
    path = tmp_path / "graph.txt"
    lines = [f"k {g.k}", f"Q {g.seq}"] + ["S " + " ".join(map(str, s)) for s in g.segs] + ["E " + " ".join(map(str, e)) for e in g.edges]
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


HAND = {
    "empty": graph(21, "", [], []),
    "isolated": graph(5, "ACGTA", [(0, 1, 1, 7, 0)], []),
    "cycle": graph(5, "ACGGTCAACGG", [(0, 1, 7, 2, 0)], [(0, 0, 2, 0, 0)]),
    "cycle_minus": graph(5, "ACGGTCAACGG", [(0, 1, 7, 2, 1)], [(0, 0, 9, 1, 1)]),
    "two_components": graph(4, "ACGTTGCAAAGGCC", [(0, 1, 2, 3, 0), (5, 2, 1, 300, 1), (9, 3, 2, 1, 0)], [(0, 1, 4, 0, 1)]),
    "hairpin": graph(4, "ACGTTG", [(0, 1, 3, 1, 0)], [(0, 0, 1, 0, 1)]),
    "both_sides": graph(4, "ACGTTGCAAAGG", [(0, 1, 1, 1, 0), (4, 2, 1, 1, 0), (8, 3, 1, 4294967295, 0)],
                        [(0, 1, 1, 0, 0), (1, 2, 4294967295, 0, 0), (2, 0, 2, 1, 1), (1, 1, 5, 1, 0)]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written(exe, tmp_path, name):
    g = HAND[name]
    assert run(exe, tmp_path, g) == G.gfa_text(g) + "==\n" + "\n".join(G.block_lines(g)) + "\n"


def test_hand_written_numbers():
    """the hand-written graphs say what the definitions mean (both implementations agree on them above)"""
    s = G.stats(HAND["two_components"])
    assert (s["components"], s["largest"], s["dead_ends"], s["disconnected"], s["disconnected_len"], s["circular"]) == (2, 9, 4, 1, 5, 0)
    assert G.stats(HAND["cycle"])["circular"] == G.stats(HAND["cycle_minus"])["circular"] == 1 and G.stats(HAND["cycle"])["dead_ends"] == 0
    assert G.stats(HAND["hairpin"])["circular"] == 0 and G.stats(HAND["hairpin"])["dead_ends"] == 1
    assert G.stats(HAND["empty"]) == {key: 0 for key in G.stats(HAND["empty"])}


@pytest.mark.parametrize("idx", (38, 43))
def test_golden_arrays(exe, tmp_path, idx):
    table, no_collapse, expected = GC.golden_table(idx)
    g = G.build(table, 21, no_collapse)
    out = run(exe, tmp_path, g)
    assert out == G.gfa_text(g) + "==\n" + "\n".join(G.block_lines(g)) + "\n"
    assert out.split("==\n")[1].split("\n")[:-1] == G.golden_block(expected)


@pytest.mark.parametrize("bad", [graph(5, "ACGTA", [(1, 1, 1, 1, 0)], []), graph(5, "ACGTA", [(0, 1, 2, 1, 0)], []), graph(5, "ACGTA", [(0, 1, 0, 1, 0)], []),
                                 graph(5, "ACGTA", [(0, 1, 1, 1, 0)], [(0, 1, 1, 0, 0)]), graph(5, "ACGTA", [(18446744073709551615, 1, 1, 1, 0)], [])])
def test_records_out_of_bounds(exe, tmp_path, bad):
    assert run(exe, tmp_path, bad) == "invalid\n"
