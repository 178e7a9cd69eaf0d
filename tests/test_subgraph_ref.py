"""The Python restatement of `kreeq subgraph` (tests/subgraph_ref.py) against the reference's own goldens
(validateFiles/test.36.tst .. test.47.tst): the five numbers of their "Subgraph summary statistics" block.  No GPU."""
import os

import pytest

from tests import helpers as H
from tests import subgraph_ref as R

SUBGRAPH_TESTS = list(range(36, 48))
K = 21                                                                   # every fixture database (db_tables/*.tsv header)


def parse_subgraph_cmd(argv):
    """['kreeq','subgraph','-d',db,'-f',fasta,...] -> keyword arguments of run_golden"""
    o = {"db": None, "fasta": None, "depth": None, "algorithm": "best-first", "no_reference": False, "cov_cutoff": 0}
    i = 2
    while i < len(argv):
        a = argv[i]
        if a == "-d":
            o["db"] = os.path.basename(argv[i + 1])[:-len(".kreeq")]
            i += 2
        elif a == "-f":
            o["fasta"] = H.golden_input(argv[i + 1])
            i += 2
        elif a == "-c":
            o["cov_cutoff"] = int(argv[i + 1])
            i += 2
        elif a == "--search-depth":
            o["depth"] = int(argv[i + 1])
            i += 2
        elif a == "--traversal-algorithm":
            o["algorithm"] = argv[i + 1]
            i += 2
        elif a == "--no-reference":
            o["no_reference"] = True
            i += 1
        else:
            i += 1                                                       # --no-collapse: no effect on the k-mer set
    return o


def golden_block(lines):
    """the five numbers under 'Subgraph summary statistics:'"""
    at = lines.index("Subgraph summary statistics:")
    names = ("total", "unique", "distinct", "missing", "edges")
    return {n: int(lines[at + 1 + j].split(": ")[1]) for j, n in enumerate(names)}


_tables = {}


def run_golden(idx, depth_override=None):
    argv, expected = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", f"test.{idx}.tst"))
    o = parse_subgraph_cmd(argv)
    if o["db"] not in _tables:
        _tables[o["db"]] = R.table_of(H.load_db_table(o["db"]))
    seqs = [s for _, s in H.read_fastx(o["fasta"])]
    depth = o["depth"] if depth_override is None else depth_override
    sub = R.subgraph(_tables[o["db"]], seqs, K, depth, o["algorithm"], o["no_reference"], o["cov_cutoff"])
    return R.summary(sub, K), golden_block(expected), o


@pytest.mark.parametrize("idx", SUBGRAPH_TESTS)
def test_restatement_matches_golden(idx):
    got, want, _ = run_golden(idx)
    assert got == want


@pytest.mark.parametrize("idx", SUBGRAPH_TESTS)
def test_goldens_need_the_expansion(idx):
    """without the expansion (depth 0) every golden but test 36 -- which asks for depth 0 -- gives other numbers"""
    got, want, o = run_golden(idx, depth_override=0)
    if o["depth"] == 0:
        assert idx == 36 and got == want
    else:
        assert got != want


def test_algorithms_covered():
    algos = {}
    for idx in SUBGRAPH_TESTS:
        argv, _ = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", f"test.{idx}.tst"))
        algos.setdefault(parse_subgraph_cmd(argv)["algorithm"], []).append(idx)
    assert algos["traversal"] == [43, 44] and len(algos["best-first"]) == 10
