"""Replays the reference's subgraph goldens (validateFiles/test.36.tst .. test.47.tst) against OUR `kreeq subgraph` on the GPU.
The "+++Assembly summary+++" block is gfalibs' report of the GFA model, which this build does not have: it is cut out of
the GOLDEN (from its first line up to, excluding, "DBG Summary statistics:"); the CLI's stdout is compared whole."""
import os
import subprocess

import pytest

from kreeq_amd import build
from tests import helpers as H
from tests.test_gpu_cli import remap

pytestmark = pytest.mark.gpu

SUBGRAPH_TESTS = list(range(36, 48))


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(build.LIB), "libkreeq_amd.so must be built in-tree"
    return build.build_cli()


def without_assembly_block(lines):
    a = lines.index("+++Assembly summary+++: ")
    b = lines.index("DBG Summary statistics:")
    assert a < b
    return lines[:a] + lines[b:]


@pytest.mark.parametrize("device_reader", [False, True])
@pytest.mark.parametrize("idx", SUBGRAPH_TESTS)
def test_subgraph_tst_replay(cli, golden_dbs, idx, device_reader):
    argv, expected = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", f"test.{idx}.tst"))
    env = dict(os.environ)
    env.pop("KQ_DB_DEVICE", None)
    if device_reader:
        env["KQ_DB_DEVICE"] = "1"
    p = subprocess.run([cli] + remap(argv, golden_dbs), capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr
    got = p.stdout.split("\n")
    while got and got[-1] == "":
        got.pop()
    assert got == without_assembly_block(expected)


def test_issue_example(cli, golden_dbs):
    p = subprocess.run([cli, "subgraph", "-d", os.path.join(golden_dbs, "random10.kreeq"), "-f", H.golden_input("random5.fasta"),
                        "--search-depth", "16", "--traversal-algorithm", "traversal"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.split("\n")[:6] == ["Subgraph summary statistics:", "Total kmers: 158", "Unique kmers: 62", "Distinct kmers: 110",
                                        "Missing kmers: 4398046510994", "Total edges: 188"]
    assert p.stdout.split("\n")[6] == "DBG Summary statistics:"


@pytest.mark.parametrize("extra", [["--traversal-algorithm", "depth-first"], ["-p", "BED"], ["-o", "x.gfa"]])
def test_refused_options(cli, golden_dbs, tmp_path, extra):
    """an unknown algorithm, -p and -o end with a message and a non-zero status: no abort, no output file"""
    extra = [H.golden_input("decompressor1.bed") if a == "BED" else a for a in extra]
    p = subprocess.run([cli, "subgraph", "-d", os.path.join(golden_dbs, "random10.kreeq"), "-f", H.golden_input("random5.fasta")] + extra,
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 1
    assert p.stderr.strip() != "" and "Traceback" not in p.stderr and "terminate" not in p.stderr
    assert "Subgraph summary statistics:" not in p.stdout
    assert os.listdir(str(tmp_path)) == []
    if extra[0] == "--traversal-algorithm":
        assert p.stderr == "Cannot find input algorithm (depth-first). Terminating.\n"      # reference src/subgraph.cpp:296
