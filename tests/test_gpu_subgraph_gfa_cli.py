"""`kreeq subgraph` with KQ_SUBGRAPH_GFA=1 against the reference's subgraph goldens (validateFiles/test.36.tst .. test.47.tst):
stdout is the WHOLE golden but for the two lines this build does not print (`# separated components`, `# bubbles`), and
-o <name>.gfa is the text tests/gfa_ref.py makes from the restatement's table.  Without the variable nothing changes."""
import os
import subprocess

import pytest

from kreeq_amd import build
from tests import gfa_cases as GC
from tests import gfa_ref as G
from tests.test_gpu_cli import remap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(build.LIB), "libkreeq_amd.so must be built in-tree"
    return build.build_cli()


def run(cli, golden_dbs, idx, extra=(), cwd=None, gfa=True, device=False):
    argv, expected = GC.golden_argv(idx)
    env = dict(os.environ)
    for name in ("KQ_SUBGRAPH_GFA", "KQ_SUBGRAPH_DEVICE", "KQ_DB_DEVICE"):
        env.pop(name, None)
    if gfa:
        env["KQ_SUBGRAPH_GFA"] = "1"
    if device:
        env["KQ_SUBGRAPH_DEVICE"] = "1"
    p = subprocess.run([cli] + remap(argv, golden_dbs) + list(extra), capture_output=True, text=True, timeout=120, env=env, cwd=cwd)
    got = p.stdout.split("\n")
    while got and got[-1] == "":
        got.pop()
    return p, got, expected


def printed(expected):
    return [x for x in expected if not x.startswith(G.UNPRINTED)]


@pytest.mark.parametrize("idx", GC.SUBGRAPH_TESTS)
def test_golden_stdout(cli, golden_dbs, idx):
    p, got, expected = run(cli, golden_dbs, idx)
    assert p.returncode == 0, p.stderr
    assert len(printed(expected)) == len(expected) - 2
    assert got == printed(expected)


@pytest.mark.parametrize("idx", (38, 47))
def test_golden_stdout_device_search(cli, golden_dbs, idx):
    p, got, expected = run(cli, golden_dbs, idx, device=True)
    assert p.returncode == 0, p.stderr
    assert got == printed(expected)


@pytest.mark.parametrize("idx", (37, 38, 43))
def test_gfa_file(cli, golden_dbs, tmp_path, idx):
    p, got, expected = run(cli, golden_dbs, idx, extra=["-o", "out.gfa", "--verbose"], cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr
    assert got == printed(expected)
    table, no_collapse, _ = GC.golden_table(idx)
    want = G.build(table, 21, no_collapse)
    assert os.listdir(str(tmp_path)) == ["out.gfa"]
    text = (tmp_path / "out.gfa").read_text()
    assert text == G.gfa_text(want)
    kinds = [line[0] for line in text.split("\n") if line]
    block = dict(line.split(": ") for line in got if line.startswith("# "))
    assert kinds.count("S") == int(block["# segments"]) and kinds.count("L") == int(block["# edges"]) and kinds.count("H") == 1
    c = want.counts
    assert f"subgraph GFA built on the device: {c['n_segments']} segments, {c['n_edges']} links, {c['n_dropped_edges']} links dropped, {c['n_cycles']} cycles" in p.stderr


def test_trace_step(cli, golden_dbs):
    argv, _ = GC.golden_argv(38)
    env = dict(os.environ, KQ_SUBGRAPH_GFA="1", KQ_SUBGRAPH_TRACE="1")
    p = subprocess.run([cli] + remap(argv, golden_dbs), capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0 and "[subgraph] gfa: " in p.stderr


@pytest.mark.parametrize("extra", [["-o", "x.gfa.gz"], ["-o", "x.gfa2"], ["-o", "x.vcf"], ["-o", "gfa"], ["-p", "BED"]])
def test_still_refused(cli, golden_dbs, tmp_path, extra):
    from tests import helpers as H

    extra = [H.golden_input("decompressor1.bed") if a == "BED" else a for a in extra]
    p, got, _ = run(cli, golden_dbs, 38, extra=extra, cwd=str(tmp_path))
    assert p.returncode == 1 and p.stderr.strip() != "" and "terminate" not in p.stderr
    assert "Subgraph summary statistics:" not in p.stdout and os.listdir(str(tmp_path)) == []


def test_refused_without_the_variable(cli, golden_dbs, tmp_path):
    p, got, _ = run(cli, golden_dbs, 38, extra=["-o", "out.gfa"], cwd=str(tmp_path), gfa=False)
    assert p.returncode == 1
    assert p.stderr == "Error: -o out.gfa: subgraph output files (GFA) are not supported by this build; the summary goes to stdout.\n"
    assert p.stdout == "" and os.listdir(str(tmp_path)) == []
