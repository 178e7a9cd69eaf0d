"""The map-range loop of the CLI (kreeq_amd/host/run.cpp: run_ranges) where the other CLI suites leave a gap: a union's
histogram added up over ranges, and `--passes 1`, which is the loop with one range and must be the resident case -- the same
bytes as the run without --passes for a per-base file and for the variant search, which reads the resident table."""
import os
import subprocess

import pytest

from kreeq_amd import build
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(build.LIB), "libkreeq_amd.so must be built in-tree"
    return build.build_cli()


def run(cli, args, cwd=None):
    p = subprocess.run([cli] + args, capture_output=True, text=True, cwd=cwd, timeout=300)
    assert p.returncode == 0, p.stderr
    return p.stdout


def test_union_hist_over_ranges(cli, tmp_path, golden_dbs):
    d1, d2 = os.path.join(golden_dbs, "test1.kreeq"), os.path.join(golden_dbs, "test2.kreeq")
    h1, h3 = str(tmp_path / "one.hist"), str(tmp_path / "three.hist")
    out1 = run(cli, ["union", "-d", d1, d2, "-o", h1])
    out3 = run(cli, ["union", "-d", d1, d2, "-o", h3, "--passes", "3"])
    _, exp35 = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", "test.35.tst"))
    assert [l for l in out1.split("\n") if l] == exp35 and out3 == out1
    assert os.path.getsize(h1) > 0 and open(h3, "rb").read() == open(h1, "rb").read()


def test_one_pass_is_the_resident_case(cli, tmp_path):
    base = ["validate", "-f", H.golden_input("random1.fasta"), "-r", H.golden_input("random1.fastq")]
    b0, b1 = str(tmp_path / "none.bkwig"), str(tmp_path / "one.bkwig")
    assert run(cli, base + ["-o", b1, "--passes", "1"]) == run(cli, base + ["-o", b0])
    assert os.path.getsize(b0) > 20 and open(b1, "rb").read() == open(b0, "rb").read()
    vcf = run(cli, base + ["-o", "vcf"], cwd=str(tmp_path))
    assert vcf.startswith("##fileformat=VCF") and run(cli, base + ["-o", "vcf", "--passes", "1"], cwd=str(tmp_path)) == vcf
    assert not [f for f in os.listdir(tmp_path) if f.startswith(".kreeq_ranges_")]      # no temporary database: the table was resident
