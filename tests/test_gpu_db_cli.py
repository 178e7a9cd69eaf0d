"""The CLI with KQ_DB_DEVICE=1: the database files are built and read on the GPU (kq_export_map_images /
kq_import_map_image).  Every file written and stdout are byte-identical to the default mode, whose writer and reader stay
on the host; the KQ_DB_TRACE line proves which path ran."""
import filecmp
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


def run(cli, args, device, cwd=None):
    env = dict(os.environ, KQ_DB_TRACE="1")
    env.pop("KQ_DB_DEVICE", None)
    if device:
        env["KQ_DB_DEVICE"] = "1"
    p = subprocess.run([cli] + args, capture_output=True, text=True, timeout=300, env=env, cwd=cwd)
    assert p.returncode == 0, p.stderr
    trace = [l for l in p.stderr.split("\n") if l.startswith("[db]")]
    assert trace and all(l.endswith("(device)" if device else "(host)") for l in trace), p.stderr
    return p.stdout


def same_database(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) == 130            # 128 maps, .map.hc.bin, .index
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


@pytest.fixture(scope="module")
def own_dbs(cli, tmp_path_factory):
    """random1 / random2 counted into databases in both modes"""
    d = tmp_path_factory.mktemp("db_cli")
    out = {}
    for name in ("random1", "random2"):
        for device in (False, True):
            db = str(d / f"{name}.{'device' if device else 'host'}.kreeq")
            out[name, device] = (db, run(cli, ["validate", "-r", H.golden_input(name + ".fastq"), "-o", db], device))
    return out


def test_count_to_database(own_dbs):
    for name in ("random1", "random2"):
        (host_db, host_out), (dev_db, dev_out) = own_dbs[name, False], own_dbs[name, True]
        assert host_out == dev_out and host_out.startswith("DBG Summary statistics:")
        same_database(host_db, dev_db)


@pytest.mark.parametrize("how", [["--passes", "4"], ["-m", "0.001"]])
def test_map_range_passes(cli, tmp_path, own_dbs, how):
    reads = [H.golden_input("random1.fastq"), H.golden_input("random2.fastq")]
    dbs = []
    for device in (False, True):
        db = str(tmp_path / f"{'device' if device else 'host'}.kreeq")
        dbs.append((db, run(cli, ["validate", "-r"] + reads + ["-o", db] + how, device)))
    assert dbs[0][1] == dbs[1][1]
    same_database(dbs[0][0], dbs[1][0])


def test_validate_from_reference_database(cli, golden_dbs):
    _, exp = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", "test.0.tst"))
    args = ["validate", "-f", H.golden_input("random1.fasta"), "-d", os.path.join(golden_dbs, "test1.kreeq")]
    got = run(cli, args, True)
    assert [l for l in got.split("\n") if l] == exp
    assert got == run(cli, args, False)


def test_union(cli, tmp_path, own_dbs, golden_dbs):
    _, exp35 = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", "test.35.tst"))
    for a, b in ((own_dbs["random1", True][0], own_dbs["random2", True][0]),
                 (os.path.join(golden_dbs, "test1.kreeq"), os.path.join(golden_dbs, "test2.kreeq"))):
        outs = []
        for device in (False, True):
            u = str(tmp_path / f"u{len(os.listdir(str(tmp_path)))}.kreeq")
            outs.append((u, run(cli, ["union", "-d", a, b, "-o", u], device)))
        assert outs[0][1] == outs[1][1] and [l for l in outs[1][1].split("\n") if l] == exp35
        same_database(outs[0][0], outs[1][0])
