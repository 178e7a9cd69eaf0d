"""`kreeq subgraph --traversal-algorithm best-first` with KQ_SUBGRAPH_DEVICE=1 (the searches run on the GPU through
kq_subgraph_best_first) against the reference's subgraph goldens (validateFiles/test.36.tst .. test.47.tst) and against the
host search of the same binary: stdout is the same, the trace on stderr says which path ran."""
import os
import subprocess

import pytest

from kreeq_amd import build
from tests import helpers as H
from tests.test_gpu_cli import remap
from tests.test_gpu_subgraph_cli import SUBGRAPH_TESTS, without_assembly_block

pytestmark = pytest.mark.gpu

DEVICE_WORDS = "best-first ran as the device search"
HOST_WORDS = "best-first ran as the host search"


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(build.LIB), "libkreeq_amd.so must be built in-tree"
    return build.build_cli()


def run(cli, args, device):
    env = dict(os.environ)
    env.pop("KQ_SUBGRAPH_DEVICE", None)
    env.pop("KQ_DB_DEVICE", None)
    env["KQ_SUBGRAPH_TRACE"] = "1"
    if device:
        env["KQ_SUBGRAPH_DEVICE"] = "1"
    p = subprocess.run([cli] + args, capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr
    return p


def best_first_of(argv):
    return "traversal" not in [argv[i + 1] for i, a in enumerate(argv[:-1]) if a == "--traversal-algorithm"]


def test_goldens_cover_both_algorithms():
    kinds = [best_first_of(H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", f"test.{idx}.tst"))[0]) for idx in SUBGRAPH_TESTS]
    assert sum(kinds) == 10 and len(kinds) == 12


@pytest.mark.parametrize("idx", SUBGRAPH_TESTS)
def test_subgraph_tst_replay_device_search(cli, golden_dbs, idx):
    argv, expected = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", f"test.{idx}.tst"))
    p = run(cli, remap(argv, golden_dbs), device=True)
    got = p.stdout.split("\n")
    while got and got[-1] == "":
        got.pop()
    assert got == without_assembly_block(expected)
    if best_first_of(argv):
        assert DEVICE_WORDS in p.stderr and HOST_WORDS not in p.stderr
    else:
        assert DEVICE_WORDS not in p.stderr and HOST_WORDS not in p.stderr


def test_deeper_search_both_modes(cli, golden_dbs):
    args = ["subgraph", "-d", os.path.join(golden_dbs, "random10.kreeq"), "-f", H.golden_input("random5.fasta"), "--search-depth", "40", "-c", "1"]
    host, dev = run(cli, args, device=False), run(cli, args, device=True)
    assert HOST_WORDS in host.stderr and DEVICE_WORDS not in host.stderr
    assert DEVICE_WORDS in dev.stderr and HOST_WORDS not in dev.stderr
    assert host.stdout == dev.stdout
    assert host.stdout.startswith("Subgraph summary statistics:\n")


def test_depth_above_255_keeps_the_host_search(cli, golden_dbs):
    args = ["subgraph", "-d", os.path.join(golden_dbs, "random10.kreeq"), "-f", H.golden_input("random5.fasta"), "--search-depth", "300"]
    p = run(cli, args, device=True)
    assert HOST_WORDS in p.stderr and DEVICE_WORDS not in p.stderr
    assert p.stdout.startswith("Subgraph summary statistics:\n")
