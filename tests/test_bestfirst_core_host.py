"""The search core of the device best-first (kreeq_amd/csrc/kq_bestfirst_core.h) as a stand-alone host program under
-fsanitize=address,undefined (tests/native/bestfirst_core_main.cpp): one search per seed in a state block of exactly the size
the ABI allocates, each source's discovered set compared with `_dijkstra` of tests/subgraph_ref.py, exactly."""
import os
import shutil
import subprocess

import pytest

from oracle import oracle as O
from tests import bestfirst_cases as B
from tests import helpers as H
from tests import subgraph_ref as R
from tests.test_gpu_subgraph import bubble_genome

MAPS = 128


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("bestfirst") / "bestfirst_core")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(H.ROOT, "kreeq_amd", "csrc"), "-o", path, os.path.join(H.ROOT, "tests", "native", "bestfirst_core_main.cpp")])
    return path


def counted(k, reads):
    db = O.OracleDB(k, MAPS)
    db.count_batch(reads)
    return R.table_of(db.export())


def entry_lines(table):
    return ["%d %s %s" % (key, " ".join(map(str, f)), " ".join(map(str, b))) for key, (f, b, _) in table.items()]


def run_core(exe, tmp_path, k, table, seeds, runs):
    """-> {(depth, cutoff): {source: set of discovered keys}}; the program reported no error code"""
    case = tmp_path / "case.txt"
    case.write_text("\n".join(["%d %d %d %d" % (k, len(table), len(seeds), len(runs))] + entry_lines(table) + entry_lines(seeds) +
                              ["%d %d" % r for r in runs]) + "\n")
    p = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.split("\n")
    assert lines[-2] == "0 failures"
    out, cur = {}, None
    for line in lines[:-2]:
        if line.startswith("run "):
            _, depth, cutoff = line.split()
            cur = out.setdefault((int(depth), int(cutoff)), {})
        else:
            source, _, keys = line.partition(":")
            cur[int(source)] = {int(x) for x in keys.split()}
    return out


def check(exe, tmp_path, k, reads, seed_seq, runs):
    """every source's set against _dijkstra -> {(depth, cutoff): k-mers added over all seeds}"""
    table = counted(k, reads)
    seeds = R.seed(table, [seed_seq], k)
    got = run_core(exe, tmp_path, k, table, seeds, runs)
    added = {}
    for depth, cutoff in runs:
        union = set()
        assert set(got[(depth, cutoff)]) == set(seeds)
        for source in seeds:
            want = R._dijkstra(table, seeds, source, k, depth, cutoff)
            assert got[(depth, cutoff)][source] == want, (k, depth, cutoff, source)
            union |= want
        sub = {key: v for key, v in seeds.items()}
        assert R.best_first(table, sub, k, depth, cutoff) == len(union)
        added[(depth, cutoff)] = len(union)
    return added, seeds


@pytest.mark.parametrize("k", [4, 5])
def test_dense_graphs(exe, tmp_path, k):
    """also the state block at its limit: depth 255 on the dense graphs, no error code"""
    g, seed_seq = B.dense(k)
    runs = [(d, c) for d in B.dense_depths(k) for c in B.DENSE_CUTOFFS]
    added, _ = check(exe, tmp_path, k, g, seed_seq, runs)
    assert {d: added[(d, 0)] for d in B.dense_depths(k)} == B.DENSE_ADDED[k]


def test_bubble(exe, tmp_path):
    k = 21
    reads, seed_seq = bubble_genome(k)
    runs = [(d, c) for d in B.BUBBLE_DEPTHS for c in (0, 2)]
    added, seeds = check(exe, tmp_path, k, reads, seed_seq, runs)
    assert len(seeds) == B.BUBBLE_SEEDS
    assert {r: added[r] for r in B.BUBBLE_ADDED} == B.BUBBLE_ADDED


def test_k32(exe, tmp_path):
    k = 32
    reads, seed_seq = B.two_stretches(k, seed=32)
    added, _ = check(exe, tmp_path, k, reads, seed_seq, [(32, 0)])
    assert added[(32, 0)] > 0


@pytest.mark.parametrize("s", [1, 2, 3, 7])
def test_saturated_dist(exe, tmp_path, s):
    k = 21
    got = []
    for gap in B.SATURATED_GAPS:
        genome, seed_seq = B.saturated(s, gap)
        added, _ = check(exe, tmp_path, k, genome, seed_seq, [(255, 0)])
        got.append(added[(255, 0)])
    if s in B.SATURATED_ADDED:
        assert got == B.SATURATED_ADDED[s]
