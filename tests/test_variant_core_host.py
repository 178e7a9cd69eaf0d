"""The search core of the device candidate-error search (kreeq_amd/csrc/kq_variant_core.h) as a stand-alone host program
under -fsanitize=address,undefined (tests/native/variant_core_main.cpp): one search per position in a state block of exactly
the size the ABI allocates, every path compared with `dbg_to_variants` of oracle/variants.py on the same table, exactly."""
import os
import shutil
import subprocess

import pytest

from oracle import variants as V
from tests import bestfirst_cases as B
from tests import helpers as H
from tests import variant_cases as C


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("variant") / "variant_core")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(H.ROOT, "kreeq_amd", "csrc"), "-o", path, os.path.join(H.ROOT, "tests", "native", "variant_core_main.cpp")])
    return path


def run_core(exe, tmp_path, g, segments, runs):
    """-> {(depth, span, cutoff): [(segment, pos, type, refLen, sequence)]}; the program reported no error code"""
    case = tmp_path / "case.txt"
    table = ["%d %s %s" % (key, " ".join(map(str, f)), " ".join(map(str, b))) for key, (f, b, _) in g.nodes.items()]
    case.write_text("\n".join(["%d %d %d %d" % (g.k, len(table), len(segments), len(runs))] + table + list(segments) + ["%d %d %d" % r for r in runs]) + "\n")
    p = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.split("\n")
    assert lines[-2] == "0 failures"
    out, cur = {}, None
    probe = [int(x) for x in lines[-3].split()[1:]]                     # overflowing searches ended by an error code, searches, refused heads
    assert lines[-3].startswith("probe ") and probe[2] == probe[1]
    out["probe"] = probe
    for line in lines[:-3]:
        w = line.split()
        if w[0] == "run":
            cur = out.setdefault((int(w[1]), int(w[2]), int(w[3])), [])
        else:
            cur.append((int(w[0]), int(w[1]), int(w[2]), int(w[3]), "" if w[4] == "-" else w[4]))
    return out


def check(exe, tmp_path, monkeypatch, g, segments, runs):
    """every run against the oracle -> {run: expected paths}"""
    got = run_core(exe, tmp_path, g, segments, runs)
    want = {}
    for depth, span, cutoff in runs:
        with monkeypatch.context() as m:
            C.with_cutoff(m, cutoff)
            want[(depth, span, cutoff)] = C.expected(g, segments, depth, span)
        assert got[(depth, span, cutoff)] == want[(depth, span, cutoff)], (g.k, depth, span, cutoff)
    return want


def types_of(paths):
    return {p[2] for p in paths}


@pytest.mark.parametrize("k", [4, 5])
def test_dense_graphs(exe, tmp_path, monkeypatch, k):
    """a random 300-base string counted at k = 4 / 5 and searched along itself: almost every position branches, windows hold
    repeated keys (erase quirk, first-occurrence refLen), targets are reached from several pops (repeated destination
    entries) and walks pass the source; depth 252 and 253 are the state block at its limit, with no error code"""
    text = B.dense(k)[0].decode()
    g = C.graph_of(k, text)
    runs = [(1, 5, 0), (k, 32, 0), (12, 255, 0), (40, 32, 2), (252, 32, 0), (253, 255, 0)]
    want = check(exe, tmp_path, monkeypatch, g, [text, text[40:40 + 2 * k], text[7:7 + k], text[100:100 + k + 1]], runs)
    deep = want[(253, 255, 0)]
    assert types_of(deep) >= {1, 2, 3}
    by_pos = {}
    for p in deep:
        by_pos.setdefault(p[:2], []).append(p)
    assert any(len(v) > len(set(v)) for v in by_pos.values())           # a target reached twice: two equal records
    # a COM of refLen r writes r bases, one per step back from the popped node; at depth 12 a chain has at most 12 steps to
    # the source, so a longer COM walked past the source (through key 0)
    assert any(p[2] == 3 and p[3] > 14 for p in want[(12, 255, 0)])
    assert all(x > 0 for x in C.window_stats(k, text, 32))
    got = run_core(exe, tmp_path, g, [text], [(1, 5, 0)])
    assert got["probe"][0] > 0                                          # searches that outgrow a depth-0 block: error code, no report from the sanitizers


def test_planted_errors(exe, tmp_path, monkeypatch):
    """k = 21: one SNV, one INS, one DEL and one COM (two substitutions closer than max_span); every max_span and depth of the
    issue's list, the empty target window (segments with kcount <= k + 1) and the search at the last k-mer of a segment"""
    k = 21
    reads, asm, genome = C.planted(k)
    g = C.graph_of(k, reads)
    segments = [asm, asm[100:100 + k + 1], asm[100:100 + 2 * k], asm[470:470 + k + 40], genome[:k - 1]]
    runs = [(60, s, 0) for s in (0, 1, 5, 32, 255)] + [(d, 32, 0) for d in (0, 1, k)]
    want = check(exe, tmp_path, monkeypatch, g, segments, runs)
    full = [p for p in want[(60, 32, 0)] if p[0] == 0]
    assert types_of(full) == {0, 1, 2, 3}
    assert [p[1:] for p in full if p[2] == 0] == [(120, 0, 0, genome[120])]
    assert [p[1:] for p in full if p[2] == 3] == [(500, 3, 6, genome[500:506])]
    assert any(p[0] == 3 for p in want[(60, 32, 0)])                    # found from a position whose segment ends inside the window


@pytest.mark.parametrize("k", [31, 32])
def test_wide_keys(exe, tmp_path, monkeypatch, k):
    """k = 31 and k = 32 (keys at and above 2^63)"""
    reads, asm, _ = C.planted(k, seed=k)
    g = C.graph_of(k, reads)
    if k == 32:
        assert any(key >= 1 << 63 for key in g.nodes)
    want = check(exe, tmp_path, monkeypatch, g, [asm], [(60, 32, 0)])
    assert types_of(want[(60, 32, 0)]) == {0, 1, 2, 3}


def test_tandem_repeat(exe, tmp_path, monkeypatch):
    """a repeat of period 7 inside the window: the same key several times in targets_queue and on both sides of the window's
    left edge, so the erase quirk decides what is a target"""
    k = 21
    reads, asm, _ = C.tandem(k)
    g = C.graph_of(k, reads)
    twice, erased = C.window_stats(k, asm, 32)
    assert twice > 20 and erased > 20                                   # the input has both situations
    want = check(exe, tmp_path, monkeypatch, g, [asm], [(60, 32, 0), (60, 5, 0), (30, 255, 0)])
    assert want[(60, 32, 0)]


def test_cutoffs(exe, tmp_path, monkeypatch):
    """cutoffs 0, 1 and 3 on a thin graph: backward counters of 1 .. 4 (the cutoff applies to backward edges only, :237)"""
    k = 21
    reads, genome = C.thin(k)
    g = C.graph_of(k, reads)
    assert {1, 2, 3, 4} <= {c for _, bw, _ in g.nodes.values() for c in bw}
    want = check(exe, tmp_path, monkeypatch, g, [genome], [(30, 32, c) for c in (0, 1, 3)])
    assert want[(30, 32, 0)] != want[(30, 32, 3)]


def test_bestfirst_header_alone(tmp_path):
    """kq_bestfirst_core.h and kq_variant_core.h each compile alone with the host compiler (they share kq_nodequeue_core.h)"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    for name in ("kq_bestfirst_core.h", "kq_variant_core.h", "kq_nodequeue_core.h"):
        src = tmp_path / (name + ".cpp")
        src.write_text('#include "%s"\nint main() { return 0; }\n' % name)
        subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(H.ROOT, "kreeq_amd", "csrc"), str(src)])
