"""The line rules of the per-base tables (kreeq_amd/csrc/kq_table_core.h) as a stand-alone host program under
-fsanitize=address,undefined (tests/native/table_core_main.cpp): lengths first, then the writers into a buffer of exactly that
size, compared byte for byte with tests/table_ref.py."""
import os
import shutil
import subprocess

import pytest

from tests import helpers as H
from tests import table_cases as C
from tests import table_ref as T


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("table") / "table_core")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(H.ROOT, "kreeq_amd", "csrc"), "-o", path, os.path.join(H.ROOT, "tests", "native", "table_core_main.cpp")])
    return path


def run_cases(exe, tmp_path, cases):
    """cases = [(format, k, triples, pieces)] -> the program's text of every case"""
    lines = ["%d" % len(cases)]
    for fmt, k, t, pieces in cases:
        lines.append("%d %d %d %d" % (fmt, k, len(t), len(pieces)))
        lines += ["%d %d %d" % tuple(r) for r in t.tolist()]
        lines += ["%d %d %d %d %d %s" % (p.first, p.n, p.abs_pos, p.n_ctx, int(p.header), p.name.decode()) for p in pieces]
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(path)], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out, at, got = p.stdout, 0, []
    for _ in cases:
        eol = out.index(b"\n", at)
        word, size = out[at:eol].split()
        assert word == b"case"
        got.append(out[eol + 1:eol + 1 + int(size)])
        at = eol + 1 + int(size)
    assert out[at:] == b"0 failures\n"
    return got


def check(exe, tmp_path, cases):
    got = run_cases(exe, tmp_path, cases)
    for (fmt, k, t, pieces), text in zip(cases, got):
        assert text == T.format_table(fmt, k, t, pieces), (fmt, k, len(t), len(pieces))


def test_layouts_values_and_coordinates(exe, tmp_path):
    cases = []
    for fmt in (T.KWIG, T.BED, T.CSV):
        for k in (2, 21, 31, 32):
            for i, abs_pos in enumerate(C.ABS_EDGES):
                t, pieces = C.one_segment(130, 10 * k + i, C.NAMES[(1, 7, 300)[i % 3]], abs_pos)
                cases.append((fmt, k, t, pieces))
            for n in (1, k - 1, k, k + 1):
                cases.append((fmt, k) + C.one_segment(n, n))
            cases.append((fmt, k) + C.big_then_one(k))
    check(exe, tmp_path, cases)


def test_pieces(exe, tmp_path):
    cases = [(fmt, 21) + C.many_pieces(3) for fmt in (T.KWIG, T.BED, T.CSV)]
    for k in (2, 21, 32):
        for cut in (1, 2, k - 1, k, k + 1, 50, 99):
            t, whole, two = C.cut_in_two(k, cut)
            cases += [(T.CSV, k, t, whole), (T.CSV, k, t, two), (T.KWIG, k, t, two)]
    got = run_cases(exe, tmp_path, cases)
    for (fmt, k, t, pieces), text in zip(cases, got):
        assert text == T.format_table(fmt, k, t, pieces)
    for i in range(3, len(cases), 3):
        assert got[i] == got[i + 1]                                        # the pieces give the whole segment's bytes


def test_core_header_alone(tmp_path):
    """kq_table_core.h compiles alone with the host compiler, warnings as errors"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    src = tmp_path / "alone.cpp"
    src.write_text('#include "kq_table_core.h"\nint main() { return kqtab::digits_u32(7) - 1; }\n')
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(H.ROOT, "kreeq_amd", "csrc"), str(src)])
