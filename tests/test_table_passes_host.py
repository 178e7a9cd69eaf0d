"""The plan of the per-base table under map-range passes (plan_table_passes, kreeq_amd/host/cli_plan.h) as a stand-alone host
program under -fsanitize=address,undefined (tests/native/table_passes_main.cpp), at call limits of 8, 100, 200 and 2^30 bytes:
sequences of 0, 1, limit - 1 and limit bytes, sequences with N runs and one without bases; every segment in exactly one group,
in order, its rebased start inside the group's text; first_triple the running sum; the accumulator 12 bytes per position, the
text buffer and the per-base array those of the largest group; a sequence above the limit reported as not fitting."""
import os
import shutil
import subprocess

from tests.helpers import ROOT


def test_table_passes_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "table_passes")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "kreeq_amd", "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "table_passes_main.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures" in p.stdout
