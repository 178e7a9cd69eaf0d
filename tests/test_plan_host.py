"""The count path's sizing arithmetic (kreeq_amd/csrc/kq_plan_host.h: region counts, windows, growth, the partition plan and its
split levels, the layout of the partition scratch, pending sets and their arena, slices, and which path a slice or a lookup
takes) as a stand-alone host program under -fsanitize=address,undefined.  tests/native/plan_main.cpp holds a table written out by
hand from the arithmetic as it stood inside kreeq_amd.hip -- the geometries of tools/bench_extra/selection_trace.py at
k in {15, 21, 25, 30, 31}, the headline table of 3 391 488 regions, round_regions not being idempotent (8 403 324 -> 8 421 376,
257 regions per sub-bucket), a table grown from 257 to 2056 regions keeping packed records, one scratch layout in full with the
second record array on an odd 8-byte word -- and checks what the kernels rely on over every region request within 600 of a power
of two from 2^4 to 2^24, at k in {15, 21, 25, 29, 32}, each also doubled up to three times (up to 2^24 regions, a 512 GiB table):
the arrays of every plan's scratch are disjoint and inside it, every fan-out is below NB_MAX, every bucketed geometry gets the
bucketed plan, and consecutive slices emit every k-mer start exactly once."""
import os
import shutil
import subprocess

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "kreeq_amd", "csrc")


def test_plan_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "plan_main.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 failures" in p.stdout
