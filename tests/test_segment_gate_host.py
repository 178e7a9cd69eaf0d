"""The gate between the two last split levels (kreeq_amd/csrc/kq_seg_gate_host.h: does a slice's largest hash-prefix bucket hold
at most 1/16 more than the mean?) as a stand-alone host program under -fsanitize=address,undefined: uniform offsets, one bucket at
the threshold and just above it, all records in one bucket, zero records, empty buckets, sizes beyond the format limit."""
import os
import shutil
import subprocess

from tests.helpers import ROOT


def test_segment_gate_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "seg_gate")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "kreeq_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "native", "seg_gate_main.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures" in p.stdout
