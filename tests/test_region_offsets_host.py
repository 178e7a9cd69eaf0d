"""The geometry of the table pass's region-major offset matrix (kreeq_amd/csrc/kq_roff_host.h: pitch, rows, bytes) as a
stand-alone host program under -fsanitize=address,undefined: set counts 0, 1, 16, 17, 64 and their neighbours, region counts
from 0 to the format limit, and every element of small matrices written into an exactly-sized block."""
import os
import shutil
import subprocess

from tests.helpers import ROOT


def test_offset_matrix_geometry_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "roff_geometry")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "kreeq_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "native", "roff_geometry_main.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures" in p.stdout
