"""The decisions of the `kreeq` CLI that need no GPU (kreeq_amd/host/cli_plan.h) as a stand-alone host program under
-fsanitize=address,undefined (tests/native/cli_plan_main.cpp): what every -o name asks for, against a table written out by hand
(summary, QV table, per-base file, VCF, database, histogram, the refusal of the variant graph); whole sequences grouped into
device calls at a limit of 8 bytes (limit - 1 bases fit with their separator, `limit` bases form a call of their own, empty
sequences, a call that ends exactly at the limit; every sequence in exactly one call, in order, and all_fit agreeing); and the
cutter of formatted chunks at k = 2, 5, 32 with chunks of 1, k - 1, k and the segment length - 1, + 0, + 1 (every position in
one piece, in order; the header flag on a segment's first piece only; n_ctx = min(done, k - 1) when expanded, else 0; no chunk
above its size; abs_pos and name of the owning sequence)."""
import os
import shutil
import subprocess

from tests.helpers import ROOT


def test_cli_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "cli_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "kreeq_amd", "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "cli_plan_main.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures" in p.stdout
