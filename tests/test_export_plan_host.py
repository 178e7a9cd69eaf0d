"""How results leave the device (kreeq_amd/csrc/kq_export_host.h: one copy or chunks through two pinned bounce buffers, the
double-buffer loop that copy_out_bounced instantiates with the HIP calls, and k_export's range and capacity conditions) as a
stand-alone host program under -fsanitize=address,undefined.  tests/native/export_plan_main.cpp checks the plan at the
library's 16 MiB chunk by a hand-written table (64 MiB goes in one copy, 1 398 102 entries are 5 chunks with a last one of 32
bytes, 2 097 152 entries are 6 full chunks), then runs the loop with host stand-ins at chunk sizes 1, 7, 48, 64, 100, 4096, 4099
and a few hundred random ones, byte counts 0, 1, 48, 4c, 4c + 1, 4c + 48, 5c - 1, 6c, 6c +- 48 and random: source, destination
and bounce buffers are heap blocks of exactly their size, a copy takes effect only at the next sync, and a state per buffer says
whether a chunk is read before its copy was waited for or overwritten before it was read.  An injected error at every call ends
the loop with the earlier chunks delivered and nothing behind them touched."""
import os
import shutil
import subprocess

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "kreeq_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "native", "export_plan_main.cpp")


def build_export_plan(out, sanitize):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags + ["-I", CSRC, "-o", out, SOURCE])
    return out


def test_export_plan_under_sanitizers(tmp_path):
    exe = build_export_plan(str(tmp_path / "export_plan"), sanitize=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 failures" in p.stdout
