"""The scoped owners of the ABI layer (kreeq_amd/csrc/kq_mem_host.h) as a stand-alone host program under
-fsanitize=address,undefined (tests/native/mem_owner_main.cpp): the runtime calls are counting stand-ins on the host heap, so
the sanitizer's leak and double-free checks see every allocation an owner makes -- growth policy and free-before-allocate
order, failed allocations, moves and swaps, DevScope, a vector of owning structs, events and streams."""
import os
import shutil
import subprocess

from tests import helpers as H


def test_owners(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mem_owner")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(H.ROOT, "kreeq_amd", "csrc"), "-o", exe, os.path.join(H.ROOT, "tests", "native", "mem_owner_main.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.split("\n")[-2] == "0 failures"
