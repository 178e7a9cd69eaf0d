"""The output plan of -o x.kwig.gz / x.bed.gz / x.csvtable.gz (kreeq_amd/host/cli_plan.h) as a stand-alone host program under
-fsanitize=address,undefined (tests/native/cli_plan_gz_main.cpp): the three names set table_gz and the format inside while ext
keeps its ".gz" and per_base stays false; x.bkwig.gz, x.gfa.gz, x.vcf.gz and the plain names do not.  And the host's BGZF
writer (kreeq_amd/host/bgzf_out.h) under the same sanitizers: what is printed into it comes back from zlib."""
import gzip
import os
import shutil
import subprocess

from tests.helpers import ROOT

FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "kreeq_amd", "host"), "-I", os.path.join(ROOT, "include")]


def cxx():
    c = shutil.which("g++") or shutil.which("clang++")
    assert c, "no host C++ compiler"
    return c


def test_gz_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "cli_plan_gz")
    subprocess.check_call([cxx()] + FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "native", "cli_plan_gz_main.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures" in p.stdout


def test_host_bgzf_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bgzf_out")
    subprocess.check_call([cxx()] + FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "native", "bgzf_out_main.cpp"), "-lz"])
    for n in (0, 1, 65279, 65280, 65281, 200000):
        out = tmp_path / ("t%d.gz" % n)
        p = subprocess.run([exe, str(n), str(out)], capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr
        data = out.read_bytes()
        assert gzip.decompress(data) == p.stdout and len(p.stdout) == 2 * n      # a compressible half and random bytes
        assert data[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
        at, members = 0, 0
        while at < len(data):                                                 # every member: BSIZE fits, at most its stored form
            size = int.from_bytes(data[at + 16:at + 18], "little") + 1
            isize = int.from_bytes(data[at + size - 4:at + size], "little")
            assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and isize <= 0xff00 and size <= 18 + 5 + isize + 8
            at += size
            members += 1
        assert at == len(data) and members == (2 * n + 0xff00 - 1) // 0xff00 + 1
