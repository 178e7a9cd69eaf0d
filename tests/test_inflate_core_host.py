"""The DEFLATE core (kreeq_amd/csrc/kq_inflate_core.h) and the BGZF block walk (kq_bgzf_host.h) as a stand-alone host program
under -fsanitize=address,undefined (tests/native/inflate_core_main.cpp), on heap arrays of exactly the sizes the core may use:
every good block gives zlib's bytes, every mutation its error code, and random damage either the exact text or an error."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import bgzf_inputs as B
from tests import helpers as H
from tests import inflate_streams as S

CSRC = os.path.join(H.ROOT, "kreeq_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("inflate") / "inflate_core")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", path, os.path.join(H.ROOT, "tests", "native", "inflate_core_main.cpp")])
    return path


def run_cases(exe, tmp_path, cases):
    """cases: [(expect, member, text)] -> [(code, max_len, max_dist)]; the program found no failure and the sanitizers nothing"""
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for expect, mem, text in cases:
            f.write(struct.pack("<III", expect, len(mem), len(text)) + mem + text)
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-4000:]
    lines = p.stdout.strip().split("\n")
    assert lines[-1] == "0 failures"
    out = [tuple(int(x) for x in l.split()[2:]) for l in lines[:-1] if l.startswith("case ") and ":" not in l]
    assert len(out) == len(cases)
    return out


@pytest.fixture(scope="module")
def good():
    return B.good_blocks()


def test_good_blocks_give_zlibs_bytes(exe, tmp_path, good):
    names = sorted(good)
    for name in names:
        mem, text = good[name]
        assert zlib.decompress(mem, 31) == text, name              # the yardstick: zlib reads the member as gzip
    got = dict(zip(names, run_cases(exe, tmp_path, [(0, good[n][0], good[n][1]) for n in names])))
    assert all(code == 0 for code, _, _ in got.values())
    assert got["fibonacci"][1] == 15                               # a 15-bit code was built and used
    assert got["far_reference"][2] > 32000
    assert got["A_65536"][2] == 1
    assert got["stored_max"][1] == 0                               # no code at all: stored


def test_block_types_are_what_the_names_say(good):
    def btypes(mem):
        return (mem[18] >> 1) & 3
    assert btypes(good["stored_max"][0]) == 0 and btypes(good["stored_70"][0]) == 0
    assert btypes(good["fixed"][0]) == 1
    assert all(btypes(good["fastq_level%d" % lv][0]) == 2 for lv in (1, 6, 9))
    assert len(good["A_65536"][0]) == 105
    assert len(good["stored_max"][0]) == 65536                     # the most a stored block holds


def test_mutations_give_their_error_codes(exe, tmp_path, good):
    mem, text = good["fastq_level6"]
    muts = B.mutations(mem, text)
    assert len(muts) == 10
    got = run_cases(exe, tmp_path, [(code, m, b"") for _, m, code in muts])
    assert [g[0] for g in got] == [code for _, _, code in muts]


def test_more_invalid_streams(exe, tmp_path):
    """the rest of the core's error list: repeat with nothing before it, an incomplete literal set, symbol 286, distance code 30,
    trailing bytes, a missing end-of-block code when the input ends"""
    cases = S.more_invalid_streams()                               # (the list lives with the other streams: the kernel runs it too)
    got = run_cases(exe, tmp_path, [(code, B.member(raw, zlib.crc32(b"a"), 1), b"") for code, raw in cases])
    assert [g[0] for g in got] == [code for code, _ in cases]
    # zlib does not take any of them for a whole stream either
    for _, raw in cases:
        d = zlib.decompressobj(-15)
        try:
            d.decompress(raw)
            assert not d.eof or d.unused_data
        except zlib.error:
            pass


def test_random_damage_ends_in_the_text_or_an_error(exe, tmp_path, good):
    """2000 seeded byte flips / truncations of three small blocks (stored, fixed, dynamic)"""
    fq = B.fastq_text(1500, seed=9)
    blocks = [(B.deflate_raw(fq[:300], level=0), fq[:300]), (B.deflate_raw(fq[:600], strategy=zlib.Z_FIXED), fq[:600]),
              (B.deflate_raw(fq, level=6), fq)]
    assert [(raw[0] >> 1) & 3 for raw, _ in blocks] == [0, 1, 2]
    rng = np.random.default_rng(2024)
    cases = []
    for i in range(2000):
        raw, text = blocks[i % 3]
        bad = bytearray(raw)
        if i % 5 == 4:
            bad = bad[:int(rng.integers(0, len(bad)))]
        for _ in range(int(rng.integers(0 if i % 5 == 4 else 1, 4))):
            if bad:
                bad[int(rng.integers(0, len(bad)))] ^= int(rng.integers(1, 256))
        cases.append((255, B.member(bytes(bad), zlib.crc32(text), len(text)), text))
    got = run_cases(exe, tmp_path, cases)
    assert sum(1 for code, _, _ in got if code != 0) > 1900         # damage is found, by one check or another
    assert len({code for code, _, _ in got}) >= 6                   # and not always by the same one
