"""The GPU-free part of the CLI's BGZF reader (kreeq_amd/host/bgzf_reader.h) as a stand-alone host program under
-fsanitize=address,undefined (tests/native/bgzf_reader_main.cpp).  The run cutter on member lists made by tests/bgzf_inputs.py --
a 3000-read stream file with empty members, a file of the EOF marker alone, one maximal member, 300 members -- at
capacities of 65 536, 65 537, 1 MiB and the sum of all sizes: the program checks that every member lies in exactly one run,
that runs are contiguous, in order, never empty, never above the capacity and as long as the capacity allows, and that the
rebased offsets start at 0; this file checks the totals against a member walk in Python.  A capacity of 65 535 is refused.
And the first-member test that decides whether a file takes the device path: a BGZF file does, plain gzip, an empty file
and a BGZF file cut inside its first header do not.  Last, the reader itself (bgzf_reader.cpp, linked into the same program with
the block walk in place of the library) into a sink of heap buffers of exactly the capacity: every run is the next piece of the
file with the list a scan of it finds, only the final run is marked last, members without text in front of the first text are
dropped, files it does not take are handed back untouched, and its two errors name what they should -- also with more
members in one buffer's worth than the reader's member list holds at first (7000 of about 90 bytes), alone and in front of a
plain gzip member."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import bgzf_inputs as B
from tests import helpers as H


def stream_input(kind):
    """-> text: about 3000 FASTQ reads (bgzf_inputs.fastq_text, cut behind its last whole record), the same with CRLF line ends and
    no final line end, or 3000 wrapped FASTA records"""
    if kind == "fasta":
        rng = np.random.default_rng(8)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        out = []
        for i in range(3000):
            sb = bytes(rng.choice(acgt, 150).tolist())
            out.append(b">r%d wrapped\n" % i + sb[:60] + b"\n" + sb[60:120] + b"\n" + sb[120:] + b"\n")
        return b"".join(out)
    text = B.fastq_text(750_000, seed=6)
    text = text[:text.rindex(b"\n@read") + 1]
    assert text.count(b"\n") % 4 == 0 and text.count(b"\n") // 4 > 2900
    return text if kind == "fastq_nl" else text.replace(b"\n", b"\r\n")[:-2]


def stream_cuts(kind):
    """seeded block boundaries 1..5000 text bytes apart"""
    text = stream_input(kind)
    rng = np.random.default_rng(len(kind))
    cuts, c = [], int(rng.integers(1, 5001))
    while c < len(text):
        cuts.append(c)
        c += int(rng.integers(1, 5001))
    return cuts


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path_factory.mktemp("bgzf_reader") / "bgzf_reader")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(H.ROOT, "kreeq_amd", "host"), "-I", os.path.join(H.ROOT, "kreeq_amd", "csrc"), "-I", os.path.join(H.ROOT, "include"),
                           "-o", path, os.path.join(H.ROOT, "tests", "native", "bgzf_reader_main.cpp"), os.path.join(H.ROOT, "kreeq_amd", "host", "bgzf_reader.cpp"), "-lz"])
    return path


def run(exe, args):
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-4000:]
    lines = p.stdout.strip().split("\n")
    assert lines[-1] == "0 failures"
    return lines[:-1]


def files():
    good = B.good_blocks()
    text = stream_input("fastq_nl")
    cuts = stream_cuts("fastq_nl")
    rng = np.random.default_rng(300)
    names = sorted(good)
    return {
        "stream": B.bgzf_file(text, cuts=cuts, empty_at=tuple(range(3, len(cuts), 17))),
        "eof_only": B.EOF_BLOCK,
        "one_maximal": good["stored_max"][0],
        "members_300": b"".join(good[names[int(i)]][0] for i in rng.integers(0, len(names), 300)),
    }


@pytest.mark.parametrize("name", ["stream", "eof_only", "one_maximal", "members_300"])
def test_run_cutter(exe, tmp_path, name):
    data = files()[name]
    members = B.blocks_of(data)
    sizes = [m[1] for m in members]
    assert sum(sizes) == len(data)
    if name == "stream":
        assert sum(1 for m in members if m[5] == 0) > 5
    if name == "one_maximal":
        assert sizes == [65536]
    if name == "members_300":
        assert len(members) == 300 and len(data) > (1 << 20)
    path = tmp_path / (name + ".gz")
    path.write_bytes(data)
    caps = [65535, 65536, 65537, 1 << 20, len(data)]
    lines = run(exe, ["cut", path] + caps)
    assert len(lines) == len(caps)
    for cap, line in zip(caps, lines):
        if cap < 65536:                                     # (the EOF marker alone: the sum of all sizes is 28)
            assert line == "cap %d refused" % cap
            continue
        m = re.fullmatch(r"cap (\d+) runs (\d+) members (\d+) bytes (\d+)", line)
        assert m, line
        c, runs, n, nbytes = (int(x) for x in m.groups())
        assert (c, n, nbytes) == (cap, len(members), len(data))
        # the greedy cut in Python: the same number of runs
        want, fill = 0, None
        for s in sizes:
            if fill is None or fill + s > cap:
                want, fill = want + 1, 0
            fill += s
        assert runs == want
        if cap >= len(data):
            assert runs == 1


def test_first_member(exe, tmp_path):
    text = B.fastq_text(200_000)
    bgzf = B.bgzf_file(text)
    first_size = B.blocks_of(bgzf)[0][1]
    cases = {
        "bgzf": (bgzf, 1),
        "bgzf_small_members": (B.bgzf_file(text[:5000], cuts=list(range(100, 5000, 100))), 1),
        "bgzf_first_member_only": (bgzf[:first_size], 1),
        "plain_gzip": (gzip.compress(text), 0),
        "empty": (b"", 0),
        "cut_in_first_header": (bgzf[:11], 0),
        "cut_in_first_extra_field": (bgzf[:15], 0),
        "cut_in_first_member": (bgzf[:first_size - 1], 0),
    }
    for name, (data, want) in cases.items():
        path = tmp_path / (name + ".gz")
        path.write_bytes(data)
        assert run(exe, ["first", path]) == ["first %d" % want], name


def read_through(exe, tmp_path, name, data, cap):
    path = tmp_path / (name + ".gz")
    path.write_bytes(data)
    lines = run(exe, ["read", path, cap])
    runs = [tuple(int(x) for x in re.fullmatch(r"run len (\d+) blocks (\d+) text (\d+) fastq (\d) last (\d)", l).groups()) for l in lines[:-1]]
    return runs, lines[-1]


def test_reader_submits_the_file_in_order(exe, tmp_path):
    fq = stream_input("fastq_crlf_open")
    fa = stream_input("fasta")
    cuts = stream_cuts("fastq_crlf_open")
    for name, data, text, fastq in [
        ("fastq", B.bgzf_file(fq, cuts=cuts, empty_at=tuple(range(3, len(cuts), 17))), fq, 1),
        ("fasta_no_eof", B.bgzf_file(fa, eof=False), fa, 0),
        ("empty_members_first", B.EOF_BLOCK * 3 + B.bgzf_file(fa), fa, 0),
        ("two_files", B.bgzf_file(fq[:len(fq) // 2]) + B.bgzf_file(fq[len(fq) // 2:]), fq, 1),
    ]:
        for cap in (65536, 100_000, 1 << 20, 64 << 20):
            runs, end = read_through(exe, tmp_path, name, data, cap)
            assert end == "done"
            assert sum(r[2] for r in runs) == len(text)
            assert all(r[0] <= cap and r[3] == fastq for r in runs)
            assert [r[4] for r in runs] == [0] * (len(runs) - 1) + [1]
            if cap >= len(data):
                assert len(runs) == 1
            else:
                assert len(runs) >= len(data) // cap


def test_reader_leaves_other_files_to_the_host(exe, tmp_path):
    text = B.fastq_text(100_000)
    for name, data in [
        ("plain_gzip", gzip.compress(text)),
        ("not_fastx", B.bgzf_file(b"H\tVN:Z:1.0\nS\t1\tACGT\n")),
        ("not_fastx_behind_empty_members", B.EOF_BLOCK * 2 + B.bgzf_file(b"#comment\n" + text)),
    ]:
        assert read_through(exe, tmp_path, name, data, 1 << 20) == ([], "fallback"), name
    # no members with text at all: taken, and nothing is submitted
    assert read_through(exe, tmp_path, "eof_only", B.EOF_BLOCK, 1 << 20) == ([], "done")
    assert read_through(exe, tmp_path, "empty_only", B.EOF_BLOCK * 5000, 65536) == ([], "done")


def test_reader_errors(exe, tmp_path):
    text = B.fastq_text(400_000)
    good = B.bgzf_file(text, eof=False)
    members = B.blocks_of(good)
    # the file ends inside its last member
    runs, end = read_through(exe, tmp_path, "truncated", good[:-100], 100_000)
    assert end.startswith("error: ") and "truncated BGZF file" in end and "byte %d " % members[-1][0] in end
    assert runs and all(r[4] == 0 for r in runs)
    # a plain gzip member behind the BGZF members: named by its offset in the file
    runs, end = read_through(exe, tmp_path, "gzip_behind", good + gzip.compress(b"@x\nACGT\n+\nIIII\n"), 100_000)
    assert end.startswith("error: ") and "byte %d " % len(good) in end and "not a BGZF block" in end
    # a pool buffer that cannot hold a member
    runs, end = read_through(exe, tmp_path, "small_buffers", good, 65535)
    assert end.startswith("error: ") and "cannot hold a BGZF member" in end


def test_reader_more_members_than_its_list_holds(exe, tmp_path):
    """7000 members of a few records each in ONE window: the member list (4096 entries at first) grows, whether the scan stops at
    the end of the file, inside a member, or at a member that is not BGZF (where it reports the count, not a capacity error)"""
    text = B.fastq_text(420_000, seed=9)
    text = text[:text.rindex(b"\n@read") + 1]
    many = B.bgzf_file(text, level=1, cuts=list(range(60, len(text), 60)), eof=False)
    members = B.blocks_of(many)
    assert len(members) > 6500 and len(many) < (4 << 20)
    runs, end = read_through(exe, tmp_path, "many", many, 32 << 20)
    assert end == "done" and runs == [(len(many), len(members), len(text), 1, 1)]
    # behind them a plain gzip member: the BGZF members are submitted, then the foreign one is named by its offset
    runs, end = read_through(exe, tmp_path, "many_gzip_behind", many + gzip.compress(b"@x\nACGT\n+\nIIII\n"), 32 << 20)
    assert runs == [(len(many), len(members), len(text), 1, 0)]
    assert end.startswith("error: ") and "byte %d " % len(many) in end and "not a BGZF block" in end
    # the file ends inside the last of them
    runs, end = read_through(exe, tmp_path, "many_truncated", many[:-5], 32 << 20)
    assert runs == [(members[-1][0], len(members) - 1, len(text) - members[-1][5], 1, 0)]
    assert end.startswith("error: ") and "truncated BGZF file" in end and "byte %d " % members[-1][0] in end
