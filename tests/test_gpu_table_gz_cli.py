"""`kreeq validate -o x.kwig.gz|.bed.gz|.csvtable.gz` writes the plain format's bytes as a BGZF file on every path: the device
formatter with the device deflater (KQ_TABLE_DEVICE=1, also with chunks of 7 lines: many short members), the accumulator under
--passes 2 (with KQ_TABLE_DEVICE_PASSES=1), and the host writer through zlib when no knob is set.  In every run gzip reads the
file back to the host writer's plain file, stdout is that run's, the file ends with the end-of-file marker, the project's block
walk accepts the whole file, and --verbose names the side that compressed.  Inputs: the fixtures of tests/test_gpu_table_cli.py and
the synthetic assembly of tests/test_gpu_table_passes_cli.py (whose .kwig takes 20-odd members)."""
import gzip
import os

import pytest

from kreeq_amd import build, capi
from tests.test_gpu_table_passes_cli import BOTH, DEVICE_LINE, HOST_LINE, Bench

pytestmark = pytest.mark.gpu

DEV_GZ_LINE, HOST_GZ_LINE = "per-base table compressed by the device deflater", "per-base table compressed by the host (zlib)"
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MEMBER = 0xff00
MODES = {
    "device": ({"KQ_TABLE_DEVICE": "1"}, [], True),
    "device_chunk7": ({"KQ_TABLE_DEVICE": "1", "KQ_TABLE_CHUNK_LINES": "7"}, [], True),
    "passes": (BOTH, ["--passes", "2"], True),
    "passes_chunk7": (dict(BOTH, KQ_TABLE_CHUNK_LINES="7"), ["--passes", "2"], True),
    "host": ({}, [], False),
    "host_passes": ({}, ["--passes", "2"], False),
}
CASES = [(name, ext, mode) for name in ("decompressor1", "repeat1") for ext in ("kwig", "bed", "csvtable") for mode in MODES] + \
        [("gen21", ext, mode) for ext in ("kwig", "csvtable") for mode in ("device", "passes", "host")]


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    assert os.path.exists(build.LIB), "libkreeq_amd.so must be built in-tree"
    return Bench(build.build_cli(), tmp_path_factory.mktemp("tables_gz"))


@pytest.mark.parametrize("name,ext,mode", CASES)
def test_gz_file_inflates_to_the_plain_format(bench, tmp_path, name, ext, mode):
    env, extra, on_device = MODES[mode]
    want_stdout, want = bench.host(name, False, ext)               # the host writer's plain file and its stdout
    out = str(tmp_path / ("x.%s.gz" % ext))
    so, se, data = bench.run(name, False, out, env, extra)
    assert so == want_stdout
    assert gzip.decompress(data) == want
    assert data[-28:] == EOF_MARKER
    blocks, used = capi.bgzf_scan(data)
    assert used == len(data) and int(blocks[-1]["isize"]) == 0
    assert all(int(b["isize"]) <= MEMBER and int(b["size"]) <= 18 + 5 + int(b["isize"]) + 8 for b in blocks)
    assert sum(int(b["isize"]) for b in blocks) == len(want)
    if on_device:
        assert DEVICE_LINE in se and DEV_GZ_LINE in se and HOST_LINE not in se and HOST_GZ_LINE not in se
    else:
        assert HOST_LINE in se and HOST_GZ_LINE in se and DEVICE_LINE not in se and DEV_GZ_LINE not in se
    if ext == "kwig":                                              # the head line "k\n" is a member of its own
        assert int(blocks[0]["isize"]) == len(want.split(b"\n", 1)[0]) + 1
    if "chunk7" in mode and on_device:
        lines = [l for l in want.split(b"\n")[1 if ext == "kwig" else 0:-1] if not l.startswith(b"fixedStep")]
        assert len(blocks) - 1 >= len(lines) / 7                   # a chunk holds at most 7 positions, and a member no more than a chunk
    if name == "gen21":
        assert len(blocks) > len(want) // MEMBER
        assert len(data) < len(want) // 2                          # digits and separators: far below half on either side


def test_names_that_are_not_compressed_tables(bench, tmp_path):
    """x.bkwig.gz is no format (the summary, no file); x.gfa.gz stays refused"""
    import subprocess

    out = str(tmp_path / "x.bkwig.gz")
    p = subprocess.run([bench.cli, "validate"] + bench.source("repeat1", False) + ["-o", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not os.path.exists(out)
    assert p.stdout == bench.host("repeat1", False, "kwig")[0]
    out = str(tmp_path / "x.gfa.gz")
    p = subprocess.run([bench.cli, "validate"] + bench.source("repeat1", False) + ["-o", out], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and not os.path.exists(out)
