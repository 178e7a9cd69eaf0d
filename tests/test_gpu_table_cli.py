"""`kreeq validate -o x.kwig|.bkwig|.bed|.csvtable` with KQ_TABLE_DEVICE=1 writes the bytes of the host writers (also with
chunks of 7 lines, and the committed .bkwig fixtures), says which side wrote, and leaves map-range passes to the host; and
`kreeq-decompressor inflate` turns our .bkwig back into our .kwig / .csvtable through the device formatter."""
import os
import subprocess

import pytest

from kreeq_amd import build
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEVICE_LINE, HOST_LINE = "per-base table written by the device formatter", "per-base table written by the host writer"
PAIRS = {"decompressor1": ("decompressor1.fasta", "random1.fastq", "decompressor1.bkwig"), "repeat1": ("repeat1.fasta", "repeat1.fastq", "decompressor2.bkwig")}
EXTS = ("kwig", "bkwig", "bed", "csvtable")


@pytest.fixture(scope="module")
def tools():
    assert os.path.exists(build.LIB), "libkreeq_amd.so must be built in-tree"
    return build.build_cli(), build.build_decompressor()


def validate(cli, pair, out, device=False, chunk=None, extra=()):
    """-> (stdout, stderr) of one validate run that writes `out`"""
    asm, reads, _ = PAIRS[pair]
    env = {k: v for k, v in os.environ.items() if k not in ("KQ_TABLE_DEVICE", "KQ_TABLE_CHUNK_LINES")}
    if device:
        env["KQ_TABLE_DEVICE"] = "1"
    if chunk:
        env["KQ_TABLE_CHUNK_LINES"] = str(chunk)
    p = subprocess.run([cli, "validate", "-f", H.golden_input(asm), "-r", H.golden_input(reads), "-o", out, "--verbose"] + list(extra),
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr
    return p.stdout, p.stderr


@pytest.fixture(scope="module")
def files(tools, tmp_path_factory):
    """every (pair, extension) written by the host writers and by the device formatter -> {(pair, ext): (host, device) bytes}"""
    d = tmp_path_factory.mktemp("tables")
    out = {}
    for pair in PAIRS:
        for ext in EXTS:
            host, dev = str(d / ("%s.host.%s" % (pair, ext))), str(d / ("%s.dev.%s" % (pair, ext)))
            so, se = validate(tools[0], pair, host)
            do, de = validate(tools[0], pair, dev, device=True)
            assert so == do                                               # stdout is the same in both modes
            assert HOST_LINE in se and DEVICE_LINE not in se
            assert DEVICE_LINE in de and HOST_LINE not in de
            out[(pair, ext)] = (open(host, "rb").read(), open(dev, "rb").read(), dev)
    return out


@pytest.mark.parametrize("ext", EXTS)
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_device_files_equal_host_files(tools, files, tmp_path, pair, ext):
    host, dev, _ = files[(pair, ext)]
    assert len(host) > 20 and dev == host
    small = str(tmp_path / ("chunks." + ext))
    validate(tools[0], pair, small, device=True, chunk=7)
    assert open(small, "rb").read() == host
    if ext == "bkwig":
        assert dev == open(H.golden_input(PAIRS[pair][2]), "rb").read()


@pytest.mark.parametrize("ext", EXTS)
def test_map_range_passes_use_the_host_writer(tools, files, tmp_path, ext):
    out = str(tmp_path / ("passes." + ext))
    _, err = validate(tools[0], "repeat1", out, device=True, extra=["--passes", "2"])
    assert HOST_LINE in err and DEVICE_LINE not in err
    assert open(out, "rb").read() == files[("repeat1", ext)][0]


def inflate(tools, args):
    return subprocess.run([tools[1], "inflate"] + args, capture_output=True, timeout=120)


def test_inflate_golden(tools):
    argv, expected = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", "test.49.tst"))
    p = subprocess.run([tools[1]] + [H.golden_input(a) if a.startswith("testFiles/") else a for a in argv[1:]], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    out = p.stdout.split("\n")
    while out and out[-1] == "":
        out.pop()
    assert out == expected


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_inflate_round_trip(tools, files, pair):
    bkwig = files[(pair, "bkwig")][2]
    p = inflate(tools, ["-i", bkwig])
    assert p.returncode == 0, p.stderr
    assert p.stdout == files[(pair, "kwig")][0]
    p = inflate(tools, ["-i", bkwig, "--expand"])
    assert p.returncode == 0, p.stderr
    assert p.stdout == files[(pair, "csvtable")][0]
    env = dict(os.environ, KQ_TABLE_CHUNK_LINES="7")                      # chunk edges inside components
    q = subprocess.run([tools[1], "inflate", "-i", bkwig, "--expand"], capture_output=True, timeout=120, env=env)
    assert q.returncode == 0 and q.stdout == p.stdout


def test_inflate_truncated(tools, files, tmp_path):
    cut = tmp_path / "cut.bkwig"
    cut.write_bytes(files[("repeat1", "bkwig")][0][:-5])
    p = inflate(tools, ["-i", str(cut)])
    assert p.returncode != 0 and p.stdout == b"Error: file truncated\n"
