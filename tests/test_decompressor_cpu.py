"""`kreeq-decompressor lookup` runs without a GPU: it replays the reference's golden (validateFiles/test.48.tst), takes a
positional coordinate and a span like tests/table_ref.py, and refuses what the reference crashes on."""
import os
import subprocess

import pytest

from kreeq_amd import build
from tests import helpers as H
from tests import table_ref as T

BKWIG = H.golden_input("decompressor1.bkwig")


@pytest.fixture(scope="module")
def exe():
    build.build_lib()
    return build.build_decompressor()


def run(exe, args):
    return subprocess.run([exe] + args, capture_output=True, timeout=60)


def lines_of(text):
    out = text.decode().split("\n")
    while out and out[-1] == "":
        out.pop()
    return out


def test_lookup_golden(exe):
    argv, expected = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", "test.48.tst"))
    p = run(exe, [H.golden_input(a) if a.startswith("testFiles/") else a for a in argv[1:]])
    assert p.returncode == 0, p.stderr
    assert lines_of(p.stdout) == expected


def test_positional_coordinate(exe):
    p = run(exe, ["lookup", "-i", BKWIG, "sequence1:20-30"])
    assert p.returncode == 0, p.stderr
    assert p.stdout == T.lookup(open(BKWIG, "rb").read(), [(b"sequence1", 20, 30)])
    _, expected = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", "test.48.tst"))
    assert lines_of(p.stdout) == expected[:expected.index("")]             # the golden's first block


def test_span(exe):
    p = run(exe, ["lookup", "-i", BKWIG, "-c", H.golden_input("decompressor1.bed"), "-s", "2"])
    assert p.returncode == 0, p.stderr
    ranges = [(w[0].encode(), int(w[1]), int(w[2])) for w in (l.split() for l in open(H.golden_input("decompressor1.bed"))) if w]
    assert p.stdout == T.lookup(open(BKWIG, "rb").read(), ranges, span=2)
    assert b"sequence1:18-32\n" in p.stdout


@pytest.mark.parametrize("coord,first_line", [("sequence3:40-60", "sequence3:40-47"), ("sequence3:40-46", "sequence3:40-46"), ("sequence3:40-47", "sequence3:40-47")])
def test_payload_start_quirk(exe, coord, first_line):
    """the reference's offset arithmetic as written: a range that overhangs its component (or ends exactly at its end) is clamped
    and read from the start of the payload; one that ends inside is read where it lies"""
    header, rng = coord.split(":")
    begin, end = (int(x) for x in rng.split("-"))
    p = run(exe, ["lookup", "-i", BKWIG, coord])
    assert p.returncode == 0, p.stderr
    data = open(BKWIG, "rb").read()
    assert p.stdout == T.lookup(data, [(header.encode(), begin, end)])
    assert lines_of(p.stdout)[1] == first_line
    b = T.Bkwig(data)
    quirk = end - 1 >= 46                                                  # sequence3's first component: positions 0..45
    at = 0 if quirk else dict(b.paths)[b"sequence3"][0][3] // 12 + begin - 1
    assert lines_of(p.stdout)[2] == "%d,%d,%d" % tuple(b.triples()[at])


@pytest.mark.parametrize("args", [["lookup", "-i", BKWIG, "nobody:1-5"],                      # an unknown header
                                  ["lookup", "-i", BKWIG, "sequence1:1000000-1000005"],        # a start outside every component
                                  ["lookup", "-i", BKWIG, "sequence1:2-9", "-s", "5"],         # begin - span < 1
                                  ["lookup", "sequence1:20-30"],                               # no -i
                                  ["lookup", "--expand", "-i", BKWIG, "sequence1:20-30"]])
def test_refusals(exe, args):
    p = run(exe, args)
    assert p.returncode != 0
    assert p.stderr.strip()
