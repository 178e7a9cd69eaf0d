"""The suite's own tools for the device deflate parse, checked without a GPU: the token reader (tests/deflate_tokens.py)
against zlib's streams, and the restated parse (tests/deflate_ref.py) on every input of tests/deflate_cases.py: its tokens
are valid and spell the text, every case's predicate holds (the edge the case was built for IS in the restated tokens), and
the member the code builder makes of them (tests/native/deflate_tokens_main.cpp, under the address and undefined-behaviour
sanitizers) is read by zlib, is no larger than the stored form, and gives the tokens back.  tests/test_gpu_deflate_parse.py
then holds the device to these tokens and members."""
import time
import zlib

import pytest

from tests import deflate_cases as DC
from tests import deflate_native as N
from tests import deflate_ref as R
from tests import test_gpu_deflate as G
from tests.deflate_tokens import tokens_of

MEMBER = R.MEMBER


@pytest.fixture(scope="module")
def restated(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_tokens")
    exe = N.build(d, sanitize=True)
    return N.restate(exe, d / "members", {c.name: c.text for c in DC.CASES.values()})


def zlib_raw(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(text) + c.flush()


def all_texts():
    t = {"plain_" + k: v for k, v in G.PLAIN.items()}
    t.update({c.name: c.text for c in DC.CASES.values()})
    return t


def test_token_reader_against_zlib():
    """every text, as zlib codes it at levels 1, 6, 9 and with fixed codes: the tokens spell the text and are DEFLATE's"""
    kinds = set()
    for name, text in all_texts().items():
        for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)):
            kind, tokens = tokens_of(zlib_raw(text, level, strategy))
            kinds.update(kind.split("+"))
            assert R.expand(tokens) == text, (name, level)
            assert all(len(t) == 1 or (3 <= t[0] <= 258 and 1 <= t[1] <= 32768) for t in tokens), (name, level)
            if strategy == zlib.Z_FIXED:
                assert "dynamic" not in kind, (name, kind)          # (fixed codes, or stored where that is shorter)
    assert kinds == {"stored", "fixed", "dynamic"}


def test_token_reader_refuses_damage():
    raw = zlib_raw(b"abcabcabcabc" * 20, 6)
    with pytest.raises(AssertionError):
        tokens_of(raw[:-2])
    with pytest.raises(AssertionError):
        tokens_of(raw + b"\0\0")
    with pytest.raises(AssertionError):
        tokens_of(b"\x07")                                          # block type 3


@pytest.mark.parametrize("name", DC.NAMES)
def test_restated_tokens(restated, name):
    case = DC.CASES[name]
    members = restated[name]
    assert b"".join(m[0] for m in members) == case.text
    for i, (piece, tokens, made) in enumerate(members):
        R.check_tokens(piece, tokens)
        assert zlib.decompress(made.data, 31) == piece, (name, i)
        assert made.size == len(made.data) <= 18 + 5 + len(piece) + 8, (name, i)
        kind, back = tokens_of(made.data[18:-8])
        assert kind == ("dynamic" if made.dynamic else "stored"), (name, i)
        assert made.dynamic or not DC.must_be_coded(name, len(piece)), "%s member %d is stored: its tokens would never be compared" % (name, i)
        assert back == (tokens if made.dynamic else [(b,) for b in piece]), (name, i, R.first_difference(piece, tokens, back))
        print("%s member %d: %d bytes of text -> %d, %s, code lengths up to %d / %d, longest token %d bits" % (
            name, i, len(piece), made.size, kind, made.max_lit_len, made.max_dist_len, made.max_token_bits))
    case.check([R.parse_at(m[0]) for m in members], [m[2] for m in members])


def test_both_kinds_of_block_occur(restated):
    kinds = {restated[name][0][2].dynamic for name in DC.KIND_NAMES}
    assert kinds == {False, True}


def test_every_edge_family_is_present():
    for prefix in ("quick_", "end_n", "step_geometry", "window_32768", "window_32769", "too_far", "in_step_", "insert_order", "hash_collision",
                   "skewed_literals", "skewed_distances", "kind_", "member_boundary", "fastq"):
        assert any(n.startswith(prefix) for n in DC.NAMES), prefix
    for n in DC.END_N:                                              # every end at every n; 258 bytes only where the text has them
        lefts = [l for l in DC.END_LEFT if "end_n%d_left%d" % (n, l) in DC.CASES]
        assert lefts == [l for l in DC.END_LEFT if l < n]


def test_a_full_member_restates_quickly():
    text = DC.CASES["fastq"].text[:MEMBER]
    t0 = time.perf_counter()
    R.parse_steps(text)
    assert time.perf_counter() - t0 < 5.0


def test_ratio_record(restated):
    """A record, not an assertion: the restated (= the device's) member sizes of the FASTQ text beside zlib level 1's."""
    ours = theirs = 0
    for i, (piece, _, made) in enumerate(restated["fastq"]):
        level1 = len(zlib_raw(piece, 1)) + 26
        print("fastq member %d: %d bytes of text, restated %d, zlib level 1 %d (%.3f x)" % (i, len(piece), made.size, level1, made.size / level1))
        ours += made.size
        theirs += level1
    print("fastq: restated %d, zlib level 1 %d (%.3f x)" % (ours, theirs, ours / theirs))
