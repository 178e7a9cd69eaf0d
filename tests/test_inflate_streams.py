"""The hand-built DEFLATE streams of tests/inflate_streams.py on the CPU.  zlib is the reference: it accepts every good case, ends
at the stream's last byte and gives text_of(tokens); it takes no error case for a whole member.  The host compile of the core
(tests/native/inflate_core_main.cpp under -fsanitize=address,undefined, as tests/test_inflate_core_host.py builds it) gives the
same texts and each error case its code.  Every case's predicate holds, with the program's max_len / max_dist where they prove
the edge.  The kernel runs the same list in tests/test_gpu_inflate_streams.py."""
import collections
import struct
import subprocess
import zlib

import pytest

from tests import inflate_streams as S
from tests.test_inflate_core_host import exe  # noqa: F401  (the sanitizer build of the host program)


@pytest.fixture(scope="module")
def report(exe, tmp_path_factory):  # noqa: F811
    """{name: (code, max_len, max_dist, err_name text)} of every case, from one run of the host program, which compares the
    texts itself; the sanitizers found nothing"""
    cases = S.cases()
    path = tmp_path_factory.mktemp("streams") / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            text = c.text if c.code == 0 else b""
            f.write(struct.pack("<III", c.code, len(c.member), len(text)) + c.member + text)
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    lines = p.stdout.strip().split("\n")
    print("\n".join(l for l in lines if ":" in l))
    assert not p.stderr, p.stderr[-4000:]
    rows = [tuple(int(x) for x in l.split()[2:]) for l in lines if l.startswith("case ") and ":" not in l]
    texts = [l.split(" ", 2)[2] for l in lines if l.startswith("name ")]
    assert len(rows) == len(texts) == len(cases)
    out = {c.name: row + (text,) for c, row, text in zip(cases, rows, texts)}
    out["#exit"] = (p.returncode, lines[-1])
    return out


def test_zlib_gives_the_text_of_every_good_case():
    for c in S.good_cases():
        d = zlib.decompressobj(-15)
        text = d.decompress(c.raw)
        assert d.eof and not d.unused_data and not d.unconsumed_tail, c.name
        assert text == c.text, c.name
        if c.tokens is not None:
            assert S.text_of(c.tokens) == text, c.name             # zlib is the reference, not the builder
        assert zlib.decompress(c.member, 31) == text, c.name       # and the member around it is a gzip member


def test_zlib_refuses_every_error_case():
    """as a gzip member: some error cases are whole DEFLATE streams in a member whose ISIZE or CRC-32 is not theirs"""
    for c in S.by_group("errors"):
        d = zlib.decompressobj(31)
        try:
            d.decompress(c.member)
            assert not d.eof or d.unused_data, c.name
        except zlib.error:
            pass
        if c.code not in (11, 13):                                 # (ERR_OUTPUT, ERR_CRC: the trailer's)  the raw stream alone
            d = zlib.decompressobj(-15)
            try:
                d.decompress(c.raw)
                assert not d.eof or d.unused_data, c.name
            except zlib.error:
                pass


def test_host_core_agrees_under_the_sanitizers(report):
    assert report["#exit"] == (0, "0 failures")
    for c in S.cases():
        assert report[c.name][0] == c.code, "%s: code %d, expected %d" % (c.name, report[c.name][0], c.code)


def test_every_error_code_has_a_case_and_the_message_table_is_the_headers(report):
    seen = collections.defaultdict(list)
    for c in S.by_group("errors"):
        seen[c.code].append(c.name)
        assert report[c.name][3] == S.ERR_TEXT[c.code], c.name
    assert sorted(seen) == list(range(1, 14)) == sorted(S.ERR_TEXT)
    assert len(set(S.ERR_TEXT.values())) == 13
    for code, names in sorted(seen.items()):
        print("code %2d  %-40s %s" % (code, S.ERR_TEXT[code], " ".join(names)))


def test_every_predicate_holds(report):
    for c in S.cases():
        _, max_len, max_dist, _ = report[c.name]
        assert c.check(c, max_len, max_dist), c.name


def test_the_limits_are_reached(report):
    """a 15-bit code in each set, used by tokens, and the distance 32 768 copied"""
    _, max_len, max_dist, _ = report["deep_codes_far_distances"]
    print("deep_codes_far_distances: max_len %d, max_dist %d" % (max_len, max_dist))
    assert (max_len, max_dist) == (15, 32768)
    assert report["copy_65536_last_258_32768"][2] == 32768
    c, = S.by_group("deep")
    ll, dl = c.blocks[0]["ll"], c.blocks[0]["dl"]
    ls, ds = S.used(c.tokens)
    assert sorted(s for s in ls if ll[s] == 15) == [284, 285] and sorted(d for d in ds if dl[d] == 15) == [14, 29]


def test_the_case_list_is_the_issues():
    groups = collections.Counter(c.group for c in S.cases())
    print(dict(groups), "largest members:", sorted((len(c.member) for c in S.cases()), reverse=True)[:4])
    assert set(groups) == set(S.GROUPS)
    copies = {(t[0], t[1]) for c in S.by_group("copies") for t in c.tokens if len(t) > 1}
    assert copies >= {(L, d) for L in S.COPY_LENGTHS for d in range(1, 71)}
    assert copies >= {(L, L + e) for L in S.COPY_LENGTHS for e in (-1, 0, 1) if L + e > 0}
    sizes = {len(c.raw) for c in S.by_group("input_geometry")}
    assert sizes >= {2, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, S.MAX_DATA}
    for edge in (1024, 2048, 3072):                                # and each edge at every lead of the kernel's aligned view
        assert sizes >= {edge - lead for lead in range(16)}
    assert {len(c.text) for c in S.by_group("output_geometry")} == set(S.OUT_SIZES)
    assert all(len(c.member) <= 65536 for c in S.cases())


def test_out_copy_index_rule_is_what_the_copy_cases_need():
    """the kernel's out_copy splits a match over 64 lanes: byte j comes from pos - dist + (j if dist >= len else j % dist).  That
    rule, restated here, gives text_of for every copy case; without the `% dist` it does not: the cases can tell"""
    def by_rule(tokens, broken):
        out = bytearray()
        for t in tokens:
            if len(t) == 1:
                out.append(t[0])
                continue
            pos, (n, dist) = len(out), t[:2]
            out += bytes(n)
            for step in range(0, n, 64):                           # the 64 lanes load, then the 64 lanes store
                js = range(step, min(step + 64, n))
                loaded = [out[pos - dist + (j if dist >= n or broken else j % dist)] for j in js]
                out[pos + step:pos + step + len(js)] = bytes(loaded)
        return bytes(out)
    caught = []
    for c in S.by_group("copies"):
        assert by_rule(c.tokens, False) == c.text, c.name
        if by_rule(c.tokens, True) != c.text:
            caught.append(c.name)
    print("without `% dist`:", " ".join(caught))
    assert len(caught) >= len(S.COPY_LENGTHS)
