"""The LZ77 parse of k_bgzf_deflate (kreeq_amd/csrc/kq_deflate.h) held to its restatement, tests/deflate_ref.py: for every input
of tests/deflate_cases.py (each built for one edge of the parse, and shown by tests/test_deflate_ref.py to contain it) and for
the formatter's table texts, every member the device writes carries exactly the restated tokens, and is byte for byte the
member the code builder makes of them on the host (tests/native/deflate_tokens_main.cpp): the choice between a dynamic and a
stored block, the header as the device compile of plan_block builds it (two cases reach the 15-bit limit of the code lengths),
CRC, ISIZE and BSIZE.  The bytes are the same at all 16 alignments of the text, with the end of the text on either side of a
16-byte boundary, and at all 16 alignments of the output."""
import pytest

from tests import deflate_cases as DC
from tests import deflate_native as N
from tests import deflate_ref as R
from tests.deflate_tokens import tokens_of
from tests.test_gpu_deflate import PLAIN, db, deflate_dev, kq, members_of, table_texts  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

MEMBER = R.MEMBER
TABLE_NAMES = ["kwig_runs", "bed", "csvtable", "kwig_pieces"]
ALIGN_N = list(range(13, 20)) + list(range(29, 36)) + [MEMBER - 1, MEMBER]
ALIGN_TEXT = PLAIN["fastq"]


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_tokens")
    return N.build(d, sanitize=False), d


@pytest.fixture(scope="module")
def restated(native):
    """{name: [(member text, restated tokens, host member)]} for the cases and the alignment texts, made once"""
    exe, d = native
    texts = {c.name: c.text for c in DC.CASES.values()}
    texts.update({"align_%d" % n: ALIGN_TEXT[:n] for n in ALIGN_N})
    return N.restate(exe, d / "cases", texts)


@pytest.fixture(scope="module")
def restated_tables(native, table_texts):  # noqa: F811
    exe, d = native
    return N.restate(exe, d / "tables", {name: table_texts[name] for name in TABLE_NAMES})


@pytest.fixture(scope="module")
def device_members():
    return {}


def on_device_members(db, cache, name, text):  # noqa: F811
    """the members db.deflate_bgzf makes of the text, one deflate per name"""
    if name not in cache:
        data = db.deflate_bgzf(text)
        cache[name] = [data[int(b["off"]):int(b["off"]) + int(b["size"])] for b in members_of(data)]
    return cache[name]


def check_tokens(name, got, want):
    assert len(got) == len(want), "%s: %d members on the device, %d restated" % (name, len(got), len(want))
    for i, (member, (piece, tokens, made)) in enumerate(zip(got, want)):
        kind, dev = tokens_of(member[18:-8])
        print("%s member %d: %d bytes of text -> %d on the device (%s), %d restated (%s)" % (
            name, i, len(piece), len(member), kind, made.size, "dynamic" if made.dynamic else "stored"))
        if not made.dynamic:
            continue                                                # (a stored member is held to its bytes below)
        assert kind == "dynamic", "%s member %d is %s on the device" % (name, i, kind)
        diff = R.first_difference(piece, tokens, dev)
        assert diff is None, "%s member %d, %s" % (name, i, diff)


def check_bytes(name, got, want):
    assert len(got) == len(want), "%s: %d members on the device, %d restated" % (name, len(got), len(want))
    for i, (member, (_, _, made)) in enumerate(zip(got, want)):
        if member != made.data:
            at = next((j for j, (x, y) in enumerate(zip(member, made.data)) if x != y), min(len(member), len(made.data)))
            raise AssertionError("%s member %d: %d bytes on the device, %d restated, the first difference at byte %d" % (
                name, i, len(member), made.size, at))


@pytest.mark.parametrize("name", DC.NAMES)
def test_tokens(db, restated, device_members, name):  # noqa: F811
    check_tokens(name, on_device_members(db, device_members, name, DC.CASES[name].text), restated[name])


@pytest.mark.parametrize("name", DC.NAMES)
def test_bytes(db, restated, device_members, name):  # noqa: F811
    check_bytes(name, on_device_members(db, device_members, name, DC.CASES[name].text), restated[name])


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_table_tokens(db, table_texts, restated_tables, device_members, name):  # noqa: F811
    check_tokens(name, on_device_members(db, device_members, "table_" + name, table_texts[name]), restated_tables[name])


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_table_bytes(db, table_texts, restated_tables, device_members, name):  # noqa: F811
    check_bytes(name, on_device_members(db, device_members, "table_" + name, table_texts[name]), restated_tables[name])


def test_limits_are_reached(restated):
    """what the byte comparison covers: both block kinds, and 15-bit codes in both sets, as the host builder reports them"""
    assert {restated[name][0][2].dynamic for name in DC.KIND_NAMES} == {False, True}
    assert restated["skewed_literals"][0][2].max_lit_len == 15 and restated["skewed_distances"][0][2].max_dist_len == 15


def at_end_of_allocation(text, offset):
    """device tensor that holds `text` as the LAST bytes of its allocation, the first byte `offset` behind a 16-byte boundary:
    a load behind the text's last 16-byte chunk leaves the allocation"""
    import torch

    buf = torch.empty(offset + len(text), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:]
    view.copy_(torch.frombuffer(bytearray(text), dtype=torch.uint8))
    torch.cuda.synchronize()
    return view


@pytest.mark.parametrize("n", ALIGN_N)
def test_text_alignment(db, restated, n):  # noqa: F811
    text = ALIGN_TEXT[:n]
    (_, _, made), = restated["align_%d" % n]
    for offset in range(16):
        got = deflate_dev(db, text, src=at_end_of_allocation(text, offset))
        assert got == made.data, "n = %d, the text %d bytes behind a 16-byte boundary" % (n, offset)


def test_output_alignment(db):  # noqa: F811
    text = ALIGN_TEXT[:2 * MEMBER + 100]
    want = db.deflate_bgzf(text)
    assert len(members_of(want)) == 3
    for out_offset in range(16):                                    # (deflate_dev checks the guard bytes on both sides)
        assert deflate_dev(db, text, out_offset=out_offset) == want, "the output %d bytes behind a 16-byte boundary" % out_offset
