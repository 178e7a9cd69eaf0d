"""k_bgzf_inflate (kreeq_amd/csrc/kq_bgzf.h) on the hand-built DEFLATE streams of tests/inflate_streams.py, through
KreeqDB.inflate_bgzf_dev only: every good case byte for byte against zlib's text, with guard bytes on both sides; the
input-geometry members with the compressed file at all 16 offsets from a 16-byte boundary and as the last bytes of its allocation;
the output-geometry members at all 16 destination alignments; every error case refused with its member named, its err_name text
in the message, nothing stored for it and its neighbours whole; the members the project's own code builder makes of the inputs of
tests/deflate_cases.py (distances up to 32 768, 15-bit codes in both sets); and the device writer's 4096-member batch boundary,
read back by the device inflater.  tests/test_inflate_streams.py holds the same list to zlib and the host compile of the core."""
import time
import zlib

import numpy as np
import pytest

from tests import bgzf_inputs as B
from tests import deflate_cases as DC
from tests import deflate_native as N
from tests import inflate_streams as S

pytestmark = pytest.mark.gpu

GUARD = 0x5A
MEMBER = 0xff00


@pytest.fixture(scope="module")
def kq():
    import kreeq_amd

    if not kreeq_amd.device_available():
        pytest.fail("no gfx950 device: the product path has no CPU fallback")
    return kreeq_amd


@pytest.fixture(scope="module")
def db(kq):
    return kq.KreeqDB(21, 128, device=0, capacity_hint=1024)


@pytest.fixture(scope="module")
def reference():
    """{name: zlib's text} of every good case, made once"""
    out = {}
    for c in S.good_cases():
        d = zlib.decompressobj(-15)
        out[c.name] = d.decompress(c.raw)
        assert d.eof and not d.unused_data, c.name
    return out


def scan(data, cap=None):
    from kreeq_amd import capi

    blocks, used = capi.bgzf_scan(data, cap)
    assert used == len(data)
    return blocks


def at_end_of_allocation(data, offset):
    """device tensor that holds `data` as the LAST bytes of its allocation, the first byte `offset` behind a 16-byte boundary"""
    import torch

    buf = torch.empty(offset + len(data), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:]
    view.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    torch.cuda.synchronize()
    return view


def inflate_guarded(db, data, blocks, comp_offset=0, text_offset=0):
    """-> the guarded output buffer as numpy, the text's offset in it and its size"""
    import torch

    comp = at_end_of_allocation(data, comp_offset)
    n = db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, None, 0)
    lo = 16 + text_offset
    out = torch.full((lo + n + 48,), GUARD, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    assert db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, out.data_ptr() + lo, n) == n
    return out.cpu().numpy(), lo, n


def check_members(db, items, comp_offset=0, text_offset=0, what=""):
    """items: [(name, member, text)] inflated in one call: member i lands at the sum of the sizes before it"""
    data = b"".join(m for _, m, _ in items)
    blocks = scan(data)
    assert len(blocks) == len(items)
    got, lo, n = inflate_guarded(db, data, blocks, comp_offset, text_offset)
    assert n == sum(len(t) for _, _, t in items)
    assert (got[:lo] == GUARD).all() and (got[lo + n:] == GUARD).all(), "guard bytes overwritten %s" % what
    at = lo
    for name, _, text in items:
        piece = got[at:at + len(text)]
        if piece.tobytes() != text:
            bad = np.flatnonzero(piece != np.frombuffer(text, dtype=np.uint8))
            raise AssertionError("%s %s: %d of %d bytes differ, the first at %d" % (name, what, len(bad), len(text), int(bad[0])))
        at += len(text)


def items_of(cases, reference):
    return [(c.name, c.member, reference[c.name]) for c in cases]


# ------------------------------------------------------------------------------------------------------------ good cases
@pytest.mark.parametrize("group", [g for g in S.GROUPS if g != "errors"])
def test_group_gives_zlibs_text(db, reference, group):
    cases = S.by_group(group)
    assert cases and all(c.code == 0 for c in cases)
    check_members(db, items_of(cases, reference), comp_offset=3, text_offset=5)


def test_every_good_case_in_one_call(db, reference):
    cases = S.good_cases()
    assert len(cases) > 250
    check_members(db, items_of(cases, reference), comp_offset=9, text_offset=11)


def test_input_geometry_at_all_16_leads(db, reference):
    """the compressed file at every offset from a 16-byte boundary, its last member's trailer the last bytes of the allocation: with
    the members byte-packed behind each other, each data_len meets each lead of the kernel's aligned view many times over"""
    items = items_of(S.by_group("input_geometry"), reference)
    leads = set()
    for offset in range(16):
        check_members(db, items, comp_offset=offset, text_offset=offset, what="(file %d bytes behind a 16-byte boundary)" % offset)
        at = offset
        for _, m, _ in items:
            leads.add((len(m) - 26, (at + 18) % 16))
            at += len(m)
    for edge in (1024, 2048, 3072):                                # data_len + lead on the chunk edge and on either side, at every lead
        for lead in range(16):
            assert {(edge - lead + d, lead) for d in (-1, 0, 1)} <= leads
    # and each member alone, so that its data is what ends the allocation (8 trailer bytes behind it)
    for name, m, text in items[:1] + [i for i in items if len(i[1]) - 26 in (1023, 1024, 1025, 2048, 3072, S.MAX_DATA)]:
        for offset in (0, 7, 15):
            check_members(db, [(name, m, text)], comp_offset=offset, what="(alone, offset %d)" % offset)


def test_output_geometry_at_all_16_alignments(db, reference):
    """member i lands at the sum of the sizes before it; with the first destination at each of 16 alignments every ISIZE meets
    every alignment of the head / vector / tail store"""
    items = items_of(S.by_group("output_geometry"), reference)
    seen = set()
    for offset in range(16):
        check_members(db, items, comp_offset=offset % 4, text_offset=offset, what="(text %d bytes behind a 16-byte boundary)" % offset)
        at = offset
        for _, _, text in items:
            seen.add((len(text), at % 16))
            at += len(text)
    assert seen == {(n, a) for n in S.OUT_SIZES for a in range(16)}
    for name, m, text in items:                                    # and alone: nothing before it, nothing behind it but the guard
        if len(text) in (0, 1, 15, 16, 17, 63, 64, 65, 65535, 65536):
            for offset in (0, 1, 15):
                check_members(db, [(name, m, text)], text_offset=offset, what="(alone, text offset %d)" % offset)


# ---------------------------------------------------------------------------------------------------------------- errors
def test_every_error_case_is_refused_in_the_middle(kq, db, reference):
    import torch

    by_name = {c.name: c for c in S.good_cases()}
    first, last = by_name["copy_len65_dist1to70"], by_name["blocks_200_mixed"]
    t0, t2 = reference[first.name], reference[last.name]
    errors = S.by_group("errors")
    assert sorted({c.code for c in errors}) == list(range(1, 14))
    failures = []
    for c in errors:
        data = first.member + c.member + last.member
        blocks = scan(data)
        assert len(blocks) == 3
        n0, n1, n2 = (int(b["isize"]) for b in blocks)
        assert (n0, n2) == (len(t0), len(t2))
        comp = at_end_of_allocation(data, 1)
        out = torch.full((16 + n0 + n1 + n2 + 48,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(kq.KqError) as e:
            db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, out.data_ptr() + 16, n0 + n1 + n2)
        got = out.cpu().numpy()
        msg = str(e.value)
        print("%-40s %s" % (c.name, msg))
        if not (e.value.code == -1 and "block 1 " in msg and S.ERR_TEXT[c.code] in msg):
            failures.append("%s: expected '%s', got %d '%s'" % (c.name, S.ERR_TEXT[c.code], e.value.code, msg))
        if not ((got[:16] == GUARD).all() and (got[16 + n0 + n1 + n2:] == GUARD).all()):
            failures.append("%s: guard bytes overwritten" % c.name)
        if not (got[16 + n0:16 + n0 + n1] == GUARD).all():
            failures.append("%s: the failed member stored something" % c.name)
        if got[16:16 + n0].tobytes() != t0 or got[16 + n0 + n1:16 + n0 + n1 + n2].tobytes() != t2:
            failures.append("%s: a neighbour's text is not whole" % c.name)
        # the same handle then decodes a good file
        check_members(db, [(first.name, first.member, t0), (last.name, last.member, t2)], comp_offset=2, what="(after %s)" % c.name)
    assert not failures, "\n".join(failures)


def test_the_first_of_all_error_cases_is_the_one_reported(kq, db, reference):
    """every error case in ascending order of its code, each behind 70 good members (more than one member per compute unit slot
    ahead of each): block 70 is reported, with the first case's text"""
    filler = [c for c in S.good_cases() if c.group in ("headers", "copies") and len(c.member) < 4000]
    assert len(filler) >= 15
    errors = sorted(S.by_group("errors"), key=lambda c: c.code)
    parts = []
    for i, c in enumerate(errors):
        parts += [filler[(i + j) % len(filler)].member for j in range(70)] + [c.member]
    data = b"".join(parts)
    blocks = scan(data)
    assert len(blocks) == 71 * len(errors)
    with pytest.raises(kq.KqError) as e:
        inflate_guarded(db, data, blocks)
    assert e.value.code == -1 and "block 70 " in str(e.value) and S.ERR_TEXT[errors[0].code] in str(e.value), str(e.value)
    check_members(db, items_of(filler, reference))


# ------------------------------------------------------------------------------------------------ the project's own members
def test_members_of_the_projects_code_builder(db, tmp_path_factory):
    """the host-built members of every input of tests/deflate_cases.py (byte for byte what the device writer makes of them, as
    tests/test_gpu_deflate_parse.py shows), concatenated and inflated in one call: window_32768_*, skewed_distances and
    skewed_literals come through the inflater"""
    d = tmp_path_factory.mktemp("deflate_tokens")
    exe = N.build(d, sanitize=False)
    restated = N.restate(exe, d / "cases", {c.name: c.text for c in DC.CASES.values()})
    items = []
    for name in DC.NAMES:
        for i, (piece, _, made) in enumerate(restated[name]):
            assert zlib.decompress(made.data, 31) == piece
            items.append(("%s.%d" % (name, i), made.data, piece))
    assert max(made.max_lit_len for r in restated.values() for _, _, made in r) == 15
    assert max(made.max_dist_len for r in restated.values() for _, _, made in r) == 15
    assert b"".join(t for _, _, t in items) == b"".join(DC.CASES[name].text for name in DC.NAMES)
    check_members(db, items, comp_offset=6, text_offset=13)


# ------------------------------------------------------------------------------------------ the writer's batch boundary
def test_deflate_batch_boundary(kq, db):
    """4098 members: kq_deflate_bgzf_dev launches 4096 at a time, so the second launch reuses the slots, sizes and offsets of the
    first behind the running total.  The text is made on the device, a FASTQ-like tile with the member's index written into it
    in eight places; nothing of its size crosses to the host but the compressed output"""
    import torch
    from kreeq_amd import capi

    n_full, tail = 4097, 17
    n = n_full * MEMBER + tail
    started = time.perf_counter()
    tile = torch.frombuffer(bytearray(B.fastq_text(MEMBER, seed=21)), dtype=torch.uint8).cuda()
    text = tile.repeat(n_full + 1)[:n].contiguous()
    rows = text[:n_full * MEMBER].view(n_full, MEMBER)
    index = torch.arange(n_full, device="cuda")
    for place in range(8):
        for k in range(4):
            rows[:, 8000 * place + 100 + k] = (48 + (index // 10 ** (3 - k)) % 10).to(torch.uint8)
    cap = capi.bgzf_bound(n, capi.BGZF_EOF)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t_text = time.perf_counter()
    n_out = db.deflate_bgzf_dev(text.data_ptr(), n, out.data_ptr(), cap, capi.BGZF_EOF)
    t_deflate = time.perf_counter()
    data = out[:n_out].cpu().numpy().tobytes()
    blocks = scan(data, cap=n_full + 8)
    t_scan = time.perf_counter()
    assert len(blocks) == n_full + 2 and data[-28:] == B.EOF_BLOCK
    assert int(blocks["off"][0]) == 0 and (blocks["off"][1:] == blocks["off"][:-1] + blocks["size"][:-1]).all()
    assert (blocks["isize"][:n_full] == MEMBER).all() and int(blocks["isize"][n_full]) == tail and int(blocks["isize"][n_full + 1]) == 0
    back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t_before = time.perf_counter()
    assert db.inflate_bgzf_dev(out.data_ptr(), n_out, blocks, back.data_ptr(), n) == n
    t_inflate = time.perf_counter()
    assert torch.equal(back, text)
    # the members on both sides of the boundary are what the writer makes of their text alone
    for i in range(4094, 4098):
        piece = text[i * MEMBER:min((i + 1) * MEMBER, n)].cpu().numpy().tobytes()
        assert piece[100:104] == b"%04d" % i or i == n_full
        member = data[int(blocks["off"][i]):int(blocks["off"][i]) + int(blocks["size"][i])]
        assert zlib.decompress(member, 31) == piece, "member %d" % i
        assert member == db.deflate_bgzf(piece), "member %d differs from the member of its text alone" % i
    done = time.perf_counter()
    print("batch boundary: %d bytes of text -> %d; text %.2f s, deflate %.2f s, copy and scan %.2f s, inflate %.2f s, all %.2f s" % (
        n, n_out, t_text - started, t_deflate - t_text, t_scan - t_deflate, t_inflate - t_before, done - started))
