"""BGZF members inflated on the device (kq_inflate_bgzf_dev) against zlib, byte for byte; corrupt members refused with the first
bad member named; and the BGZF stream entry point (kq_count_bgzf_dev) against kq_count_fastx_dev of the
plain text and the CPU oracle's table of the host-style batch.  Inputs: tests/bgzf_inputs.py.  The CPU tests of the same decoder
(tests/test_inflate_core_host.py) come first: the kernel runs the same core."""
import functools
import zlib

import numpy as np
import pytest

from tests import bgzf_inputs as B
from tests import helpers as H
from tests.test_fastx_rule import FASTA, FASTQ, host_batch
from tests.test_gpu_fastx import make_fastq, on_device

pytestmark = pytest.mark.gpu

GUARD = 0x5A


@pytest.fixture(scope="module")
def kq():
    import kreeq_amd

    if not kreeq_amd.device_available():
        pytest.fail("no gfx950 device: the product path has no CPU fallback")
    return kreeq_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def good():
    return B.good_blocks()


def scan(data):
    from kreeq_amd import capi

    blocks, used = capi.bgzf_scan(data)
    assert used == len(data)
    return blocks


def inflate(db, data, offset=0, text_offset=0, blocks=None):
    """-> the whole guarded output buffer as numpy, the text's offset in it and its size"""
    import torch

    blocks = scan(data) if blocks is None else blocks
    comp = on_device(data, offset)
    n = db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, None, 0)
    lo = 16 + text_offset
    out = torch.full((lo + n + 48,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n2 = db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, out.data_ptr() + lo, n)
    assert n2 == n
    return out.cpu().numpy(), lo, n


def check_inflate(db, data, want, **kw):
    got, lo, n = inflate(db, data, **kw)
    assert n == len(want)
    assert (got[:lo] == GUARD).all() and (got[lo + n:] == GUARD).all(), "guard bytes overwritten"
    if got[lo:lo + n].tobytes() != want:
        w = np.frombuffer(want, dtype=np.uint8)
        bad = np.flatnonzero(got[lo:lo + n] != w)
        raise AssertionError("%d of %d bytes differ, the first at %d" % (len(bad), n, int(bad[0])))


# ------------------------------------------------------------------------------------------------------------ inflate
SINGLE = ["empty", "eof_marker", "one_byte", "stored_max", "stored_70", "fixed", "fastq_level1", "fastq_level6", "fastq_level9", "three_flushes",
          "A_65536", "far_reference", "far_reference_issue", "all_bytes", "fibonacci", "second_subfield"]


@pytest.mark.parametrize("name", SINGLE)
def test_inflate_single_block(kq, good, name):
    mem, text = good[name]
    assert zlib.decompress(mem, 31) == text
    db = kq.KreeqDB(21, 128)
    check_inflate(db, mem, text, offset=len(name) % 4, text_offset=len(name) % 16)


def test_inflate_300_blocks_shuffled(kq, good):
    rng = np.random.default_rng(300)
    names = sorted(good)
    picks = [names[int(i)] for i in rng.integers(0, len(names), 300)]
    assert set(picks) == set(names)
    data = b"".join(good[n][0] for n in picks)                      # byte-packed members
    want = b"".join(good[n][1] for n in picks)                      # each text lands at the sum of ISIZE before it
    db = kq.KreeqDB(21, 128)
    for off in (0, 1, 2, 3):
        check_inflate(db, data, want, offset=off, text_offset=off * 5)


def test_inflate_sizes_and_capacity(kq, good):
    import torch

    data = b"".join(good[n][0] for n in ("fixed", "empty", "fastq_level6"))
    want = good["fixed"][1] + good["fastq_level6"][1]
    db = kq.KreeqDB(21, 128)
    blocks = scan(data)
    comp = on_device(data)
    assert db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, None, 0) == len(want)
    out = torch.full((len(want) + 32,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(kq.KqError) as e:
        db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, out.data_ptr(), len(want) - 1)
    assert e.value.code == -6 and e.value.needed == len(want)
    assert (out.cpu().numpy() == GUARD).all()
    assert db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks[:0], out.data_ptr(), 10) == 0
    # a list that does not lie inside comp_len
    with pytest.raises(kq.KqError) as e:
        db.inflate_bgzf_dev(comp.data_ptr(), len(data) - 1, blocks, out.data_ptr(), len(want))
    assert e.value.code == -1 and "block 2" in str(e.value)
    assert (out.cpu().numpy() == GUARD).all()
    assert db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, out.data_ptr(), len(want)) == len(want)
    assert out.cpu().numpy()[:len(want)].tobytes() == want


# ------------------------------------------------------------------------------------------------------------ corrupt
MUTATIONS = ["isize_plus_1", "isize_minus_1", "crc_bit", "data_len_minus_1", "data_len_half", "btype_3", "stored_nlen", "distance_before_start",
             "oversubscribed", "hlit_287"]


@pytest.mark.parametrize("name", MUTATIONS)
def test_corrupt_middle_block_is_refused(kq, good, name):
    import torch

    first, last = good["fixed"], good["three_flushes"]
    mem, text = good["fastq_level6"]
    muts = {n: (m, code) for n, m, code in B.mutations(mem, text)}
    assert sorted(muts) == sorted(MUTATIONS)
    bad, code = muts[name]
    data = first[0] + bad + last[0]
    blocks = scan(data)
    assert len(blocks) == 3
    n0, n1, n2 = (int(b["isize"]) for b in blocks)
    db = kq.KreeqDB(21, 128)
    comp = on_device(data, 1)
    out = torch.full((16 + n0 + n1 + n2 + 48,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(kq.KqError) as e:
        db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, out.data_ptr() + 16, n0 + n1 + n2)
    assert e.value.code == -1 and "block 1 " in str(e.value), str(e.value)
    got = out.cpu().numpy()
    assert (got[:16] == GUARD).all() and (got[16 + n0 + n1 + n2:] == GUARD).all()
    assert (got[16 + n0:16 + n0 + n1] == GUARD).all(), "the failed block stored something"
    assert got[16:16 + n0].tobytes() == first[1] and got[16 + n0 + n1:16 + n0 + n1 + n2].tobytes() == last[1]
    # the same handle then inflates the good file
    check_inflate(db, first[0] + mem + last[0], first[1] + text + last[1], offset=2)


def test_first_bad_block_is_the_one_reported(kq, good):
    mem, text = good["fastq_level6"]
    muts = {n: m for n, m, _ in B.mutations(mem, text)}
    data = b"".join([good["fixed"][0]] * 40 + [muts["crc_bit"]] + [good["fixed"][0]] * 40 + [muts["btype_3"]] * 100)
    db = kq.KreeqDB(21, 128)
    with pytest.raises(kq.KqError) as e:
        inflate(db, data)
    assert "block 40 " in str(e.value) and "CRC" in str(e.value)


# ------------------------------------------------------------------------------------------------------------ stream
def fastq_reads():
    rng = np.random.default_rng(6)
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = []
    for i in range(3000):
        r = bytearray(rng.choice(alphabet, int(rng.integers(1, 401))).tolist())
        if i % 7 == 0:
            r = bytearray(bytes(r).lower())
        if i % 11 == 0:
            r[int(rng.integers(0, len(r)))] = ord("N")
        reads.append(bytes(r))
    return reads


@functools.lru_cache(maxsize=None)
def stream_input(kind):
    """-> (text, format): the 3000-read FASTQ in its four line-end variants, and the wrapped multi-record FASTA"""
    if kind == "fasta":
        rng = np.random.default_rng(8)
        alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
        out = []
        for i in range(3000):
            sb = bytes(rng.choice(alphabet, 150).tolist())
            if i % 5 == 0:
                sb = sb.lower()
            out.append(b">r%d wrapped\n" % i + sb[:60] + b"\n" + sb[60:120] + b"\n" + sb[120:] + b"\n")
        return b"".join(out), FASTA
    eol, final = {"fastq_nl": (b"\n", True), "fastq_nl_open": (b"\n", False), "fastq_crlf": (b"\r\n", True), "fastq_crlf_open": (b"\r\n", False)}[kind]
    return make_fastq(fastq_reads(), seed=3, eol=eol, final_eol=final), FASTQ


def cut_class(text, c, fmt):
    if text[c - 1:c] == b"\n":
        return "behind_nl"
    if text[c - 1:c] == b"\r" and text[c:c + 1] == b"\n":
        return "cr_nl"
    line = text.count(b"\n", 0, c)
    if fmt == FASTA:
        return "header" if text[text.rfind(b"\n", 0, c) + 1:][:1] == b">" else "sequence"
    return ("header", "sequence", "plus", "quality")[line % 4]


@functools.lru_cache(maxsize=None)
def stream_cuts(kind):
    """seeded random block boundaries 1..5000 bytes apart, plus one boundary placed in each kind of position the text has"""
    text, fmt = stream_input(kind)
    rng = np.random.default_rng(len(kind))
    cuts = set()
    c = int(rng.integers(1, 5001))
    while c < len(text):
        cuts.add(c)
        c += int(rng.integers(1, 5001))
    kinds = ["header", "sequence", "behind_nl"] + (["plus", "quality"] if fmt == FASTQ else []) + (["cr_nl"] if b"\r" in text else [])
    for want in kinds:
        c = len(text) // 3
        while cut_class(text, c, fmt) != want:
            c += 1
        cuts.add(c)
    cuts = sorted(cuts)
    assert {cut_class(text, c, fmt) for c in cuts} >= set(kinds)
    return cuts


def test_stream_cuts_cover_the_six_positions():
    seen = set()
    for kind in ("fastq_nl", "fastq_nl_open", "fastq_crlf", "fastq_crlf_open"):
        text, fmt = stream_input(kind)
        seen |= {cut_class(text, c, fmt) for c in stream_cuts(kind)}
    assert seen == {"header", "sequence", "plus", "quality", "behind_nl", "cr_nl"}


@functools.lru_cache(maxsize=None)
def stream_file(kind):
    text, _ = stream_input(kind)
    cuts = stream_cuts(kind)
    data = B.bgzf_file(text, cuts=cuts, empty_at=tuple(range(3, len(cuts), 17)))
    blocks = scan(data)
    assert int(blocks["isize"].sum()) == len(text) and (blocks["isize"] == 0).sum() > 5
    return data, blocks


_reference = {}


def reference(kq, O, kind):
    """(summary, export) of kq_count_fastx_dev on the plain text, checked once against the oracle's table of the host-style batch"""
    if kind not in _reference:
        text, fmt = stream_input(kind)
        gpu = kq.KreeqDB(21, 128, capacity_hint=2_000_000)
        t = on_device(text)
        gpu.count_fastx_dev(t.data_ptr(), len(text), fmt)
        gpu.sync()
        cpu = O.OracleDB(21, 128)
        cpu.count_batch(host_batch(text, fmt), threads=8)
        assert gpu.summary() == cpu.summary()
        assert H.entries_equal(gpu.export(), cpu.export())
        _reference[kind] = (gpu.summary(), gpu.export())
    return _reference[kind]


def feed(db, comp, data, blocks, fmt, per_call, end=True):
    """the blocks in runs of per_call, each run with its own piece of the compressed buffer"""
    from kreeq_amd import capi

    n = len(blocks)
    for a in range(0, n, per_call):
        run = blocks[a:a + per_call].copy()
        lo = int(run["off"][0])
        hi = int(run["off"][-1] + run["size"][-1])
        run["off"] -= lo
        db.count_bgzf_dev(comp.data_ptr() + lo, hi - lo, run, fmt, capi.BGZF_END if end and a + per_call >= n else 0)


@pytest.mark.parametrize("per_call", [1, 2, 7, 0])
@pytest.mark.parametrize("kind", ["fastq_nl", "fastq_nl_open", "fastq_crlf", "fastq_crlf_open", "fasta"])
def test_stream_equals_the_plain_text(kq, O, kind, per_call):
    want_summary, want_export = reference(kq, O, kind)
    _, fmt = stream_input(kind)
    data, blocks = stream_file(kind)
    db = kq.KreeqDB(21, 128, capacity_hint=2_000_000)
    comp = on_device(data, 3)
    feed(db, comp, data, blocks, fmt, per_call or len(blocks))
    db.sync()
    assert db.summary() == want_summary
    assert H.entries_equal(db.export(), want_export)


def test_stream_long_record_spans_four_calls(kq, O):
    """one FASTQ record of 200 000 bp between short ones: three calls end inside it (FASTQ cut = 0: everything is carried)"""
    from kreeq_amd import capi

    rng = np.random.default_rng(20)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    long_read = bytes(rng.choice(acgt, 200_000).tolist())
    short = [bytes(rng.choice(acgt, 100).tolist()) for _ in range(6)]
    text = make_fastq(short[:3], seed=1) + b"@long\n" + long_read + b"\n+\n" + b"I" * 200_000 + b"\n" + make_fastq(short[3:], seed=2)
    data = B.bgzf_file(text)
    blocks = scan(data)
    start = text.index(b"@long")
    first = start // B.BLOCK_TEXT                                   # the block the long record begins in
    edges = [0, first + 1, first + 2, first + 4, first + 6, len(blocks)]
    sizes = np.concatenate([[0], np.cumsum(blocks["isize"])])
    assert all(start < sizes[e] < start + 400_000 for e in edges[1:5])      # four calls end inside the record
    db = kq.KreeqDB(21, 128, capacity_hint=1 << 20)
    comp = on_device(data)
    for a, b in zip(edges[:-1], edges[1:]):
        run = blocks[a:b].copy()
        lo, hi = int(run["off"][0]), int(run["off"][-1] + run["size"][-1])
        run["off"] -= lo
        db.count_bgzf_dev(comp.data_ptr() + lo, hi - lo, run, FASTQ, capi.BGZF_END if b == len(blocks) else 0)
    db.sync()
    cpu = O.OracleDB(21, 128)
    cpu.count_batch(host_batch(text, FASTQ))
    assert db.summary() == cpu.summary()
    assert H.entries_equal(db.export(), cpu.export())


def test_stream_abandoned_then_cleared(kq, O):
    want_summary, want_export = reference(kq, O, "fastq_nl")
    data, blocks = stream_file("fastq_nl")
    other, fmt = stream_input("fasta")
    other_data = B.bgzf_file(other[:len(other) // 2 + 33])           # ends inside a record
    db = kq.KreeqDB(21, 128, capacity_hint=2_000_000)
    oc = on_device(other_data)
    feed(db, oc, other_data, scan(other_data), fmt, 3, end=False)    # no KQ_BGZF_END: a carry is left behind
    db.clear()
    comp = on_device(data)
    feed(db, comp, data, blocks, FASTQ, 50)
    db.sync()
    assert db.summary() == want_summary
    assert H.entries_equal(db.export(), want_export)


def test_stream_wrapped_fastq_is_refused(kq, O):
    from kreeq_amd import capi

    reads = fastq_reads()
    bad_text = (make_fastq(reads[:40], seed=1) + b"@w\nACGTACGTACGTACGTACGTACGTACGT\nACGTACGTACGTACGTACGTACGTACGT\n+\n" + b"I" * 28 + b"\n" + b"I" * 28 + b"\n" +
                make_fastq(reads[40:200], seed=2))
    data = B.bgzf_file(bad_text, cuts=list(range(3000, len(bad_text), 3000)))
    blocks = scan(data)
    db = kq.KreeqDB(21, 128, capacity_hint=2_000_000)
    comp = on_device(data)
    db.count_bgzf_dev(comp.data_ptr(), len(data), blocks, FASTQ, capi.BGZF_END)
    for _ in range(2):
        with pytest.raises(kq.KqError) as e:
            db.sync()
        assert e.value.code == -1 and "FASTQ" in str(e.value)
    db.clear()
    db.sync()
    # a corrupt block in a stream: the same, and the message names the block
    mem, text = B.good_blocks()["fastq_level6"]
    muts = {n: m for n, m, _ in B.mutations(mem, text)}
    bad = B.good_blocks()["fixed"][0] + muts["crc_bit"]
    bc = on_device(bad)
    db.count_bgzf_dev(bc.data_ptr(), len(bad), scan(bad), FASTQ, capi.BGZF_END)
    with pytest.raises(kq.KqError) as e:
        db.sync()
    assert e.value.code == -1 and "block 1 " in str(e.value) and "CRC" in str(e.value)
    db.clear()
    want_summary, want_export = reference(kq, O, "fastq_nl")
    gdata, gblocks = stream_file("fastq_nl")
    gc = on_device(gdata)
    feed(db, gc, gdata, gblocks, FASTQ, 40)
    db.sync()
    assert db.summary() == want_summary and H.entries_equal(db.export(), want_export)
