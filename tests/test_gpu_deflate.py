"""Text deflated into BGZF members on the device (kq_deflate_bgzf / kq_deflate_bgzf_dev, kreeq_amd/csrc/kq_deflate.h): gzip reads
the output back, the project's block walk accepts every member, the device inflater returns the text, the bytes do not depend on
the alignment of the text or on the call, and the sizes meet conditions that are derived, not tuned: no member above its stored
form, 65 280 x 'A' below 1 KiB (253 matches of 258 bytes cost 13 bits each even with fixed codes, about 411 bytes: only
maximal-length matches get there), and every full member of a formatted table below its order-0 entropy bound, which Huffman
coding without matches cannot reach.  The CPU tests of the code builder (tests/test_deflate_core_host.py) come first; WHICH
tokens and bytes the device writes is held to a restatement of its parse in tests/test_gpu_deflate_parse.py."""
import gzip
import zlib

import numpy as np
import pytest

from tests import bgzf_inputs as B
from tests import table_cases as TC
from tests import table_ref as T
from tests.test_gpu_fastx import on_device

pytestmark = pytest.mark.gpu

MEMBER = 0xff00
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
GUARD = 0x5A
ERR_INVALID, ERR_CAPACITY = -1, -6


@pytest.fixture(scope="module")
def kq():
    import kreeq_amd

    if not kreeq_amd.device_available():
        pytest.fail("no gfx950 device: the product path has no CPU fallback")
    return kreeq_amd


@pytest.fixture(scope="module")
def db(kq):
    return kq.KreeqDB(21, 128, device=0, capacity_hint=1024)


def periodic(period, n, seed):
    unit = np.random.default_rng(seed).integers(0, 256, period, dtype=np.uint8).tobytes()
    return (unit * (n // period + 1))[:n]


def run_values(n, seed):
    """table values in runs of 1..59 equal positions, as the coverage of a real assembly has them"""
    rng = np.random.default_rng(seed)
    return np.repeat(TC.values(n, seed), rng.integers(1, 60, n), axis=0)[:n]


def plain_texts():
    fq = B.fastq_text(3 * MEMBER, seed=5)
    rnd = np.random.default_rng(77).integers(0, 256, MEMBER + 1000, dtype=np.uint8).tobytes()
    t = {"len_%d" % n: fq[:n] for n in (0, 1, 2, 3, 257, 258, 259, MEMBER - 1, MEMBER, MEMBER + 1, 2 * MEMBER + 5)}
    t["A_65280"] = b"A" * MEMBER
    t["period_2"] = b"xy" * 20000
    t["period_32768"] = periodic(32768, 2 * MEMBER, 1)
    t["period_32769"] = periodic(32769, 2 * MEMBER, 2)             # one byte beyond the window: no match may reach that far back
    t["all_bytes"] = bytes(range(256)) * 3 + bytes(range(255, -1, -1))
    t["random"] = rnd
    t["fastq"] = fq
    return t


PLAIN = plain_texts()
TABLES = [("kwig_runs", T.KWIG), ("bed", T.BED), ("csvtable", T.CSV)]


@pytest.fixture(scope="module")
def table_texts(db):
    """the formatter's own texts (kq_format_table), k = 21: .kwig of values in runs, .bed / .csvtable of the 4097-position segment"""
    out = {}
    n = 40000
    segs, names = T.pack_pieces([T.Piece(0, n, 3, b"chr", 0, True)])
    out["kwig_runs"] = db.format_table(T.KWIG, run_values(n, 7), segs, names)
    t, pieces = TC.one_segment(4097, 4, TC.NAMES[7], 99990)
    segs, names = T.pack_pieces(pieces)
    out["bed"] = db.format_table(T.BED, t, segs, names)
    out["csvtable"] = db.format_table(T.CSV, t, segs, names)
    t, pieces = TC.many_pieces(3, 300)
    segs, names = T.pack_pieces(pieces)
    out["kwig_pieces"] = db.format_table(T.KWIG, t, segs, names)
    for name in ("kwig_runs", "bed", "csvtable"):
        assert len(out[name]) > 4 * MEMBER
    return out


def members_of(data):
    from kreeq_amd import capi

    blocks, used = capi.bgzf_scan(data)
    assert used == len(data)
    return blocks


def check_container(data, text, eof):
    """gzip reads it, the block walk accepts every member, sizes and CRC are the text's"""
    from kreeq_amd import capi

    assert gzip.decompress(data) == text if data else text == b""
    blocks = members_of(data)
    n_members = (len(text) + MEMBER - 1) // MEMBER
    assert len(blocks) == n_members + (1 if eof else 0)
    at = 0
    for i, b in enumerate(blocks[:n_members]):
        piece = text[i * MEMBER:(i + 1) * MEMBER]
        assert int(b["off"]) == at and int(b["isize"]) == len(piece) <= MEMBER and int(b["crc32"]) == zlib.crc32(piece)
        assert int(b["size"]) <= 18 + 5 + len(piece) + 8, "member %d is larger than its stored form" % i
        at += int(b["size"])
    if eof:
        assert data[-28:] == EOF_MARKER and int(blocks[-1]["isize"]) == 0
    assert len(data) <= capi.bgzf_bound(len(text), capi.BGZF_EOF if eof else 0)
    return blocks


def deflate_dev(db, text, offset=0, flags=0, out_offset=3, src=None):
    """kq_deflate_bgzf_dev with the text `offset` bytes behind a 16-byte boundary (or in `src`, a device tensor that holds it
    already) and the output `out_offset` bytes behind one, guarded"""
    import torch
    from kreeq_amd import capi

    if src is None:
        src = on_device(text, offset)
    cap = capi.bgzf_bound(len(text), flags)
    lead = 16 + out_offset
    out = torch.full((lead + cap + 48,), GUARD, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    n = db.deflate_bgzf_dev(src.data_ptr() if len(text) else 0, len(text), out.data_ptr() + lead, cap, flags)
    got = out.cpu().numpy()
    assert (got[:lead] == GUARD).all() and (got[lead + n:] == GUARD).all(), "bytes outside the output were written"
    return got[lead:lead + n].tobytes()


def inflate_dev(db, data):
    import torch

    blocks = members_of(data)
    comp = on_device(data)
    n = db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, None, 0)
    out = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, out.data_ptr(), n) == n
    return out.cpu().numpy()[:n].tobytes()


def check_text(db, text):
    from kreeq_amd import capi

    plain = db.deflate_bgzf(text)
    check_container(plain, text, eof=False)
    with_eof = db.deflate_bgzf(text, capi.BGZF_EOF)
    assert with_eof == plain + EOF_MARKER
    check_container(with_eof, text, eof=True)
    assert inflate_dev(db, with_eof) == text                        # the device round trip
    for off in (0, 1, 7, 15):                                       # the bytes are a function of the text alone
        assert deflate_dev(db, text, off) == plain, "offset %d" % off
    assert db.deflate_bgzf(text) == plain
    return plain


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_round_trip(db, name):
    check_text(db, PLAIN[name])


@pytest.mark.parametrize("name", ["kwig_runs", "bed", "csvtable", "kwig_pieces"])
def test_table_round_trip(db, table_texts, name):
    check_text(db, table_texts[name])


def test_successive_calls_concatenate(db):
    from kreeq_amd import capi

    a, b, c = PLAIN["fastq"][:70000], PLAIN["len_3"], PLAIN["period_2"]
    data = db.deflate_bgzf(a) + db.deflate_bgzf(b) + db.deflate_bgzf(b"") + db.deflate_bgzf(c, capi.BGZF_EOF)
    assert gzip.decompress(data) == a + b + c
    assert data[-28:] == EOF_MARKER
    members_of(data)
    assert db.deflate_bgzf(b"") == b"" and db.deflate_bgzf(b"", capi.BGZF_EOF) == EOF_MARKER


def test_sizes_are_derived(db, table_texts):
    a = members_of(db.deflate_bgzf(PLAIN["A_65280"]))
    assert len(a) == 1 and int(a[0]["size"]) < 1024                 # maximal matches are found and used
    r = members_of(db.deflate_bgzf(PLAIN["random"]))
    assert [int(b["size"]) for b in r] == [18 + 5 + MEMBER + 8, 18 + 5 + 1000 + 8]      # random bytes: stored, exactly
    for name, _ in TABLES:                                          # every full member beats Huffman coding without matches
        text = table_texts[name]
        blocks = members_of(db.deflate_bgzf(text))
        for i in range(len(text) // MEMBER):
            piece = np.frombuffer(text[i * MEMBER:(i + 1) * MEMBER], dtype=np.uint8)
            c = np.bincount(piece, minlength=256).astype(np.float64)
            c = c[c > 0]
            bound = float(-(c * np.log2(c / c.sum())).sum()) / 8
            ref = zlib.compressobj(1, zlib.DEFLATED, -15)
            level1 = len(ref.compress(piece.tobytes()) + ref.flush())
            print("%s member %d: %d bytes, order-0 bound %.0f, zlib level 1 %d" % (name, i, int(blocks[i]["size"]), bound, level1))
            assert level1 + 26 < bound                              # the input leaves room: zlib's matches get well below it
            assert int(blocks[i]["size"]) < bound, (name, i)


def test_capacity_and_refusals(db):
    import ctypes as C

    import torch
    from kreeq_amd import KqError, capi

    text = PLAIN["fastq"][:MEMBER + 10]
    assert capi.bgzf_bound(0) == 0 and capi.bgzf_bound(0, capi.BGZF_EOF) == 28
    assert capi.bgzf_bound(1) == 32 and capi.bgzf_bound(MEMBER) == MEMBER + 31 and capi.bgzf_bound(MEMBER + 1, capi.BGZF_EOF) == MEMBER + 1 + 62 + 28
    bound = capi.bgzf_bound(len(text), capi.BGZF_EOF)
    src = on_device(text)
    out = torch.full((bound + 16,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for cap in (0, bound - 1):                                      # below the bound: refused before any device work, nothing written
        with pytest.raises(KqError) as e:
            db.deflate_bgzf_dev(src.data_ptr(), len(text), out.data_ptr(), cap, capi.BGZF_EOF)
        assert e.value.code == ERR_CAPACITY and e.value.needed == bound
    with pytest.raises(KqError) as e:
        db.deflate_bgzf(text, capi.BGZF_EOF, cap=bound - 1)
    assert e.value.code == ERR_CAPACITY and e.value.needed == bound
    assert (out.cpu().numpy() == GUARD).all()
    n = db.deflate_bgzf_dev(src.data_ptr(), len(text), out.data_ptr(), bound, capi.BGZF_EOF)
    assert gzip.decompress(out.cpu().numpy()[:n].tobytes()) == text
    L = capi.load()
    no = C.c_uint64(7)
    h = db._h
    assert L.kq_deflate_bgzf_dev(h, None, 5, C.c_void_p(out.data_ptr()), bound, C.byref(no), 0) == ERR_INVALID       # no text
    assert L.kq_deflate_bgzf_dev(h, C.c_void_p(src.data_ptr()), 5, None, bound, C.byref(no), 0) == ERR_INVALID      # no output
    assert L.kq_deflate_bgzf_dev(h, C.c_void_p(src.data_ptr()), 5, C.c_void_p(out.data_ptr()), bound, None, 0) == ERR_INVALID
    assert L.kq_deflate_bgzf_dev(None, C.c_void_p(src.data_ptr()), 5, C.c_void_p(out.data_ptr()), bound, C.byref(no), 0) == ERR_INVALID
    for flags in (1, 4, 3):                                         # KQ_BGZF_END is not a flag of this entry
        assert L.kq_deflate_bgzf_dev(h, C.c_void_p(src.data_ptr()), 5, C.c_void_p(out.data_ptr()), bound, C.byref(no), flags) == ERR_INVALID
        assert L.kq_deflate_bgzf(h, None, 0, None, 0, C.byref(no), flags) == ERR_INVALID
    assert L.kq_deflate_bgzf(h, None, 5, None, 0, C.byref(no), 0) == ERR_INVALID
