"""kq_bgzf_scan, the host-only block walk of a BGZF file, through ctypes on libkreeq_amd.so: no device is needed."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from kreeq_amd import build, capi
from tests import bgzf_inputs as B
from tests.helpers import INPUTS

OK, INVALID, CAPACITY = 0, -1, -6


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return capi.load()


def scan(lib, data, cap):
    """-> (rc, blocks, consumed); the buffer handed over is exactly len(data) bytes"""
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    blocks = np.zeros(max(cap, 1), dtype=capi.BGZF_BLOCK_DTYPE)
    n, used = C.c_uint64(99), C.c_uint64(99)
    rc = lib.kq_bgzf_scan(buf, len(data), blocks.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(used))
    return rc, blocks[:min(n.value, cap)], n.value, used.value


@pytest.fixture(scope="module")
def multi():
    text = B.fastq_text(200_000, seed=12)
    return B.bgzf_file(text, empty_at=(2,)), text


def test_symbols_and_struct(lib):
    for s in ("kq_bgzf_scan", "kq_inflate_bgzf_dev", "kq_count_bgzf_dev"):
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    assert capi.BGZF_BLOCK_DTYPE.itemsize == 32 and capi.BGZF_END == 1
    assert lib.kq_abi_version() == 4


def test_blocks_of_a_multi_block_file(lib, multi):
    data, _ = multi
    want = B.blocks_of(data)
    rc, blocks, n, used = scan(lib, data, 64)
    assert (rc, n, used) == (OK, len(want), len(data))
    got = [tuple(int(b[f]) for f in ("off", "size", "data_off", "data_len", "crc32", "isize")) for b in blocks]
    assert got == want
    assert got[2][5] == 0 and got[-1][5] == 0                      # the empty block mid-file and the EOF marker
    blocks2, used2 = capi.bgzf_scan(data)
    assert used2 == len(data) and np.array_equal(blocks2, blocks)


def test_second_subfield_in_front_of_bc(lib):
    mem, _ = B.good_blocks()["second_subfield"]
    rc, blocks, n, used = scan(lib, mem + B.EOF_BLOCK, 4)
    assert (rc, n, used) == (OK, 2, len(mem) + 28)
    assert int(blocks[0]["data_off"]) == 12 + 7 + 6 and int(blocks[0]["data_len"]) == len(mem) - 25 - 8
    assert int(blocks[1]["off"]) == len(mem)


def test_len_cut_inside_the_last_member(lib, multi):
    data, _ = multi
    want = B.blocks_of(data[:-28])                                  # without the EOF marker: the last member has data
    last = want[-1]
    body = data[:-28]
    cuts = list(range(last[0], last[0] + 19)) + list(range(len(body) - 9, len(body)))      # every byte of header and trailer
    for cut in cuts:
        rc, _, n, used = scan(lib, body[:cut], 64)
        assert (rc, n, used) == (OK, len(want) - 1, last[0]), cut
    rc, _, n, used = scan(lib, body, 64)
    assert (rc, n, used) == (OK, len(want), len(body))
    assert scan(lib, b"", 4)[0::2] == (OK, 0) and scan(lib, b"", 4)[3] == 0


def test_plain_gzip_is_refused_at_its_first_member(lib):
    data = open(os.path.join(INPUTS, "random1.fastq.gz"), "rb").read()
    rc, _, n, used = scan(lib, data, 16)
    assert (rc, n, used) == (INVALID, 0, 0)
    assert b"BGZF" in lib.kq_last_error()
    with pytest.raises(capi.KqError) as e:
        capi.bgzf_scan(data)
    assert e.value.code == INVALID and e.value.consumed == 0 and e.value.n_blocks == 0


def test_bgzf_followed_by_plain_gzip(lib, multi):
    data, _ = multi
    plain = open(os.path.join(INPUTS, "random1.fastq.gz"), "rb").read()
    rc, _, n, used = scan(lib, data + plain, 64)
    assert (rc, n, used) == (INVALID, len(B.blocks_of(data)), len(data))


def test_cap_too_small(lib, multi):
    data, _ = multi
    want = B.blocks_of(data)
    rc, blocks, n, used = scan(lib, data, 2)
    assert (rc, n) == (CAPACITY, len(want))
    assert [int(b["off"]) for b in blocks] == [w[0] for w in want[:2]]
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    n, used = C.c_uint64(0), C.c_uint64(0)
    assert lib.kq_bgzf_scan(buf, len(data), None, 0, C.byref(n), C.byref(used)) == CAPACITY and n.value == len(want)


def test_xlen_pointing_past_len(lib):
    mem, _ = B.good_blocks()["one_byte"]
    bad = bytearray(mem)
    struct.pack_into("<H", bad, 10, 60000)                          # the extra field would end far behind the buffer
    rc, _, n, used = scan(lib, bytes(bad), 4)
    assert (rc, n, used) == (OK, 0, 0)                              # "not all here yet": nothing is read behind len
    # a subfield whose SLEN runs past XLEN hides 'BC': not BGZF
    bad = bytearray(mem)
    struct.pack_into("<H", bad, 12 + 2, 5000)
    bad[12:14] = b"XY"
    rc, _, n, used = scan(lib, bytes(bad), 4)
    assert (rc, n, used) == (INVALID, 0, 0)


def test_bsize_smaller_than_header_plus_trailer(lib):
    mem, _ = B.good_blocks()["one_byte"]
    for bsize in (0, 10, 24):                                       # size = BSIZE + 1 < XLEN + 20 = 26
        bad = bytearray(mem)
        struct.pack_into("<H", bad, 16, bsize)
        rc, _, n, used = scan(lib, bytes(bad) * 2, 4)
        assert (rc, n, used) == (INVALID, 0, 0), bsize
    ok = bytearray(mem)
    struct.pack_into("<H", ok, 16, 25)                              # exactly header + trailer: an acceptable shape with no data
    ok = bytes(ok[:18]) + struct.pack("<II", 0, 0)
    rc, blocks, n, used = scan(lib, ok, 4)
    assert (rc, n, used) == (OK, 1, 26) and int(blocks[0]["data_len"]) == 0


def test_isize_above_64k_is_refused(lib):
    mem, _ = B.good_blocks()["one_byte"]
    bad = bytearray(mem)
    struct.pack_into("<I", bad, len(bad) - 4, 65537)
    assert scan(lib, bytes(bad), 4)[0] == INVALID


def test_null_arguments(lib):
    n, used = C.c_uint64(0), C.c_uint64(0)
    assert lib.kq_bgzf_scan(None, 5, None, 0, C.byref(n), C.byref(used)) == INVALID
    buf = (C.c_uint8 * 8)()
    assert lib.kq_bgzf_scan(buf, 8, None, 0, None, C.byref(used)) == INVALID
    t = C.c_uint64(0)
    assert lib.kq_inflate_bgzf_dev(None, buf, 8, None, 0, None, 0, C.byref(t)) == INVALID
    assert lib.kq_count_bgzf_dev(None, buf, 8, None, 0, 1, 0) == INVALID
