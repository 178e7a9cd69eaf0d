"""The yardstick of the BGZF tests: what tests/bgzf_inputs.py writes is valid multi-member gzip that holds the text it was given
(gzip.decompress), with the block kinds the names promise."""
import gzip
import zlib

import numpy as np

from tests import bgzf_inputs as B


def test_files_round_trip_through_gzip():
    text = B.fastq_text(300_000, seed=4)
    data = B.bgzf_file(text)
    assert gzip.decompress(data) == text
    assert data.endswith(B.EOF_BLOCK) and len(B.EOF_BLOCK) == 28
    blocks = B.blocks_of(data)
    assert [b[5] for b in blocks] == [B.BLOCK_TEXT] * (len(text) // B.BLOCK_TEXT) + [len(text) % B.BLOCK_TEXT, 0]
    assert sum(b[1] for b in blocks) == len(data)
    rng = np.random.default_rng(1)
    cuts = np.cumsum(rng.integers(1, 5001, 100)).tolist()
    data = B.bgzf_file(text[:cuts[-1] + 77], cuts=cuts, empty_at=(0, 5, 6, 50))
    assert gzip.decompress(data) == text[:cuts[-1] + 77]
    assert len(B.blocks_of(data)) == 101 + 4 + 1
    assert gzip.decompress(B.bgzf_file(b"")) == b""


def test_every_good_block_is_gzip_of_its_text():
    for name, (mem, text) in B.good_blocks().items():
        assert gzip.decompress(mem) == text, name
        assert len(mem) <= 65536, name
        (off, size, data_off, data_len, crc, isize), = B.blocks_of(mem)
        assert (off, size, isize, crc) == (0, len(mem), len(text), zlib.crc32(text)), name


def test_block_kinds():
    g = B.good_blocks()
    assert (g["stored_70"][0][18] >> 1) & 3 == 0 and (g["fixed"][0][18] >> 1) & 3 == 1
    assert all((g["fastq_level%d" % lv][0][18] >> 1) & 3 == 2 for lv in (1, 6, 9))
    assert len(g["A_65536"][0]) == 105
    assert len(g["far_reference"][1]) == 32700 and len(g["far_reference_issue"][1]) == 33069
    assert len(g["far_reference"][0]) < 33000 - 250              # the second copy of the 300 random bytes did not cost 300 bytes again
    assert sorted(set(g["all_bytes"][1])) == list(range(256))
    assert len(set(g["fibonacci"][1])) >= 24


def test_hand_made_streams_are_what_zlib_says():
    d = zlib.decompressobj(-15)
    for raw in (B.crafted_distance_before_start(), B.crafted_oversubscribed(), B.crafted_hlit_287()):
        try:
            zlib.decompressobj(-15).decompress(raw)
            raise AssertionError("zlib took a stream made to be invalid")
        except zlib.error:
            pass
    w = B.BitWriter().bits(1, 1).bits(1, 2)
    for ch in b"hello":
        w.fixed_lit(ch)
    assert d.decompress(w.fixed_lit(256).done()) == b"hello"
