"""The parse contract of the device FASTQ / FASTA parser (include/kreeq_amd.h, kq_parse_fastx_dev), restated twice and
compared on the CPU: `rule_bytes` is the byte rule itself in numpy (what the GPU tests expect, byte for byte),
`host_batch` walks the text record by record like the host parser (kreeq_amd/host/fastx.cpp).  Both must give the same
reads, i.e. the same maximal [ACGTacgt]+ runs.  Also here: the new entry points exist and reject bad arguments without
a device."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from kreeq_amd import build, capi
from tests.helpers import INPUTS

FASTQ, FASTA = 1, 2


def rule_keep(text: bytes, fmt: int):
    """bool mask of the kept bytes.  l(i) = number of '\\n' before byte i; EOL-CR = '\\r' directly followed by '\\n'.
    FASTQ: kept iff l(i) mod 4 == 1 and no EOL-CR.  FASTA: of a header line (first byte '>') only its '\\n'; of any other
    line every byte but '\\n' and EOL-CR."""
    a = np.frombuffer(text, dtype=np.uint8)
    if len(a) == 0:
        return np.zeros(0, dtype=bool)
    nl = a == 10
    line = np.cumsum(nl) - nl                                   # exclusive: a '\n' belongs to the line it ends
    eolcr = (a == 13) & np.concatenate([nl[1:], [False]])
    if fmt == FASTQ:
        return (line % 4 == 1) & ~eolcr
    starts = np.concatenate([[0], np.flatnonzero(nl) + 1])      # first byte of every line (the last may lie behind the text)
    first = np.where(starts < len(a), a[np.minimum(starts, len(a) - 1)], 0)
    header = (first == ord(">"))[line]
    return np.where(header, nl, ~nl & ~eolcr)


def rule_bytes(text: bytes, fmt: int) -> bytes:
    return np.frombuffer(text, dtype=np.uint8)[rule_keep(text, fmt)].tobytes()


def rule_flag(text: bytes, fmt: int) -> bool:
    """what the device refuses: a FASTQ line 0 (mod 4) not starting with '@' / line 2 not starting with '+'; a FASTA text
    not starting with '>'"""
    if not text:
        return False
    if fmt == FASTA:
        return text[:1] != b">"
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()                                             # no line starts behind the text
    return any((i % 4 == 0 and l[:1] != b"@") or (i % 4 == 2 and l[:1] != b"+") for i, l in enumerate(lines))


def host_batch(text: bytes, fmt: int) -> bytes:
    """the host parser's batch (seq0\\nseq1...), record by record: four-line FASTQ records with the sequence line's trailing
    '\\r' trimmed; FASTA records = a '>' line and every line up to the next one, each trimmed of trailing '\\n' / '\\r', joined"""
    lines = text.split(b"\n")
    seqs = []
    if fmt == FASTQ:
        i = 0
        while i < len(lines) and not (i == len(lines) - 1 and lines[i] == b""):
            assert lines[i][:1] == b"@"
            seqs.append(lines[i + 1].rstrip(b"\r") if i + 1 < len(lines) else b"")
            i += 4
    else:
        cur = None
        for l in lines:
            if l[:1] == b">":
                if cur is not None:
                    seqs.append(cur)
                cur = b""
            else:
                cur += l.rstrip(b"\r")
        if cur is not None:
            seqs.append(cur)
    return b"\n".join(seqs)


def runs(batch: bytes):
    return re.findall(rb"[ACGTacgt]+", batch)


def fmt_of(text: bytes) -> int:
    return FASTQ if text[:1] == b"@" else FASTA


CORNERS = {
    "fastq_crlf": b"@r1 x\r\nACGTN\r\n+\r\nIIIII\r\n@r2\r\nGGCC\r\n+\r\nIIII\r\n",
    "fastq_no_final_newline": b"@r1\nACGT\n+\nIIII\n@r2\nTTGA\n+\nIIII",
    "fastq_lowercase_n": b"@r1\nacgtNNacgT\n+\nIIIIIIIIII\n@r2\nnnnn\n+\nIIII\n",
    "fastq_empty_sequence": b"@r1\n\n+\n\n@r2\nACGT\n+\nIIII\n",
    "fastq_quality_starts_with_at_and_plus": b"@r1\nACGT\n+\n@III\n@r2\nGGTT\n+r2\n+III\n@r3\nCC\n+\n@+\n",
    "fastq_cr_inside_sequence": b"@r1\nAC\rGT\n+\nIIIII\n",
    "fastq_single_record": b"@only\nACGTACGTAC\n+\nIIIIIIIIII\n",
    "fasta_crlf_wrapped": b">s1 d\r\nACGT\r\nTTGA\r\n>s2\r\nGG\r\nCC\r\n",
    "fasta_no_final_newline": b">s1\nACGT\nTT\n>s2\nGGCC",
    "fasta_lowercase_n": b">s1\nacgtNNNNac\ngt\n>s2\nNNNN\n",
    "fasta_two_headers_in_a_row": b">a\n>b\nACGT\n>c\n>d\n>e\nTT\nGG\n",
    "fasta_empty_line_in_record": b">a\nACGT\n\nTTTT\n>b\n\nGG\n",
    "fasta_cr_inside_sequence": b">a\nAC\rGT\nTT\n",
    "fasta_gt_inside_sequence_line": b">a\nAC>GT\nTT\n",
    "fasta_single_record": b">only\nACGTACGTAC\n",
}


def golden_texts():
    out = []
    for p in sorted(glob.glob(os.path.join(INPUTS, "*.fast[aq]"))):
        out.append((os.path.basename(p), open(p, "rb").read()))
    return out


def test_golden_inputs_found():
    names = [n for n, _ in golden_texts()]
    assert len(names) == 22, names


@pytest.mark.parametrize("name", [n for n, _ in golden_texts()])
def test_rule_matches_host_parser_on_golden_inputs(name):
    text = open(os.path.join(INPUTS, name), "rb").read()
    fmt = fmt_of(text)
    got, want = rule_bytes(text, fmt), host_batch(text, fmt)
    assert runs(got) == runs(want)
    assert got.strip(b"\n") == want.strip(b"\n") or b"\r" in text
    assert not rule_flag(text, fmt)


@pytest.mark.parametrize("name", sorted(CORNERS))
def test_rule_matches_host_parser_on_corner_texts(name):
    text = CORNERS[name]
    fmt = fmt_of(text)
    got, want = rule_bytes(text, fmt), host_batch(text, fmt)
    assert runs(got) == runs(want), (got, want)
    assert not rule_flag(text, fmt)
    if fmt == FASTQ:
        assert got.count(b"\n") == (text.count(b"\n") + 2) // 4          # one separator per sequence line that has its '\n'


def test_rule_states_the_documented_shapes():
    assert rule_bytes(b"@a\nACGT\n+\nIIII\n@b\nGG\n+\nII\n", FASTQ) == b"ACGT\nGG\n"
    assert rule_bytes(b"@a\r\nACGT\r\n+\r\nIIII\r\n", FASTQ) == b"ACGT\n"
    assert rule_bytes(b">a\nAC\nGT\n>b\nTT\n", FASTA) == b"\nACGT\nTT"
    assert rule_bytes(b">a\r\nAC\r\nGT\r\n", FASTA) == b"\nACGT"
    assert rule_bytes(b"@a\nAC\rGT\n+\nIIIII\n", FASTQ) == b"AC\rGT\n"          # a '\r' that is no EOL-CR stays, as an invalid byte
    assert rule_bytes(b">a\nAC\r\r\nGT\n", FASTA) == b"\nAC\rGT"                # the documented difference from the host parser
    assert rule_bytes(b"", FASTQ) == b""


def test_rule_flags_malformed_texts():
    assert rule_flag(b"@a\nACGT\nACGT\n+\nIIIIIIII\n", FASTQ)                  # wrapped sequence
    assert rule_flag(b"a\nACGT\n+\nIIII\n", FASTQ)
    assert rule_flag(b"ACGT\n>a\nAC\n", FASTA)
    assert not rule_flag(b"@a\nACGT\n+\n@@@@\n", FASTQ)


# ---- the C ABI: symbols and argument checks that need no device ---------------------------------------------------------

NEW_SYMBOLS = ["kq_pack_bases_dev", "kq_parse_fastx_dev", "kq_count_fastx_dev", "kq_count_fastx_async"]


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return capi.load()


def test_new_symbols_listed_and_exported(lib):
    for s in NEW_SYMBOLS:
        assert s in capi.SYMBOLS, s
        assert hasattr(lib, s), s
    assert (capi.FASTX_FASTQ, capi.FASTX_FASTA) == (FASTQ, FASTA)
    hdr = open(os.path.join(os.path.dirname(INPUTS), "..", "..", "include", "kreeq_amd.h")).read()
    assert re.search(r"KQ_FASTX_FASTQ\s*=\s*1\s*,\s*KQ_FASTX_FASTA\s*=\s*2", hdr)
    assert lib.kq_abi_version() == 4


def test_null_and_bad_format_arguments_rejected_without_a_device(lib):
    buf = (C.c_char * 64)()
    n, t = C.c_uint64(7), C.c_uint64(0)
    p = C.cast(buf, C.c_void_p)
    assert lib.kq_pack_bases_dev(None, p, 16, p, p) == -1
    assert lib.kq_parse_fastx_dev(None, p, 16, FASTQ, p, 64, C.byref(n)) == -1
    assert lib.kq_count_fastx_dev(None, p, 16, FASTA) == -1
    assert lib.kq_count_fastx_async(None, p, 16, FASTQ, C.byref(t)) == -1
    assert lib.kq_count_fastx_dev(None, p, 16, 3) == -1
    assert b"null" in lib.kq_last_error() or b"format" in lib.kq_last_error()
