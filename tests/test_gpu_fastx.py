"""The device FASTQ / FASTA parser and the device 2-bit packer through the C ABI (kq_pack_bases_dev, kq_parse_fastx_dev,
kq_count_fastx_dev, kq_count_fastx_async).  Parsed bytes are compared with the byte rule of tests/test_fastx_rule.py,
packed units with kq_pack_bases bit for bit, tables with the CPU oracle's table of the host-style batch."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from tests import helpers as H
from tests.test_fastx_rule import CORNERS, FASTA, FASTQ, fmt_of, golden_texts, host_batch, rule_bytes, rule_flag

pytestmark = pytest.mark.gpu

UNIT = 4096          # bytes of text per scan unit (kq_fastx.h FX_UNIT)


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


def on_device(data: bytes, offset=0):
    """device uint8 tensor holding `data`, its first byte `offset` bytes behind a 16-byte boundary"""
    import torch

    buf = torch.zeros(len(data) + offset + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + len(data)]
    if data:
        view.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    torch.cuda.synchronize()
    return view


def make_fastq(reads, seed, eol=b"\n", final_eol=True, header_len=lambda i, rng: int(rng.integers(1, 40))):
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(reads):
        head = b"@" + (b"r%d " % i + b"x" * 5000)[:max(1, header_len(i, rng))]
        qual = bytes(rng.choice(np.frombuffer(b"@+IIFF#>", dtype=np.uint8), len(r)).tolist())
        out.append(head + eol + r + eol + b"+" + eol + qual + eol)
    text = b"".join(out)
    return text if final_eol else text[:-len(eol)]


def make_fasta(seqs, width, eol=b"\n", final_eol=True, headers=None):
    out = []
    for i, s in enumerate(seqs):
        out.append((headers[i] if headers else b">s%d some text" % i) + eol)
        for a in range(0, len(s), width):
            out.append(s[a:a + width] + eol)
    text = b"".join(out)
    return text if final_eol else text[:-len(eol)]


def split_reads(batch):
    return batch.split(b"\n")


def parse_on_device(db, text, fmt, offset=0):
    import torch

    t = on_device(text, offset)
    n = db.parse_fastx_dev(t.data_ptr(), len(text), fmt, None, 0)
    out = torch.full((n + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n2 = db.parse_fastx_dev(t.data_ptr(), len(text), fmt, out.data_ptr(), n)
    assert n2 == n
    got = out.cpu().numpy()
    assert (got[n:] == 0x5A).all(), "bytes written behind the batch"
    return got[:n].tobytes()


def check_parse(db, text, fmt, offsets=(0,)):
    want = rule_bytes(text, fmt)
    for off in offsets:
        got = parse_on_device(db, text, fmt, off)
        if got != want:
            g, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            m = min(len(g), len(w))
            bad = np.flatnonzero(g[:m] != w[:m])
            first = int(bad[0]) if len(bad) else m
            raise AssertionError(f"offset {off}: {len(got)} bytes, want {len(want)}; first difference at output byte {first}: "
                                 f"{got[max(0, first - 20):first + 20]!r} / {want[max(0, first - 20):first + 20]!r}")


# ---------------------------------------------------------------------------------- 2-bit packing
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4097, 100_003, (1 << 24) + 5])
def test_pack_bases_dev_matches_host_packer(kq, n):
    import torch

    from kreeq_amd import capi

    rng = np.random.default_rng(n)
    raw = rng.choice(np.frombuffer(b"ACGTacgtNn\n-", dtype=np.uint8), n).astype(np.uint8).tobytes()
    want_c, want_i = capi.pack_bases(raw)
    db = kq.KreeqDB(21, 128)
    units = (n + 15) // 16
    for off in ((0, 1, 2, 3) if n < (1 << 20) else (0, 3)):
        t = on_device(raw, off)
        codes = torch.full((units + 4,), -1, dtype=torch.int32, device="cuda")
        inv = torch.full((units + 4,), -1, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        db.pack_bases_dev(t.data_ptr(), n, codes.data_ptr(), inv.data_ptr())
        db.sync()
        c, i = codes.cpu().numpy(), inv.cpu().numpy()
        assert np.array_equal(c[:units].view(np.uint32), want_c), (n, off)
        assert np.array_equal(i[:units].view(np.uint16), want_i), (n, off)
        assert (c[units:] == -1).all() and (i[units:] == -1).all(), (n, off)


def test_pack_dev_kernel_equals_pack_dev(kq):
    import torch

    from kreeq_amd import synth

    rng = np.random.default_rng(77)
    db = kq.KreeqDB(21, 128)
    for n in (1, 16, 33, 1_000_003):
        raw = torch.from_numpy(rng.choice(np.frombuffer(b"ACGTacgtNn\n-", dtype=np.uint8), n).astype(np.uint8)).cuda()
        c1, i1 = synth.pack_dev(raw)
        c2, i2 = synth.pack_dev_kernel(db, raw)
        assert c1.dtype == c2.dtype and i1.dtype == i2.dtype and c1.shape == c2.shape and i1.shape == i2.shape
        assert torch.equal(c1, c2) and torch.equal(i1, i2), n


def test_packed_by_the_device_counts_like_ascii(kq, O):
    import torch

    batch, _ = H.synth_reads(20_000, 150, 300_000, seed=5, err=0.01, n_rate=0.003)
    cpu = O.OracleDB(21, 128)
    cpu.count_batch(batch, threads=8)
    gpu = kq.KreeqDB(21, 128, capacity_hint=4_000_000)
    t = on_device(batch, 2)
    units = (len(batch) + 15) // 16
    codes = torch.empty(units, dtype=torch.int32, device="cuda")
    inv = torch.empty(units, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    gpu.pack_bases_dev(t.data_ptr(), len(batch), codes.data_ptr(), inv.data_ptr())
    gpu.count_packed_dev(codes.data_ptr(), inv.data_ptr(), len(batch))        # same stream: no synchronisation between them
    gpu.sync()
    assert H.entries_equal(gpu.export(), cpu.export())


# ---------------------------------------------------------------------------------- parse: bytes
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
def test_parse_fastq_many_units(kq, eol):
    batch, _ = H.synth_reads(12_000, 150, 100_000, seed=21, err=0.01, n_rate=0.004)
    reads = split_reads(batch)
    reads[7] = b""                                              # an empty sequence line
    reads[100] = reads[100][:40] + b"\r" + reads[100][40:]      # a '\r' inside a sequence line stays
    text = make_fastq(reads, seed=3, eol=eol)
    assert len(text) > 900 * UNIT
    db = kq.KreeqDB(21, 128)
    check_parse(db, text, FASTQ, offsets=(0, 1, 7, 15))
    check_parse(db, make_fastq(reads[:500], seed=4, eol=eol, final_eol=False), FASTQ)


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
def test_parse_fasta_wrapped_long_lines_and_headers(kq, eol):
    rng = np.random.default_rng(9)
    acgt = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)
    seqs = [bytes(rng.choice(acgt, int(n)).tolist()) for n in rng.integers(1, 30_000, 120)]
    seqs[3] = b""                                               # two headers in a row
    heads = [b">s%d " % i + b"h" * int(rng.integers(0, 80)) for i in range(len(seqs))]
    heads[5] = b">long " + b"H>" * 3000                         # a header line longer than a unit, with '>' inside
    text = make_fasta(seqs, 70, eol=eol, headers=heads)
    long_line = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 3_000_000).tolist())
    text += b">chr one line" + eol + long_line + eol + make_fasta(seqs[:10], 61, eol=eol, headers=heads[:10])
    db = kq.KreeqDB(21, 128)
    check_parse(db, text, FASTA, offsets=(0, 3, 9))
    check_parse(db, text[:-len(eol)], FASTA)                    # no final newline
    # a text whose last line is a header, and one that ends inside the long line
    check_parse(db, make_fasta(seqs[:4], 70, eol=eol) + b">last", FASTA)
    cut = text.index(long_line) + 2_000_001
    check_parse(db, text[:cut], FASTA)


@pytest.mark.parametrize("fmt", [FASTQ, FASTA])
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
def test_parse_line_ends_at_unit_edges(kq, fmt, eol):
    """the '\\n' of header, sequence and other lines on, one before and one after unit (4096 B), wave-iteration (1024 B) and
    lane (16 B) edges, for every alignment of the text: the header of record i is padded so that its sequence line ends at
    a chosen position"""
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    db = kq.KreeqDB(21, 128)
    for offset in (0, 1, 15):
        text, targets = b"", []
        for edge in (UNIT, 2 * UNIT, 2 * UNIT + 1024, 3 * UNIT + 16, 5 * UNIT, 6 * UNIT, 7 * UNIT):
            targets += [edge - 2, edge - 1, edge, edge + 1]
        pos = 0
        for i, tgt in enumerate(sorted(set(targets))):
            # record i: its sequence line's '\n' lands at view position `tgt + 2 * UNIT * i` (view = text shifted by `offset`)
            tgt = tgt + 2 * UNIT * i
            seq = bytes(rng.choice(acgt, 50).tolist())
            fixed = (1 + len(eol)) + len(seq) + len(eol)            # '@' / '>' + eol of the header line, sequence + eol
            pad = tgt + 1 - offset - pos - fixed
            assert pad >= 0
            if fmt == FASTQ:
                rec = b"@" + b"p" * pad + eol + seq + eol + b"+" + eol + b"I" * len(seq) + eol
            else:
                rec = b">" + b"p" * pad + eol + seq + eol
            text += rec
            pos += len(rec)
            assert (text.index(seq) + len(seq) + len(eol) - 1 + offset) == tgt
        want = rule_bytes(text, fmt)
        got = parse_on_device(db, text, fmt, offset)
        assert got == want, (offset, len(got), len(want))


@pytest.mark.parametrize("name", sorted(CORNERS))
def test_parse_corner_texts(kq, name):
    text = CORNERS[name]
    db = kq.KreeqDB(21, 128)
    check_parse(db, text, fmt_of(text), offsets=(0, 5))


@pytest.mark.parametrize("name", [n for n, _ in golden_texts()])
def test_parse_golden_inputs(kq, name):
    text = open(os.path.join(H.INPUTS, name), "rb").read()
    db = kq.KreeqDB(21, 128)
    check_parse(db, text, fmt_of(text), offsets=(0, 11))


def test_parse_sizes_and_capacity(kq):
    import torch

    db = kq.KreeqDB(21, 128)
    text = make_fastq(split_reads(H.synth_reads(3000, 100, 50_000, seed=2)[0]), seed=8)
    want = rule_bytes(text, FASTQ)
    t = on_device(text)
    assert db.parse_fastx_dev(t.data_ptr(), len(text), FASTQ, None, 0) == len(want)          # sizing call
    out = torch.full((len(want) + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(kq.KqError) as e:
        db.parse_fastx_dev(t.data_ptr(), len(text), FASTQ, out.data_ptr(), len(want) - 1)
    assert e.value.code == -6 and e.value.needed == len(want)
    assert (out.cpu().numpy() == 0x5A).all()                    # nothing written into a buffer that is too small
    assert db.parse_fastx_dev(t.data_ptr(), len(text), FASTQ, out.data_ptr(), len(want)) == len(want)
    assert out.cpu().numpy()[:len(want)].tobytes() == want
    # len == 0, and bad arguments on a live handle
    assert db.parse_fastx_dev(t.data_ptr(), 0, FASTQ, out.data_ptr(), 8) == 0
    assert db.parse_fastx_dev(0, 0, FASTA, None, 0) == 0
    db.count_fastx_dev(t.data_ptr(), 0, FASTQ)
    for bad_fmt in (0, 3, -1):
        with pytest.raises(kq.KqError) as e:
            db.parse_fastx_dev(t.data_ptr(), len(text), bad_fmt, out.data_ptr(), len(want))
        assert e.value.code == -1
        with pytest.raises(kq.KqError) as e:
            db.count_fastx_dev(t.data_ptr(), len(text), bad_fmt)
        assert e.value.code == -1
    with pytest.raises(kq.KqError) as e:
        db.count_fastx_dev(0, 5, FASTQ)
    assert e.value.code == -1


# ---------------------------------------------------------------------------------- parse + count: tables
def count_texts():
    batch, _ = H.synth_reads(20_000, 150, 250_000, seed=61, err=0.01, n_rate=0.003)
    reads = split_reads(batch)
    genome_like = [b"".join(reads[i:i + 40]) for i in range(0, 4000, 40)]
    return [make_fastq(reads[:9000], seed=1), make_fastq(reads[9000:15_000], seed=2, eol=b"\r\n"),
            make_fasta(genome_like, 60), make_fasta(reads[15_000:], 70, eol=b"\r\n", final_eol=False)]


@pytest.mark.parametrize("k", [21, 31, 5])
def test_count_fastx_dev_equals_oracle(kq, O, k):
    texts = count_texts()
    cpu = O.OracleDB(k, 128)
    gpu = kq.KreeqDB(k, 128, capacity_hint=6_000_000)
    for i, text in enumerate(texts):
        cpu.count_batch(host_batch(text, fmt_of(text)), threads=8)
        t = on_device(text, i)
        gpu.count_fastx_dev(t.data_ptr(), len(text), fmt_of(text))
    gpu.sync()
    assert gpu.summary() == cpu.summary()
    assert H.entries_equal(gpu.export(), cpu.export())


@pytest.mark.parametrize("k", [21, 31, 5])
def test_count_fastx_async_four_threads_two_buffers(kq, O, k):
    from kreeq_amd import capi

    L = capi.load()
    texts = count_texts()
    batch, _ = H.synth_reads(16_000, 120, 250_000, seed=62, err=0.01, n_rate=0.002)
    reads = split_reads(batch)
    texts += [make_fastq(reads[a:a + 2000], seed=a) for a in range(0, 16_000, 2000)]
    cpu = O.OracleDB(k, 128)
    for text in texts:
        cpu.count_batch(host_batch(text, fmt_of(text)), threads=8)
    gpu = kq.KreeqDB(k, 128, capacity_hint=8_000_000)
    cap = max(len(t) for t in texts)
    pool = [L.kq_host_alloc(cap) for _ in range(2)]
    assert all(pool)
    free, tickets = list(range(2)), {}
    cv = threading.Condition()
    errors = []

    def worker(w):
        try:
            for i in range(w, len(texts), 4):
                with cv:
                    while not free:
                        cv.wait()
                    j = free.pop()
                if j in tickets:
                    gpu.host_wait(tickets[j])              # the copy out of this buffer has finished
                C.memmove(pool[j], texts[i], len(texts[i]))
                tickets[j] = gpu.count_fastx_async(pool[j], len(texts[i]), fmt_of(texts[i]))
                with cv:
                    free.append(j)
                    cv.notify()
        except Exception as e:                               # noqa: BLE001 - reported below
            errors.append(e)

    try:
        threads = [threading.Thread(target=worker, args=(w,)) for w in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for tk in tickets.values():
            gpu.host_wait(tk)
        gpu.sync()
        assert gpu.summary() == cpu.summary()
        assert H.entries_equal(gpu.export(), cpu.export())
    finally:
        L.kq_sync(gpu.handle)
        for p in pool:
            L.kq_host_free(p)


def test_count_fastx_with_a_map_range(kq, O):
    texts = count_texts()
    cpu = O.OracleDB(21, 128)
    for text in texts:
        cpu.count_batch(host_batch(text, fmt_of(text)), threads=8)
    want = cpu.export()
    maps = want["key"] % np.uint64(128)
    gpu = kq.KreeqDB(21, 128, capacity_hint=6_000_000)
    gpu.set_option("count_map_range", (32, 96))
    for text in texts:
        t = on_device(text)
        gpu.count_fastx_dev(t.data_ptr(), len(text), fmt_of(text))
    assert H.entries_equal(gpu.export(), want[(maps >= 32) & (maps < 96)])


def test_count_fastx_never_takes_a_stale_count_matrix(kq, O):
    """KQ_OPT_COUNT_MAP_PASSES keeps count matrices keyed on the batch's device address.  The parsed batch lives in a
    library-owned buffer that keeps its address: two DIFFERENT texts of equal length, counted one after the other for each
    range, must each be counted for what they hold"""
    k = 21
    a, _ = H.synth_reads(30_000, 150, 500_000, seed=81, err=0.006)
    b, _ = H.synth_reads(30_000, 150, 500_000, seed=82, err=0.006)
    texts = [make_fastq(split_reads(x), seed=5, header_len=lambda i, rng: 12) for x in (a, b)]
    assert len(texts[0]) == len(texts[1]) and texts[0] != texts[1]
    ref = O.OracleDB(k, 128)
    for x in (a, b):
        ref.count_batch(x, threads=8)
    want = ref.export()
    maps = want["key"] % np.uint64(128)
    gpu = kq.KreeqDB(k, 128, capacity_hint=5_000_000)
    gpu.set_option("trust_capacity", 1)
    gpu.set_option("count_path", "partitioned")
    gpu.set_option("slice_kmers", 1_700_000)
    gpu.set_option("count_map_passes", 2)
    dev = [on_device(t) for t in texts]
    for r in (0, 1, 0):
        gpu.clear()
        gpu.set_option("count_map_range", (r * 64, (r + 1) * 64))
        for t, text in zip(dev, texts):
            gpu.count_fastx_dev(t.data_ptr(), len(text), FASTQ)
        assert H.entries_equal(gpu.export(), want[(maps >= r * 64) & (maps < (r + 1) * 64)]), r


# ---------------------------------------------------------------------------------- malformed text: an error, not a count
WRAPPED_FASTQ = b"@r1\nACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIII\n@r2\nACGTACGTACG\nTTTTGGGGCCC\n+\nIIIIIIIIIII\nIIIIIIIIIII\n"
HEADLESS_FASTA = b"ACGTACGTACGTACGTACGTACGTAC\n>s\nACGTTTGACCAGTAGGACCATTTAGG\n"


@pytest.mark.parametrize("text,fmt,name", [(WRAPPED_FASTQ, FASTQ, "FASTQ"), (HEADLESS_FASTA, FASTA, "FASTA"),
                                           (b"@r\nACGT\n+\nIIII\n" * 3000 + b"@r\nACGT\nACGT\n+\nIIIIIIII\n", FASTQ, "FASTQ")])
def test_malformed_text_is_refused(kq, O, text, fmt, name):
    from kreeq_amd import capi

    L = capi.load()
    assert rule_flag(text, fmt)
    gpu = kq.KreeqDB(21, 128, capacity_hint=1 << 20)
    t = on_device(text, 1)
    with pytest.raises(kq.KqError) as e:
        gpu.parse_fastx_dev(t.data_ptr(), len(text), fmt, None, 0)
    assert e.value.code == -1 and name in str(e.value)
    # device entry: reported by kq_sync, up to kq_clear
    gpu.count_fastx_dev(t.data_ptr(), len(text), fmt)
    for _ in range(2):
        with pytest.raises(kq.KqError) as e:
            gpu.sync()
        assert e.value.code == -1 and name in str(e.value)
    gpu.clear()
    gpu.sync()
    # host entry: the ticket's kq_host_wait and the next kq_sync
    good = make_fastq(split_reads(H.synth_reads(400, 150, 20_000, seed=4)[0]), seed=6)
    buf = L.kq_host_alloc(max(len(text), len(good)))
    assert buf
    try:
        C.memmove(buf, text, len(text))
        tk = gpu.count_fastx_async(buf, len(text), fmt)
        with pytest.raises(kq.KqError) as e:
            gpu.host_wait(tk)
        assert e.value.code == -1 and name in str(e.value)
        with pytest.raises(kq.KqError) as e:
            gpu.sync()
        assert e.value.code == -1 and name in str(e.value)
        # after kq_clear the handle counts a good text correctly
        gpu.clear()
        C.memmove(buf, good, len(good))
        tk = gpu.count_fastx_async(buf, len(good), FASTQ)
        gpu.host_wait(tk)
        gpu.sync()
        cpu = O.OracleDB(21, 128)
        cpu.count_batch(host_batch(good, FASTQ))
        assert gpu.summary() == cpu.summary()
        assert H.entries_equal(gpu.export(), cpu.export())
    finally:
        L.kq_sync(gpu.handle)                              # (whatever it returns: nothing reads the buffer any more)
        L.kq_host_free(buf)
