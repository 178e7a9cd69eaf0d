"""The CLI's device ingest mode (KQ_INGEST_DEVICE=1): plain FASTQ / FASTA files travel to the GPU as raw text and are
parsed there (kq_count_fastx_async).  Whatever the default mode prints, this mode prints; the KQ_INGEST_TRACE line proves
which path ran (the knob is an environment variable: a build without the mode would ignore it silently)."""
import os
import re
import subprocess

import numpy as np
import pytest

from kreeq_amd import build
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(build.LIB), "libkreeq_amd.so must be built in-tree"
    return build.build_cli()


def run(cli, args, env=None):
    p = subprocess.run([cli] + args, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr
    return p.stdout.split("\n"), p.stderr


def device_submits(stderr):
    m = re.findall(r"device-parsed submits (\d+)", stderr)
    assert m, "no KQ_INGEST_TRACE line with the device-parsed submits:\n" + stderr
    return sum(int(x) for x in m)


def both_modes(cli, args, extra_env=None):
    """-> (stdout of the default mode, stdout of the device mode, device-parsed submits)"""
    env = dict(os.environ, **(extra_env or {}))
    env.pop("KQ_INGEST_DEVICE", None)
    base, _ = run(cli, args, env=env)
    got, err = run(cli, args, env=dict(env, KQ_INGEST_DEVICE="1", KQ_INGEST_TRACE="1"))
    return base, got, device_submits(err)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """the 30 000-read FASTQ of test_cli_ingest_modes_agree (lower-case and N reads), the same with CRLF, the genome as
    FASTA, and the reads as a wrapped multi-record FASTA"""
    d = tmp_path_factory.mktemp("device_ingest")
    rng = np.random.default_rng(77)
    genome = rng.integers(0, 4, 400_000)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    paths = {k: str(d / k) for k in ("r.fastq", "r_crlf.fastq", "g.fasta", "r_wrapped.fasta")}
    with open(paths["r.fastq"], "wb") as f, open(paths["r_crlf.fastq"], "wb") as fc, open(paths["r_wrapped.fasta"], "wb") as fw:
        for i in range(30_000):
            p0 = int(rng.integers(0, len(genome) - 150))
            seq = acgt[genome[p0:p0 + 150]].copy()
            if i % 97 == 0:
                seq[int(rng.integers(0, 150))] = ord("N")
            sb = seq.tobytes().lower() if i % 5 == 0 else seq.tobytes()
            f.write(b"@r%d\n" % i + sb + b"\n+\n" + b"I" * 150 + b"\n")
            fc.write(b"@r%d\r\n" % i + sb + b"\r\n+\r\n" + b"I" * 150 + b"\r\n")
            fw.write(b">r%d wrapped\n" % i + sb[:60] + b"\n" + sb[60:120] + b"\n" + sb[120:] + b"\n")
    with open(paths["g.fasta"], "wb") as f:
        f.write(b">c\n" + acgt[genome].tobytes() + b"\n")
    return paths


@pytest.mark.parametrize("reads", ["r.fastq", "r_crlf.fastq", "r_wrapped.fasta"])
def test_device_mode_prints_what_the_default_mode_prints(cli, inputs, reads):
    base, got, n_dev = both_modes(cli, ["validate", "-f", inputs["g.fasta"], "-r", inputs[reads], "-j", "7"])
    assert got == base and base[0] == "DBG Summary statistics:"
    assert n_dev > 0


def test_all_read_files_give_the_same_table(cli, inputs):
    outs = [both_modes(cli, ["validate", "-f", inputs["g.fasta"], "-r", inputs[r], "-j", "5"])[1] for r in ("r.fastq", "r_crlf.fastq", "r_wrapped.fasta")]
    assert outs[0] == outs[1] == outs[2]


def test_device_mode_two_small_buffers(cli, inputs):
    base, got, n_dev = both_modes(cli, ["validate", "-f", inputs["g.fasta"], "-r", inputs["r.fastq"], "-j", "7"],
                                  {"KQ_INGEST_BUFFERS": "2", "KQ_INGEST_CAP_MB": "1"})
    assert got == base and base[0] == "DBG Summary statistics:"
    assert n_dev >= 9                                           # 9.6 MB of text through 1 MiB buffers


def test_device_mode_map_range_passes(cli, inputs):
    base, got, n_dev = both_modes(cli, ["validate", "-f", inputs["g.fasta"], "-r", inputs["r.fastq"], "-j", "4", "--passes", "2"])
    assert got == base and base[0] == "DBG Summary statistics:"
    assert n_dev > 0
    single, _ = run(cli, ["validate", "-f", inputs["g.fasta"], "-r", inputs["r.fastq"], "-j", "4"])
    assert [l for l in got if l][:6] == [l for l in single if l][:6]


def test_device_mode_writes_the_same_database(cli, inputs, tmp_path):
    from kreeq_amd import hostdb

    dbs = []
    for mode, env in (("host", {}), ("device", {"KQ_INGEST_DEVICE": "1", "KQ_INGEST_TRACE": "1"})):
        db = str(tmp_path / f"{mode}.kreeq")
        e = dict(os.environ, **env)
        if mode == "host":
            e.pop("KQ_INGEST_DEVICE", None)
        out, err = run(cli, ["validate", "-r", inputs["r.fastq"], "-o", db, "-j", "6"], env=e)
        if mode == "device":
            assert device_submits(err) > 0
        dbs.append((out, hostdb.read_db(db)))
    (o1, (e1, k1, m1)), (o2, (e2, k2, m2)) = dbs
    assert o1 == o2 and (k1, m1) == (k2, m2) == (21, 128)
    assert len(e1) > 300_000 and H.entries_equal(e1, e2)


def test_device_mode_record_longer_than_a_pool_buffer(cli, tmp_path):
    """the chromosome-in-a-FASTA input of test_cli_sequence_longer_than_a_pool_buffer: the short records go through the device
    parser, the 3 Mbp record through the host path in a buffer of its own, whole"""
    from oracle import oracle as O

    rng = np.random.default_rng(9)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    long_seq = acgt[rng.integers(0, 4, 3_000_000)].tobytes()
    short = [acgt[rng.integers(0, 4, 200)].tobytes() for _ in range(50)]
    fa = str(tmp_path / "chr.fasta")
    with open(fa, "wb") as f:
        for i, s in enumerate(short[:25]):
            f.write(b">s%d\n" % i + s + b"\n")
        f.write(b">chr\n")
        for i in range(0, len(long_seq), 80):
            f.write(long_seq[i:i + 80] + b"\n")
        for i, s in enumerate(short[25:]):
            f.write(b">t%d\n" % i + s + b"\n")
    db = O.OracleDB(21, 128)
    db.count_batch(b"\n".join(short[:25] + [long_seq] + short[25:]), threads=8)
    want = H.stats_block(db.summary())
    env = dict(os.environ, KQ_INGEST_CAP_MB="1", KQ_INGEST_BUFFERS="3", KQ_INGEST_DEVICE="1", KQ_INGEST_TRACE="1")
    got, err = run(cli, ["validate", "-r", fa, "-j", "4"], env=env)
    assert [l for l in got if l] == want
    assert device_submits(err) > 0


def test_gzipped_reads_stay_on_the_host_path(cli):
    gz, plain = H.golden_input("random1.fastq.gz"), H.golden_input("random1.fastq")
    env = dict(os.environ, KQ_INGEST_DEVICE="1", KQ_INGEST_TRACE="1")
    got, err = run(cli, ["validate", "-r", gz], env=env)
    assert device_submits(err) == 0
    got_plain, err_plain = run(cli, ["validate", "-r", plain], env=env)
    assert device_submits(err_plain) > 0
    assert got == got_plain and got[0] == "DBG Summary statistics:"


@pytest.mark.parametrize("where", ["first", "later"])
def test_wrapped_fastq_is_refused(cli, tmp_path, where):
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    fq = str(tmp_path / "wrapped.fastq")
    with open(fq, "wb") as f:
        for i in range(2000):
            s = acgt[rng.integers(0, 4, 120)].tobytes()
            if (where == "first" and i == 0) or (where == "later" and i == 1500):
                f.write(b"@w%d\n" % i + s[:60] + b"\n" + s[60:] + b"\n+\n" + b"I" * 60 + b"\n" + b"I" * 60 + b"\n")
            else:
                f.write(b"@r%d\n" % i + s + b"\n+\n" + b"I" * 120 + b"\n")
    env = dict(os.environ, KQ_INGEST_DEVICE="1", KQ_INGEST_TRACE="1")
    p = subprocess.run([cli, "validate", "-r", fq, "-j", "3"], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode != 0
    assert "malformed FASTQ" in p.stderr, p.stderr
