"""`kreeq validate -o x.kwig|.bkwig|.bed|.csvtable --passes N` with KQ_TABLE_DEVICE=1 and KQ_TABLE_DEVICE_PASSES=1 accumulates the
table on the device over the map ranges and writes the bytes of the host writer's single-pass file, with the same stdout, from
reads and from a database, for 2, 5 and 128 ranges; says so on stderr (no case falls back silently); groups the sequences by
KQ_TABLE_CALL_BYTES; and leaves the table to the host writer, with its reason, when a sequence exceeds that limit or the
device memory exceeds KQ_TABLE_ACC_MAX_BYTES."""
import os
import re
import subprocess

import numpy as np
import pytest

from kreeq_amd import build, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEVICE_LINE, HOST_LINE = "per-base table written by the device formatter", "per-base table written by the host writer"
ACC_LINE = re.compile(r"per-base table accumulated on the device over (\d+) map ranges in (\d+) calls")
FALLBACK_LINE = re.compile(r"per-base table not accumulated on the device \((\d+) bytes\): (.*)")
EXTS = ("kwig", "bkwig", "bed", "csvtable")
PASSES = (2, 5, 128)
GOLDEN = {"decompressor1": ("decompressor1.fasta", "random1.fastq", "decompressor1.bkwig"), "repeat1": ("repeat1.fasta", "repeat1.fastq", "decompressor2.bkwig")}
INPUTS = ("decompressor1", "repeat1", "gen21", "gen31")
KNOBS = ("KQ_TABLE_DEVICE", "KQ_TABLE_DEVICE_PASSES", "KQ_TABLE_CHUNK_LINES", "KQ_TABLE_CALL_BYTES", "KQ_TABLE_ACC_MAX_BYTES")
BOTH = {"KQ_TABLE_DEVICE": "1", "KQ_TABLE_DEVICE_PASSES": "1"}


class Bench:
    """the CLI, the four input sets (assembly, reads, -k arguments), their databases, and the host writer's single-pass runs"""

    def __init__(self, cli, work):
        self.cli, self.work = cli, work
        self.inputs = {name: (H.golden_input(asm), H.golden_input(reads), []) for name, (asm, reads, _) in GOLDEN.items()}
        # three sequences of 70 000 bases with N runs (one at a sequence's start, one at another's end), and 8x reads of them
        g = synth.genome_codes(3 * 70_000, seed=41)
        asm = synth.codes_to_ascii(synth.mutate(g, 0.002, seed=42)).copy()
        rng = np.random.default_rng(43)
        for at in rng.integers(100, len(asm) - 100, 30):
            asm[at:at + int(rng.integers(1, 40))] = ord("N")
        asm[70_000:70_005] = ord("N")
        asm[139_990:140_000] = ord("N")
        fasta, reads = str(work / "gen.fasta"), str(work / "gen_reads.fasta")
        with open(fasta, "wb") as f:
            for i in range(3):
                f.write(b">chr%d\n" % (i + 1) + asm[i * 70_000:(i + 1) * 70_000].tobytes() + b"\n")
        batch = synth.reads_batch(g, 8 * len(g) // 150, 150, seed=44, err=0.005).tobytes().split(b"\n")
        with open(reads, "wb") as f:
            f.write(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(batch)))
        self.inputs["gen21"] = (fasta, reads, ["-k", "21"])
        self.inputs["gen31"] = (fasta, reads, ["-k", "31"])
        self._db, self._host = {}, {}

    def source(self, name, from_db):
        asm, reads, k = self.inputs[name]
        if not from_db:
            return ["-f", asm, "-r", reads] + k
        if name not in self._db:                                          # written by a prior run
            db = str(self.work / (name + ".kreeq"))
            p = subprocess.run([self.cli, "validate", "-r", reads, "-o", db] + k, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, p.stderr
            self._db[name] = db
        return ["-f", asm, "-d", self._db[name]]

    def run(self, name, from_db, out, env_extra=None, extra=()):
        """-> (stdout, stderr, the file's bytes) of one validate run"""
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(env_extra or {})
        p = subprocess.run([self.cli, "validate"] + self.source(name, from_db) + ["-o", out, "--verbose"] + list(extra), capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stderr
        return p.stdout, p.stderr, open(out, "rb").read()

    def host(self, name, from_db, ext):
        """the host writer's single-pass run (computed once, never changed)"""
        key = (name, from_db, ext)
        if key not in self._host:
            so, se, data = self.run(name, from_db, str(self.work / ("host.%s.%d.%s" % (name, from_db, ext))))
            assert HOST_LINE in se and DEVICE_LINE not in se and len(data) > 20
            self._host[key] = (so, data)
        return self._host[key]

    def check_device(self, name, from_db, ext, out, passes, env_extra=None, calls=None):
        """one run of the new path: the host writer's bytes and stdout, and the two device lines"""
        want_out, want = self.host(name, from_db, ext)
        so, se, data = self.run(name, from_db, out, dict(BOTH, **(env_extra or {})), ["--passes", str(passes)])
        m = ACC_LINE.search(se)
        assert DEVICE_LINE in se and m and HOST_LINE not in se and not FALLBACK_LINE.search(se), se      # no silent fall-back
        assert int(m.group(1)) == passes and (calls is None or int(m.group(2)) == calls), m.group(0)
        assert data == want
        assert so == want_out
        return data

    def check_fallback(self, name, ext, out, env_extra, reason):
        want_out, want = self.host(name, False, ext)
        so, se, data = self.run(name, False, out, dict(BOTH, **env_extra), ["--passes", "2"])
        m = FALLBACK_LINE.search(se)
        assert HOST_LINE in se and DEVICE_LINE not in se and not ACC_LINE.search(se) and m, se
        assert int(m.group(1)) > 0 and reason in m.group(2), m.group(0)
        assert data == want and so == want_out


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    assert os.path.exists(build.LIB), "libkreeq_amd.so must be built in-tree"
    return Bench(build.build_cli(), tmp_path_factory.mktemp("table_passes"))


@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("ext", EXTS)
@pytest.mark.parametrize("name", INPUTS)
def test_passes_from_reads(bench, tmp_path, name, ext, passes):
    bench.check_device(name, False, ext, str(tmp_path / ("out." + ext)), passes)


@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("ext", EXTS)
@pytest.mark.parametrize("name", INPUTS)
def test_passes_from_a_database(bench, tmp_path, name, ext, passes):
    bench.check_device(name, True, ext, str(tmp_path / ("out." + ext)), passes)


@pytest.mark.parametrize("ext", EXTS)
def test_group_limit(bench, tmp_path, ext):
    """decompressor1: four sequences of 99 bases (100 bytes of joined text each), two with gaps"""
    out = str(tmp_path / ("out." + ext))
    bench.check_device("decompressor1", False, ext, out, 2, calls=1)
    bench.check_device("decompressor1", False, ext, out, 2, {"KQ_TABLE_CALL_BYTES": "200"}, calls=2)
    bench.check_device("decompressor1", False, ext, out, 2, {"KQ_TABLE_CALL_BYTES": "100"}, calls=4)
    bench.check_fallback("decompressor1", ext, out, {"KQ_TABLE_CALL_BYTES": "99"}, "call limit")


@pytest.mark.parametrize("ext", EXTS)
@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_chunk_edges(bench, tmp_path, name, ext):
    """chunks of 7 lines: cuts inside segments, and with groups of one sequence also chunks that end with their group"""
    out = str(tmp_path / ("out." + ext))
    bench.check_device(name, False, ext, out, 2, {"KQ_TABLE_CHUNK_LINES": "7"})
    bench.check_device(name, False, ext, out, 5, {"KQ_TABLE_CHUNK_LINES": "7", "KQ_TABLE_CALL_BYTES": "100" if name == "decompressor1" else "1000"})


@pytest.mark.parametrize("ext", EXTS)
def test_accumulator_limit(bench, tmp_path, ext):
    bench.check_fallback("repeat1", ext, str(tmp_path / ("out." + ext)), {"KQ_TABLE_ACC_MAX_BYTES": "1"}, "KQ_TABLE_ACC_MAX_BYTES")


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_bkwig(bench, tmp_path, name):
    data = bench.check_device(name, False, "bkwig", str(tmp_path / "out.bkwig"), 2)
    assert data == open(H.golden_input(GOLDEN[name][2]), "rb").read()


def test_opt_in(bench, tmp_path):
    """KQ_TABLE_DEVICE_PASSES alone, or one range, does not take the path"""
    _, se, data = bench.run("repeat1", False, str(tmp_path / "a.kwig"), {"KQ_TABLE_DEVICE_PASSES": "1"}, ["--passes", "2"])
    assert HOST_LINE in se and DEVICE_LINE not in se and data == bench.host("repeat1", False, "kwig")[1]
    _, se, data = bench.run("repeat1", False, str(tmp_path / "b.kwig"), BOTH, ["--passes", "1"])
    assert DEVICE_LINE in se and not ACC_LINE.search(se) and data == bench.host("repeat1", False, "kwig")[1]
