"""bench.py --dump-outputs on the CPU: the read sample is fixed by its seed, and the dump holds exact float64 copies of the
table's entries for the sampled keys of the table's map range, within 64 MB.  The CPU oracle stands in for the GPU table."""
import os

import numpy as np
import pytest
import torch

import bench
from kreeq_amd import synth
from oracle import oracle as O


class OracleTable:
    """kq_lookup_keys' contract on an oracle database: entries of the given keys, cov == 0 when absent"""

    def __init__(self, db):
        self.ent = db.export()

    def lookup_keys(self, keys):
        i = np.minimum(np.searchsorted(self.ent["key"], keys), len(self.ent) - 1)
        out = np.where(self.ent["key"][i] == keys, self.ent[i], np.zeros(1, dtype=self.ent.dtype))
        out["key"] = keys
        return out


@pytest.fixture(scope="module")
def batch():
    n, L = 4000, 150
    reads = synth.reads_batch(synth.genome_codes(300_000, seed=1), n, L, seed=2)
    db = O.OracleDB(21, 128)
    db.count_batch(reads.tobytes())
    return reads, n, L, db


def test_read_sample_is_seeded(batch):
    reads, n, L, _ = batch
    s = bench.sample_reads(torch.from_numpy(reads.copy()), n, L)
    assert s == bench.sample_reads(torch.from_numpy(reads.copy()), n, L)
    assert len(s) == bench.DUMP_READS * (L + 1) - 1
    rows = s.split(b"\n")
    assert len(set(rows)) > bench.DUMP_READS - 10 and all(r in reads.tobytes() for r in rows[:50])


def test_dump_is_exact_bounded_and_repeatable(batch, tmp_path):
    reads, n, L, db = batch
    s = bench.sample_reads(torch.from_numpy(reads.copy()), n, L)
    summ = db.summary(with_hist=True)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), OracleTable(db), 21, s, summ, summ["hist"], (64, 128))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["histogram.npy", "sample_bw.npy", "sample_cov.npy", "sample_fw.npy", "sample_hc.npy", "sample_key.npy", "summary.npy"]
    arr = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    for f in names:
        assert np.array_equal(arr[f[:-4]], np.load(tmp_path / "b" / f))
    assert all(a.dtype == np.float64 for a in arr.values()) and sum(a.nbytes for a in arr.values()) <= 64 << 20
    keys = (arr["sample_key"][:, 0].astype(np.uint64) << np.uint64(32)) | arr["sample_key"][:, 1].astype(np.uint64)
    assert len(keys) > 0 and np.all(np.diff(keys.astype(np.float64)) > 0)
    assert np.all((keys % 128 >= 64) & (keys % 128 < 128))
    want = OracleTable(db).lookup_keys(keys)
    assert np.all(want["cov"] > 0)
    for f in ("fw", "bw", "cov", "hc"):
        assert np.array_equal(arr["sample_" + f], want[f].astype(np.float64))
    assert arr["summary"].tolist() == [summ[f] for f in ("total", "unique", "distinct", "missing", "edges")]
    assert arr["histogram"].tolist() == [list(x) for x in sorted(summ["hist"].items())]
