"""Record-input entry points (kq_insert_packed_dev, kq_insert_records_dev, kq_insert_sharded_dev) across the level shapes of
the record split, with the region-sorted set in the partition scratch (KQ_OPT_PENDING_BYTES = 0: applied at once) and in the
pending arena (-1).  Every case inserts the same run twice, the second time into a filled table, and must leave the oracle's
table."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

# capacity_hint, KQ_OPT_NARROW_MID: one narrow level / a middle level / >= 2^16 regions (4-byte FMT_TIGHT sets for 5-byte records)
ONE_LEVEL, MIDDLE, TIGHT = (5_000_000, 0), (5_870_000, 2), (100_000_000, 0)


@pytest.fixture(scope="module")
def kq():
    import kreeq_amd
    if not kreeq_amd.device_available():
        pytest.fail("no gfx950 device: the product has no CPU fallback")
    return kreeq_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    O.build()
    return O


@pytest.fixture(scope="module")
def reads():
    # ~1.4 M records at k = 21: past the 2^20 threshold of the partitioned paths
    return H.synth_reads(10_800, 150, 300_000, seed=500, err=0.01, n_rate=0.002)[0]


@pytest.fixture(scope="module")
def want(O, reads):
    """k -> (export, summary) of the oracle after the reads were counted twice; made once per k"""
    cache = {}

    def get(k):
        if k not in cache:
            cpu = O.OracleDB(k, 128)
            for _ in range(2):
                cpu.count_batch(reads, threads=8)
            cache[k] = (cpu.export(), cpu.summary())
        return cache[k]
    return get


def _receiver(kq, k, geometry, pending):
    hint, mid = geometry
    db = kq.KreeqDB(k, 128, capacity_hint=hint)
    db.set_option("trust_capacity", 1)
    db.set_option("count_path", "partitioned")
    db.set_option("pending_bytes", pending)
    if mid:
        db.set_option("narrow_mid", mid)
    return db


def _device_reads(reads):
    import torch
    return torch.frombuffer(bytearray(reads), dtype=torch.uint8).cuda()


# k = 27 takes 8-byte packed records through coarse bucket -> regions whatever the table: it never reaches a middle level
@pytest.mark.parametrize("pending", [0, -1])
@pytest.mark.parametrize("k,geometry", [(21, ONE_LEVEL), (21, MIDDLE), (21, TIGHT), (27, ONE_LEVEL), (27, TIGHT)])
def test_insert_packed_dev(kq, want, reads, k, geometry, pending):
    import torch

    t = _device_reads(reads)
    recs = torch.empty(t.numel(), dtype=torch.int64, device="cuda")
    n = int(kq.KreeqDB(k, 128).emit_packed_dev(t.data_ptr(), t.numel(), 1, recs.data_ptr(), recs.numel())[0])
    db = _receiver(kq, k, geometry, pending)
    for _ in range(2):
        db.insert_packed_dev(recs.data_ptr(), n)
        db.sync()
    export, summary = want(k)
    assert db.summary() == summary
    assert H.entries_equal(db.export(), export)


# raw keys + edge bytes are WIDE records, never 5-byte ones: no middle level here either
@pytest.mark.parametrize("pending", [0, -1])
@pytest.mark.parametrize("k,geometry", [(21, ONE_LEVEL), (21, TIGHT), (31, ONE_LEVEL), (31, TIGHT)])
def test_insert_records_dev_partitioned(kq, want, reads, k, geometry, pending):
    import torch

    t = _device_reads(reads)
    keys = torch.empty(t.numel(), dtype=torch.int64, device="cuda")
    edges = torch.empty(t.numel(), dtype=torch.uint8, device="cuda")
    n = int(kq.KreeqDB(k, 128).emit_partitioned_dev(t.data_ptr(), t.numel(), 1, keys.data_ptr(), edges.data_ptr(), keys.numel())[0])
    db = _receiver(kq, k, geometry, pending)
    for _ in range(2):
        db.insert_records_dev(keys.data_ptr(), edges.data_ptr(), n)
        db.sync()
    export, summary = want(k)
    assert db.summary() == summary
    assert H.entries_equal(db.export(), export)


@pytest.mark.parametrize("pending", [0, -1])
@pytest.mark.parametrize("geometry", [ONE_LEVEL, MIDDLE, TIGHT])
def test_insert_sharded_dev(kq, want, reads, geometry, pending):
    """2 peers (the halves of the reads) into 2 windowed receivers"""
    import torch

    from kreeq_amd.dist import bucket_of, bucket_range

    k, n_parts = 21, 2
    cut = reads.rfind(b"\n", 0, len(reads) // 2)
    sender = kq.KreeqDB(k, 128)
    runs, metas = [], []
    for b in (reads[:cut], reads[cut + 1:]):
        t = _device_reads(b)
        recs = torch.empty(t.numel(), dtype=torch.int32, device="cuda")
        aux = torch.empty(t.numel(), dtype=torch.uint8, device="cuda")
        meta = torch.empty((n_parts, 256), dtype=torch.int64, device="cuda")
        counts = sender.emit_sharded_dev(t.data_ptr(), t.numel(), n_parts, recs.data_ptr(), aux.data_ptr(), recs.numel(), meta.data_ptr())
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        runs.append([(recs[off[p]:off[p + 1]], aux[off[p]:off[p + 1]]) for p in range(n_parts)])
        metas.append(meta)
    export, summary = want(k)
    bucket = bucket_of(export["key"], k)
    total = dict.fromkeys(summary, 0)
    for p in range(n_parts):
        lo, hi = bucket_range(p, n_parts)
        db = _receiver(kq, k, geometry, pending)
        db.set_option("bucket_window", lo | (hi << 16))
        r = torch.cat([run[p][0] for run in runs])
        a = torch.cat([run[p][1] for run in runs])
        m = torch.stack([meta[p] for meta in metas]).contiguous()
        for _ in range(2):
            db.insert_sharded_dev(r.data_ptr(), a.data_ptr(), r.numel(), len(runs), m.data_ptr())
            db.sync()
        assert H.entries_equal(db.export(), export[(bucket >= lo) & (bucket < hi)])
        for f, v in db.summary().items():
            total[f] += v
    # every shard answers for its buckets only ("missing" counts the key space a shard does not hold)
    assert all(total[f] == summary[f] for f in ("total", "unique", "distinct", "edges"))
