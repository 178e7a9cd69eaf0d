"""gloo tests (no GPU) of the bucket-sharded count path at k = 31 with 8-byte hash-remainder records: the routing code of
kreeq_amd/dist.py is the product's, the per-rank engine is the host stand-in of tests/test_dist_gloo.py taught the record
format of GpuEngine.sharded8 -- one u64 array of (table hash << 8 | two edge indices) plus per-(part, bucket) counts."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import helpers as H
from tests.test_dist_gloo import HostBucketEngine, _free_port

U = np.uint64


def top8_pack(keys, edges, k):
    """records of canonical keys + reference edge bytes: bits 8..63 = the 56 hash bits below the bucket prefix, bits 0..5 = the
    fw / bw edge indices (0..3, 7 = none), and the bucket each record belongs to"""
    from kreeq_amd.dist import table_hash

    h = table_hash(keys, k)
    e = np.asarray(edges, dtype=np.uint8)
    f = np.full(len(e), 7, dtype=np.uint64)
    b = np.full(len(e), 7, dtype=np.uint64)
    for i in range(4):
        f[((e >> (7 - i)) & 1) == 1] = i
        b[((e >> (3 - i)) & 1) == 1] = i
    return (h << U(8)) | f | (b << U(3)), (h >> U(56)).astype(np.int64)


def top8_unpack(recs, buckets, k):
    """-> (canonical keys, reference edge bytes)"""
    from kreeq_amd.dist import key_of_hash

    recs = np.asarray(recs, dtype=np.uint64)
    h = (np.asarray(buckets).astype(np.uint64) << U(56)) | (recs >> U(8))
    f, b = (recs & U(7)).astype(np.int64), ((recs >> U(3)) & U(7)).astype(np.int64)
    e = np.where(f < 4, 1 << (7 - np.minimum(f, 3)), 0) | np.where(b < 4, 1 << (3 - np.minimum(b, 3)), 0)
    return key_of_hash(h, k), e.astype(np.uint8)


class HostTop8Engine(HostBucketEngine):
    """GpuEngine's k = 29..32 bucket mode on the host"""
    sharded5 = False
    sharded8 = True

    def emit_partitioned(self, bases, n_parts, slot=0):
        from kreeq_amd.dist import bucket_range

        keys, edges = self.O.emit_records(self.k, bases.numpy().tobytes())
        recs, b = top8_pack(keys, edges, self.k)
        order = np.argsort(b, kind="stable")                                  # bucket-sorted = grouped by owner
        firsts = [bucket_range(p, n_parts)[0] for p in range(n_parts)] + [256]
        per_bucket = np.bincount(b, minlength=256).astype(np.int64)
        counts = np.array([per_bucket[firsts[p]:firsts[p + 1]].sum() for p in range(n_parts)], dtype=np.int64)
        meta = np.zeros((n_parts, 256), dtype=np.int64)
        for p in range(n_parts):
            meta[p, firsts[p]:firsts[p + 1]] = per_bucket[firsts[p]:firsts[p + 1]]
        return [torch.from_numpy(recs[order].view(np.int64))], counts, torch.from_numpy(meta)

    def insert(self, payload, meta=None):
        assert len(payload) == 1 and meta is not None                         # one payload array plus the bucket counts
        recs = payload[0].numpy().view(np.uint64)
        m = meta.numpy()
        assert int(m.sum()) == len(recs)
        lo, hi = self.window
        assert np.all(m[:, :lo] == 0) and np.all(m[:, hi:] == 0)              # only k-mers of this rank's buckets arrive
        buckets = np.repeat(np.tile(np.arange(256), m.shape[0]), m.reshape(-1))      # the runs are peer-major, bucket-sorted
        keys, edges = top8_unpack(recs, buckets, self.k)
        self.db.insert_records(keys, edges)


def _worker(rank, world, port, k, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kreeq_amd.dist import ShardedCounter, bucket_of, bucket_range

        sc = ShardedCounter(HostTop8Engine(k, 128), k, 128)
        assert sc.bucket_mode and sc.engine.sharded8 and not sc.engine.sharded5
        assert sc.engine.window == bucket_range(rank, world) == (sc.bucket_lo, sc.bucket_hi)
        for b in range(2):
            n_reads = 1500 if rank != 1 else 3            # rank 1 brings a tiny batch: fewer chunks than its peers
            batch, _ = H.synth_reads(n_reads, 100, 30000, seed=1100 + 10 * rank + b, err=0.01, n_rate=0.003)
            sc.count_batch(torch.frombuffer(bytearray(batch), dtype=torch.uint8))
        _, genome = H.synth_reads(10, 100, 30000, seed=1100)
        ctr = sc.validate(torch.frombuffer(bytearray(genome), dtype=torch.uint8))
        summ = sc.summary()
        hist = sc.histogram()
        sc.export_db(os.path.join(out_dir, "sharded.kreeq"))
        ent = sc.engine.db.export()
        b = bucket_of(ent["key"], k)
        assert np.all((b >= sc.bucket_lo) & (b < sc.bucket_hi))
        np.save(os.path.join(out_dir, f"entries_{rank}.npy"), ent)
        if rank == 0:
            np.save(os.path.join(out_dir, "hist.npy"), np.array(sorted(hist.items()), dtype=np.uint64))
            np.save(os.path.join(out_dir, "ctr.npy"), ctr)
            np.save(os.path.join(out_dir, "summ.npy"), np.array([summ[f] for f in ("total", "unique", "distinct", "missing", "edges")], dtype=np.uint64))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded8_count_matches_single(tmp_path, world):
    from oracle import oracle as O

    k = 31
    mp.spawn(_worker, args=(world, _free_port(), k, str(tmp_path)), nprocs=world, join=True)
    ref = O.OracleDB(k, 128)
    for rank in range(world):
        for b in range(2):
            batch, _ = H.synth_reads(1500 if rank != 1 else 3, 100, 30000, seed=1100 + 10 * rank + b, err=0.01, n_rate=0.003)
            ref.count_batch(batch)
    _, genome = H.synth_reads(10, 100, 30000, seed=1100)
    merged = np.concatenate([np.load(os.path.join(tmp_path, f"entries_{r}.npy")) for r in range(world)])
    merged = merged[np.argsort(merged["key"])]
    assert H.entries_equal(merged, ref.export())
    c, _ = ref.validate_sequence(genome)
    assert np.load(os.path.join(tmp_path, "ctr.npy")).tolist() == c.tolist()
    s = ref.summary(with_hist=True)
    assert np.load(os.path.join(tmp_path, "summ.npy")).tolist() == [s[f] for f in ("total", "unique", "distinct", "missing", "edges")]
    assert [tuple(x) for x in np.load(os.path.join(tmp_path, "hist.npy")).tolist()] == sorted(s["hist"].items())
    from kreeq_amd import hostdb

    got, gk, gm = hostdb.read_db(os.path.join(tmp_path, "sharded.kreeq"))
    assert (gk, gm) == (k, 128)
    assert H.entries_equal(got, ref.export())


def test_force_wide_keeps_the_key_edge_path():
    """ShardedCounter(force_wide=True): an engine that could emit hash-remainder records stays on map ownership"""
    from kreeq_amd.dist import ShardedCounter

    sc = ShardedCounter(HostTop8Engine(31, 128), 31, 128, force_wide=True)
    assert not sc.bucket_mode and not sc.engine.sharded8
    assert ShardedCounter(HostTop8Engine(31, 128), 31, 128).bucket_mode


@pytest.mark.parametrize("k", [29, 30, 31, 32])
def test_top8_records_round_trip(k):
    """a record plus its bucket is the whole k-mer: pack -> unpack through key_of_hash gives the canonical key and the edge
    byte back; bits 6..7 of a record are zero, and for k = 29 so are the six hash bits above them (58 significant bits)"""
    rng = np.random.default_rng(k)
    raw = rng.integers(0, 1 << 63, 20_000, dtype=np.uint64) * U(2) + rng.integers(0, 2, 20_000, dtype=np.uint64)
    if k < 32:
        raw &= U((1 << (2 * k)) - 1)
    keys = np.concatenate([H.canonical_keys_of(raw, k), np.array([0, H.max_canonical_key(k)], dtype=np.uint64)])
    # an instance has at most one forward and one backward edge
    f, b = rng.integers(0, 5, len(keys)), rng.integers(0, 5, len(keys))
    edges = (np.where(f < 4, 1 << (7 - np.minimum(f, 3)), 0) | np.where(b < 4, 1 << (3 - np.minimum(b, 3)), 0)).astype(np.uint8)
    recs, buckets = top8_pack(keys, edges, k)
    assert np.all(recs & U(0xC0) == 0) and buckets.min() >= 0 and buckets.max() <= 255
    if k == 29:
        assert np.all(recs & U(0x3F00) == 0)
    back_keys, back_edges = top8_unpack(recs, buckets, k)
    assert np.array_equal(back_keys, keys) and np.array_equal(back_edges, edges)
    assert len(np.unique(recs >> U(8) | (buckets.astype(np.uint64) << U(56)))) == len(np.unique(keys))
