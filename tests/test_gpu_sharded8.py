"""k = 29..32 sharded by hash-prefix bucket with 8-byte hash-remainder records: kq_emit_sharded8_dev / kq_insert_sharded8_dev
and KQ_OPT_SHARD_WINDOW (include/kreeq_amd.h), one process standing in for the ranks.  What test_sharded5_emit_exchange_insert
and test_bucket_window_rules (tests/test_gpu_parity.py) check for k <= 21, for the HiFi k."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

HINT = 5_000_000
GENOME = 300_000


@pytest.fixture(scope="module")
def kq():
    import kreeq_amd
    from kreeq_amd import build

    build.build_lib()
    return kreeq_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O

    O.build()
    return O


def _window(lo, hi):
    return lo | (hi << 16)


def _batches(n_peers, tiny_peer=None):
    """one batch per peer (reads of 150 bp, <= 10^4 per batch); the first one also holds a read 300 times: its k-mers reach
    the high-copy tier through the sharded insert.  tiny_peer: that peer brings three reads, so most of its runs are empty"""
    out = []
    for q in range(n_peers):
        n = 3 if q == tiny_peer else 6000 + 500 * q
        b = H.synth_reads(n, 150, GENOME, seed=800 + q, err=0.01, n_rate=0.002)[0]
        if q == 0:
            b = b + b"\n" + b"\n".join([b[:150].upper()] * 300)
        out.append(b)
    return out


_ORACLE = {}


def _oracle(O, k, n_peers, tiny_peer=None, twice=True):
    """the oracle's table of the peers' batches (every run inserted twice), its buckets, counters and summary -- once per key"""
    from kreeq_amd.dist import bucket_of

    key = (k, n_peers, tiny_peer, twice)
    if key not in _ORACLE:
        cpu = O.OracleDB(k, 128)
        for b in _batches(n_peers, tiny_peer):
            for _ in range(2 if twice else 1):
                cpu.count_batch(b, threads=8)
        want = cpu.export()
        _, genome = H.synth_reads(10, 150, GENOME, seed=800)
        _ORACLE[key] = (want, bucket_of(want["key"], k), cpu.validate_sequence(genome)[0], cpu.summary(), genome)
        cpu.close()
    return _ORACLE[key]


def _emit(kq, sender, batch, n_parts, dev):
    """-> (per-part runs, meta [n_parts, 256]) of one batch, with the emit contract checked"""
    import torch

    from kreeq_amd.dist import bucket_range

    t = torch.frombuffer(bytearray(batch), dtype=torch.uint8).to(dev)
    recs = torch.empty(t.numel(), dtype=torch.int64, device=dev)
    meta = torch.empty((n_parts, 256), dtype=torch.int64, device=dev)
    counts = sender.emit_sharded8_dev(t.data_ptr(), t.numel(), n_parts, recs.data_ptr(), recs.numel(), meta.data_ptr())
    assert meta.sum(dim=1).cpu().tolist() == counts.tolist()
    for p in range(n_parts):                      # a part's counts lie in its bucket range only
        lo, hi = bucket_range(p, n_parts)
        assert int(meta[p, :lo].sum()) == 0 and int(meta[p, hi:].sum()) == 0
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return [recs[off[p]:off[p + 1]].clone() for p in range(n_parts)], meta.clone()


def _exchange_and_check(kq, O, k, n_parts, n_peers, narrow_mid=None, tiny_peer=None):
    import torch

    from kreeq_amd.dist import bucket_range

    want, want_bucket, c_cpu, ref, genome = _oracle(O, k, n_peers, tiny_peer)
    dev = torch.device("cuda", 0)
    sender = kq.KreeqDB(k, 128)                   # a sender needs no particular table
    sent = [_emit(kq, sender, b, n_parts, dev) for b in _batches(n_peers, tiny_peer)]
    if tiny_peer is not None:                     # some (peer, bucket) runs are empty
        lo, hi = bucket_range(0, n_parts)
        assert int((sent[tiny_peer][1][0, lo:hi] == 0).sum()) > 0
    total = 0
    ctr_direct, ctr_part = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
    summ = {"total": 0, "unique": 0, "distinct": 0, "edges": 0}
    for p in range(n_parts):
        recv = kq.KreeqDB(k, 128, capacity_hint=HINT)
        recv.set_option("trust_capacity", 1)
        if narrow_mid is not None:
            recv.set_option("narrow_mid", narrow_mid)
        lo, hi = bucket_range(p, n_parts)
        if n_parts > 1:
            before = recv.info()["slots_total"]
            recv.set_option("shard_window", _window(lo, hi))
            assert before <= recv.info()["slots_total"] <= 2 * before + (1 << 22)      # the window keeps the memory kq_create sized (rounded up)
        r = torch.cat([sent[q][0][p] for q in range(n_peers)])
        m = torch.stack([sent[q][1][p] for q in range(n_peers)]).contiguous()
        torch.cuda.synchronize()                  # (the library works on its own stream)
        recv.insert_sharded8_dev(r.data_ptr(), r.numel(), n_peers, m.data_ptr())
        recv.insert_sharded8_dev(r.data_ptr(), r.numel(), n_peers, m.data_ptr())       # a second, pending-set round on the filled table
        got = recv.export()
        mine = want[(want_bucket >= lo) & (want_bucket < hi)]
        assert H.entries_equal(got, mine)
        total += len(got)
        s = recv.summary()
        for f in summ:
            summ[f] += s[f]
        recv.set_option("lookup_path", "direct")
        ctr_direct += recv.lookup_sequence(genome)[0]
        recv.set_option("lookup_path", "partitioned")
        ctr_part += recv.lookup_sequence(genome)[0]
        sub = recv.export(32, 96)                 # map-range export of a shard (the database writer of the multi-GPU driver)
        mm = mine["key"] % np.uint64(128)
        assert H.entries_equal(sub, mine[(mm >= 32) & (mm < 96)])
    assert total == len(want)
    assert int(want["hc"].sum()) > 0              # the repeated read reached the high-copy tier
    assert np.array_equal(ctr_direct, c_cpu) and np.array_equal(ctr_part, c_cpu)
    assert all(summ[f] == ref[f] for f in summ)


@pytest.mark.parametrize("k,n_parts,n_peers", [(31, 3, 2),     # ranges that do not divide 256
                                               (29, 2, 1),     # the six low hash bits of a record are zero
                                               (32, 5, 4),     # all 56 remainder bits, a full 64-bit canonical key
                                               (30, 8, 3),
                                               (31, 1, 2)])    # one part: an ordinary (unwindowed) table
def test_sharded8_emit_exchange_insert(kq, O, k, n_parts, n_peers):
    """n_peers senders split their reads by hash-prefix bucket (kq_emit_sharded8_dev), each of n_parts receivers -- the window
    of its buckets (KQ_OPT_SHARD_WINDOW) -- gets its run from every peer plus the per-bucket counts and inserts them twice
    (kq_insert_sharded8_dev).  Every receiver holds exactly the oracle's k-mers of its buckets; counters and summaries add up."""
    _exchange_and_check(kq, O, k, n_parts, n_peers)


def test_sharded8_middle_level(kq, O):
    """KQ_OPT_NARROW_MID = 2 on receivers of 28 regions per bucket (two parts: a window of 128 buckets over the 3584 regions
    a hint of 5 M gives): 28 = 4 x 7, so the received runs first go through a middle level of 4 sub-buckets per bucket"""
    _exchange_and_check(kq, O, 31, 2, 2, narrow_mid=2)


def test_sharded8_empty_runs(kq, O):
    """one peer brings three reads: most of its (peer, bucket) runs are empty segments of the first level"""
    _exchange_and_check(kq, O, 31, 3, 3, tiny_peer=1)


def test_sharded8_lazy_emit(kq):
    """part_counts == NULL only enqueues: the part sizes are the row sums of the device bucket counts"""
    import torch

    from kreeq_amd.dist import bucket_range

    dev = torch.device("cuda", 0)
    db = kq.KreeqDB(31, 128)
    t = torch.frombuffer(bytearray(_batches(1)[0]), dtype=torch.uint8).to(dev)
    for n_parts in (1, 3):
        recs = torch.empty(t.numel(), dtype=torch.int64, device=dev)
        meta = torch.empty((n_parts, 256), dtype=torch.int64, device=dev)
        counts = db.emit_sharded8_dev(t.data_ptr(), t.numel(), n_parts, recs.data_ptr(), recs.numel(), meta.data_ptr())
        recs2, meta2 = torch.zeros_like(recs), torch.full_like(meta, -1)
        torch.cuda.synchronize()                  # (the library works on its own stream)
        assert db.emit_sharded8_dev(t.data_ptr(), t.numel(), n_parts, recs2.data_ptr(), recs2.numel(), meta2.data_ptr(), sync=False) is None
        db.sync()
        assert meta2.sum(dim=1).cpu().tolist() == counts.tolist()
        assert torch.equal(meta, meta2)
        for p in range(n_parts):
            lo, hi = bucket_range(p, n_parts)
            assert int(meta2[p, :lo].abs().sum()) == 0 and int(meta2[p, hi:].abs().sum()) == 0
        # bucket-sorted: the runs hold the same records whatever the order inside a bucket
        n = int(counts.sum())
        assert torch.equal(torch.sort(recs[:n])[0], torch.sort(recs2[:n])[0])
        assert int((recs[:n] & 0xC0).abs().sum()) == 0         # bits 6..7 of a record are zero


def test_shard_window_rules(kq, O):
    """KQ_OPT_SHARD_WINDOW: KQ_OPT_BUCKET_WINDOW's rules, for k <= 21 and k = 29..32; a windowed k = 31 handle drops foreign
    k-mers on every count path, keeps its window through growth, answers cov 0 for a foreign key, and merges with its like"""
    from kreeq_amd.dist import bucket_of

    k = 31
    b, _ = H.synth_reads(9000, 150, 200_000, seed=41, err=0.01, n_rate=0.002)
    with pytest.raises(kq.KqError) as e:
        kq.KreeqDB(25, 128, capacity_hint=HINT).set_option("shard_window", _window(0, 128))
    assert e.value.code == -1 and "22" in str(e.value) and "28" in str(e.value)
    kq.KreeqDB(21, 128, capacity_hint=HINT).set_option("shard_window", _window(0, 128))      # k <= 21: option 10's path
    db = kq.KreeqDB(k, 128, capacity_hint=HINT)
    with pytest.raises(kq.KqError):
        db.set_option("shard_window", _window(7, 7))             # empty range
    with pytest.raises(kq.KqError):
        db.set_option("shard_window", _window(200, 257))         # beyond the 256 buckets
    db.set_option("shard_window", _window(0, 128))               # k = 31 is accepted ...
    slots = db.info()["slots_total"]
    db.set_option("shard_window", _window(128, 256))             # ... moves to a window of the same width in place ...
    assert db.info()["slots_total"] == slots
    db.set_option("shard_window", _window(0, 256))               # ... and becomes an ordinary table again
    db.count_batch(b)
    with pytest.raises(kq.KqError):
        db.set_option("shard_window", _window(0, 128))           # not empty any more
    cpu = O.OracleDB(k, 128)
    cpu.count_batch(b, threads=8)
    want = cpu.export()
    wb = bucket_of(want["key"], k)
    assert H.entries_equal(db.export(), want)
    mine = want[(wb >= 100) & (wb < 171)]
    foreign = want[(wb < 100) | (wb >= 171)]
    cpu2 = O.OracleDB(k, 128)
    grow = [H.synth_reads(9000, 150, 2_000_000, seed=60 + i, err=0.01)[0] for i in range(3)]
    for bi in grow:
        cpu2.count_batch(bi, threads=8)
    w2 = cpu2.export()
    w2b = bucket_of(w2["key"], k)
    shards = []
    for path in ("direct", "partitioned"):
        win = kq.KreeqDB(k, 128, capacity_hint=HINT)
        win.set_option("shard_window", _window(100, 171))
        win.set_option("count_path", path)
        win.count_batch(b)
        assert H.entries_equal(win.export(), mine)
        look = win.lookup_keys(np.concatenate([foreign["key"][:50], mine["key"][:50]]))
        assert np.all(look["cov"][:50] == 0) and np.array_equal(look["cov"][50:], mine["cov"][:50])
        shards.append(win)
        # growth keeps the window (no trust_capacity: the worst-case reservation of the later batches forces a rehash)
        small = kq.KreeqDB(k, 128, capacity_hint=1_000_000)
        small.set_option("shard_window", _window(100, 171))
        small.set_option("count_path", path)
        slots0 = small.info()["slots_total"]
        for bi in grow:
            small.count_batch(bi)
        assert H.entries_equal(small.export(), w2[(w2b >= 100) & (w2b < 171)])
        assert small.info()["slots_total"] > slots0
    # kq_merge of two shards with the same window, per-entry and region by region
    cpu.count_batch(b, threads=8)
    twice = cpu.export()
    tb = bucket_of(twice["key"], k)
    for merge_path in ("direct", "partitioned"):
        dst = kq.KreeqDB(k, 128, capacity_hint=HINT)
        dst.set_option("shard_window", _window(100, 171))
        dst.set_option("merge_path", merge_path)
        dst.merge(shards[0])
        dst.merge(shards[1])
        assert H.entries_equal(dst.export(), twice[(tb >= 100) & (tb < 171)])


def test_sharded8_argument_errors(kq):
    """the error contract of the 5-byte entries; the handle stays usable after each refusal"""
    import torch

    dev = torch.device("cuda", 0)
    b = _batches(1)[0][:20_000]
    t = torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    recs = torch.empty(t.numel(), dtype=torch.int64, device=dev)
    meta = torch.zeros((2, 256), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()                      # (the library works on its own stream)
    for k in (21, 27):                            # neither format of k <= 28 is a hash remainder
        db = kq.KreeqDB(k, 128, capacity_hint=HINT)
        with pytest.raises(kq.KqError) as e:
            db.emit_sharded8_dev(t.data_ptr(), t.numel(), 2, recs.data_ptr(), recs.numel(), meta.data_ptr())
        assert e.value.code == -1
        with pytest.raises(kq.KqError) as e:
            db.insert_sharded8_dev(recs.data_ptr(), 100, 2, meta.data_ptr())
        assert e.value.code == -1
        db.count_batch(b)
        assert db.summary()["total"] > 0
    db = kq.KreeqDB(31, 128, capacity_hint=HINT)
    n_kmers = t.numel() - 31 + 1
    with pytest.raises(kq.KqError) as e:          # cap one short
        db.emit_sharded8_dev(t.data_ptr(), t.numel(), 2, recs.data_ptr(), n_kmers - 1, meta.data_ptr())
    assert e.value.code == -6
    for bad_parts in (0, 257):
        with pytest.raises(kq.KqError) as e:
            db.emit_sharded8_dev(t.data_ptr(), t.numel(), bad_parts, recs.data_ptr(), recs.numel(), meta.data_ptr())
        assert e.value.code == -1
    with pytest.raises(kq.KqError) as e:          # null record buffer
        db.emit_sharded8_dev(t.data_ptr(), t.numel(), 2, 0, recs.numel(), meta.data_ptr())
    assert e.value.code == -6
    meta.fill_(7)
    torch.cuda.synchronize()
    counts = db.emit_sharded8_dev(t.data_ptr(), 30, 2, recs.data_ptr(), recs.numel(), meta.data_ptr())      # len < k
    assert counts.tolist() == [0, 0] and int(meta.abs().sum()) == 0
    counts = db.emit_sharded8_dev(t.data_ptr(), t.numel(), 2, recs.data_ptr(), n_kmers, meta.data_ptr())    # cap exact: accepted
    assert 0 < int(counts.sum()) <= n_kmers
    # a table below 2048 regions has no bucket split: refused, the message names the fallback
    small = kq.KreeqDB(31, 128)
    assert small.info()["slots_total"] // 2048 < 2048
    with pytest.raises(kq.KqError) as e:
        small.insert_sharded8_dev(recs.data_ptr(), int(counts.sum()), 1, meta.data_ptr())
    assert e.value.code == -1 and "kq_insert_records_dev" in str(e.value)
    small.count_batch(b)
    db.count_batch(b)
    assert small.summary() == db.summary()


def test_sharded8_scanner_edge_reads(kq):
    """the reads of tests/scan_inputs.py (run ends on tile and lane edges, N runs, lower case) at an unaligned device address
    through emit -> insert at k = 31 with two parts: the shards together are the oracle's table of those reads"""
    import torch

    from kreeq_amd.dist import bucket_of, bucket_range
    from tests import scan_inputs as S

    k, lead, n_parts = 31, 1, 2
    ref = S.reference(k, lead)
    dev = torch.device("cuda", 0)
    store = torch.zeros(len(ref.reads) + 256, dtype=torch.uint8, device=dev)
    at = (-store.data_ptr()) % 16 + 64 + lead     # the scanner's window starts `lead` bytes in front of the text
    t = store[at:at + len(ref.reads)]
    t.copy_(torch.frombuffer(bytearray(ref.reads), dtype=torch.uint8))
    assert t.data_ptr() % 16 == lead
    torch.cuda.synchronize()                      # (the library works on its own stream)
    runs, meta = _emit(kq, kq.KreeqDB(k, S.MAP), ref.reads, n_parts, dev)
    recs = torch.empty(t.numel(), dtype=torch.int64, device=dev)
    meta2 = torch.empty((n_parts, 256), dtype=torch.int64, device=dev)
    counts = kq.KreeqDB(k, S.MAP).emit_sharded8_dev(t.data_ptr(), t.numel(), n_parts, recs.data_ptr(), recs.numel(), meta2.data_ptr())
    assert torch.equal(meta, meta2)               # the alignment of the input changes nothing
    wb = bucket_of(ref.table["key"], k)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = 0
    for p in range(n_parts):
        lo, hi = bucket_range(p, n_parts)
        recv = kq.KreeqDB(k, S.MAP, capacity_hint=HINT)
        recv.set_option("shard_window", _window(lo, hi))
        r = recs[off[p]:off[p + 1]].clone()
        m = meta2[p:p + 1].contiguous()
        torch.cuda.synchronize()
        recv.insert_sharded8_dev(r.data_ptr(), r.numel(), 1, m.data_ptr())
        got = recv.export()
        assert H.entries_equal(got, ref.table[(wb >= lo) & (wb < hi)])
        total += len(got)
    assert total == len(ref.table)
