"""Handle lifecycle: three handles created, grown, used and destroyed one after the other in one process -- every resource of
a handle belongs to an owner that `kq_destroy` lets go (kreeq_amd/csrc/kq_mem_host.h), and a table that grows or moves to
another window swaps owners.  Each life counts the same reads from a tiny capacity hint (the main table grows several
times), exports with too little and with enough room, looks the genome up per base, runs two map-range passes over a resident
batch and clears.  Everything is compared with the CPU oracle, exactly.

(At this table size a map-range pass takes the generic filter; the count matrices that KQ_OPT_COUNT_MAP_PASSES keeps on a
bucketed table are covered by test_gpu_fastx / test_gpu_p1_compact / test_gpu_regions.  Here the option is set and reset on a
handle that goes on living.)"""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

K, MAPS, HINT = 21, 128, 4096
GENOME, READ_LEN = 200_000, 150
N_READS = 2 * GENOME // READ_LEN                # 2x coverage
KQ_ERR_CAPACITY = -6


@pytest.fixture(scope="module")
def kq():
    import kreeq_amd

    if not kreeq_amd.device_available():
        pytest.fail("no gfx950 device: the product path has no CPU fallback")
    return kreeq_amd


@pytest.fixture(scope="module")
def job():
    """the reads in four batches (cut at read ends), the genome, and the oracle's answers"""
    from oracle import oracle as O

    reads, genome = H.synth_reads(N_READS, READ_LEN, GENOME, seed=77, err=0.005, n_rate=0.002)
    cuts = [0] + [reads.rfind(b"\n", 0, len(reads) * i // 4) for i in (1, 2, 3)] + [len(reads)]
    batches = [reads[cuts[i] + (1 if i else 0):cuts[i + 1]] for i in range(4)]
    assert b"\n".join(batches) == reads
    cpu = O.OracleDB(K, MAPS)
    for b in batches:
        cpu.count_batch(b, threads=8)
    want = cpu.export()
    counters, per_base = cpu.validate_sequence(genome, per_base=True, threads=8)
    cpu.count_batch(batches[1], threads=8)      # the resident batch once more: its two map-range passes together
    return {"batches": batches, "genome": genome, "want": want, "counters": counters, "per_base": per_base, "want_twice": cpu.export()}


def count_all(db, batches):
    for b in batches:
        db.count_batch(b)


@pytest.mark.parametrize("count_path", ["direct", "partitioned", None])
def test_life(kq, job, count_path):
    import torch

    from kreeq_amd import capi

    want = job["want"]
    db = kq.KreeqDB(K, MAPS, capacity_hint=HINT)
    try:
        if count_path:
            db.set_option("count_path", count_path)
        slots0 = db.info()["slots_total"]
        count_all(db, job["batches"])
        assert db.info()["slots_total"] >= 4 * slots0          # the main table grew at least twice
        assert H.entries_equal(db.export(), want)
        # export: one entry short, then with room
        n = C.c_uint64(0)
        out = np.zeros(len(want), dtype=capi.ENTRY_DTYPE)
        rc = capi.load().kq_export(db.handle, 0, MAPS, out.ctypes.data_as(C.c_void_p), len(want) - 1, C.byref(n))
        assert rc == KQ_ERR_CAPACITY and n.value == len(want)
        n = C.c_uint64(0)
        rc = capi.load().kq_export(db.handle, 0, MAPS, out.ctypes.data_as(C.c_void_p), len(want), C.byref(n))
        assert rc == 0 and n.value == len(want)
        assert np.all(out["key"][1:] > out["key"][:-1])
        assert H.entries_equal(out, want)
        # per-base lookup of the genome
        ctr, pb = db.lookup_sequence(job["genome"], per_base=True)
        assert np.array_equal(ctr, job["counters"])
        for f in ("fw", "bw", "cov", "isFw"):
            assert np.array_equal(pb[f], job["per_base"][f]), f
        # two map-range passes over one resident batch; back to one pass (which drops what the passes kept)
        resident = torch.frombuffer(bytearray(job["batches"][1]), dtype=torch.uint8).cuda()
        db.set_option("count_map_passes", 2)
        for rng in ((0, MAPS // 2), (MAPS // 2, MAPS)):
            db.set_option("count_map_range", rng)
            db.count_batch_dev(resident.data_ptr(), resident.numel())
        db.sync()
        db.set_option("count_map_range", (0, MAPS))
        db.set_option("count_map_passes", 1)
        assert H.entries_equal(db.export(), job["want_twice"])
        # clear and once more
        db.clear()
        count_all(db, job["batches"])
        assert H.entries_equal(db.export(), want)
    finally:
        db.close()


def test_window_moves_and_reallocates(kq, job):
    """an empty handle: a window, another of the same width (the same memory), a narrower one (a new table); the last one
    counts its own buckets only"""
    from kreeq_amd.dist import bucket_of

    want = job["want"]
    db = kq.KreeqDB(K, MAPS, capacity_hint=HINT)
    try:
        db.set_option("bucket_window", 0 | (128 << 16))
        slots = db.info()["slots_total"]
        db.set_option("bucket_window", 128 | (256 << 16))
        assert db.info()["slots_total"] == slots
        db.set_option("bucket_window", 0 | (64 << 16))
        count_all(db, job["batches"])
        wb = bucket_of(want["key"], K)
        mine = want[wb < 64]
        assert 0 < len(mine) < len(want)
        assert H.entries_equal(db.export(), mine)
    finally:
        db.close()
