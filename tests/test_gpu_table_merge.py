"""kq_per_base_merge_dev (k_tab_merge, kreeq_amd/csrc/kq_table.h) against numpy: a stored entry (any of its 16 bytes non-zero)
overwrites its oriented triple and is zeroed, a zero entry leaves the triple alone, nothing between the segments is touched;
segment lengths around the wave and the workgroup, 10^5 one-position segments, odd entry indices, more positions than one grid
pass; and end to end on the device: the triples accumulated over map ranges equal kq_per_base_triples_dev after one lookup
over every map, with the three counters adding up."""
import ctypes as C

import numpy as np
import pytest

from kreeq_amd import KreeqDB, capi, synth
from tests import table_ref as T

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
GUARD = 16                                # triples (u32) behind the last one that no call may touch


@pytest.fixture(scope="module")
def db():
    return KreeqDB(21, 128, device=0, capacity_hint=1024)


def random_entries(rng, n, zero_share=0.5):
    pb = np.zeros(n, dtype=capi.DBGBASE_DTYPE)
    pb["fw"], pb["bw"], pb["cov"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64), rng.integers(0, 1000, n), rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    pb["isFw"] = rng.integers(0, 2, n)
    pb[rng.random(n) < zero_share] = np.zeros(1, dtype=capi.DBGBASE_DTYPE)[0]
    return pb


def listed_mask(n, segments):
    m = np.zeros(n, dtype=bool)
    for s, l in segments:
        m[s:s + l] = True
    return m


def merge_on_device(db, pb, segments, prior):
    """-> (triples with their guard, per-base entries) after one kq_per_base_merge_dev"""
    import torch

    d_pb = torch.from_numpy(pb.view(np.uint8).copy()).cuda()
    d_t = torch.from_numpy(prior.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    db.per_base_merge_dev(d_pb.data_ptr(), segments, d_t.data_ptr())
    db.sync()
    return d_t.cpu().numpy().view(np.uint32), d_pb.cpu().numpy().view(capi.DBGBASE_DTYPE)


def check_merge(db, pb, segments, seed):
    """random prior triples; the listed stored entries arrive and are cleared, everything else stays"""
    rng = np.random.default_rng(seed)
    total = sum(l for _, l in segments)
    prior = rng.integers(0, 2 ** 32, total * 3 + GUARD, dtype=np.uint64).astype(np.uint32)
    got_t, got_pb = merge_on_device(db, pb, segments, prior)
    stored = np.concatenate([pb[s:s + l].view(np.uint8).reshape(-1, 16).any(axis=1) for s, l in segments]) if segments else np.zeros(0, dtype=bool)
    want_t = np.where(stored[:, None], T.triples_of(pb, segments), prior[:total * 3].reshape(-1, 3))
    assert np.array_equal(got_t[:total * 3].reshape(-1, 3), want_t)
    assert np.array_equal(got_t[total * 3:], prior[total * 3:])                       # the guard
    listed = listed_mask(len(pb), segments)
    assert not got_pb[listed].view(np.uint8).any()                                    # consumed: zero over the segments again
    assert np.array_equal(got_pb[~listed].view(np.uint8), pb[~listed].view(np.uint8))     # between the segments: as it was
    return stored


def test_random_entries(db):
    rng = np.random.default_rng(21)
    pb = random_entries(rng, 5000)
    segments = [(0, 1), (2, 255), (258, 257), (600, 0), (601, 1024), (1700, 3299), (4999, 1)]
    pb[~listed_mask(len(pb), segments)] = random_entries(rng, len(pb), 0.0)[~listed_mask(len(pb), segments)]      # random bytes between the segments
    stored = check_merge(db, pb, segments, 1)
    assert 0.3 < stored.mean() < 0.7                                                  # about half the entries are zero ...
    assert {0, 1} <= set(pb["isFw"][listed_mask(len(pb), segments) & (pb["cov"] != 0)].tolist())      # ... and both orientations arrive


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257))
def test_one_segment(db, n):
    rng = np.random.default_rng(n)
    for start in (0, 3):                                                              # an even and an odd entry index
        pb = random_entries(rng, start + n + 5)
        pb[:start] = random_entries(rng, start, 0.0)
        pb[start + n:] = random_entries(rng, 5, 0.0)
        check_merge(db, pb, [(start, n)], 100 + n)


def test_many_one_position_segments(db):
    rng = np.random.default_rng(5)
    n = 100_000
    pb = random_entries(rng, 2 * n + 1)
    pb[0::2] = random_entries(rng, n + 1, 0.0)                                         # a separator before, between and behind them
    check_merge(db, pb, [(2 * i + 1, 1) for i in range(n)], 6)


def test_more_than_one_grid_pass(db):
    """3 x 10^6 positions: 11 719 workgroups of work for a grid of at most 8 per CU"""
    rng = np.random.default_rng(7)
    n = 1_000_000
    pb = random_entries(rng, 3 * n + 11)
    segments = [(1, n), (n + 4, n), (2 * n + 9, n)]
    check_merge(db, pb, segments, 8)


def test_consume_and_clear(db):
    """an entry whose only non-zero byte is isFw (or a pad byte) is stored: the triple (0, 0, 0) replaces the prior one and the
    entry is cleared; the all-zero entry next to it keeps its prior triple"""
    pb = np.zeros(6, dtype=capi.DBGBASE_DTYPE)
    pb["isFw"][1] = 1
    pb["pad"][3, 2] = 9
    pb["fw"][4] = 7                                                                    # (isFw = 0: fw lands in the third column)
    prior = np.arange(100, 100 + 6 * 3 + GUARD, dtype=np.uint32)
    got_t, got_pb = merge_on_device(db, pb, [(0, 6)], prior)
    want = prior.copy()
    want[3:6] = 0
    want[9:12] = 0
    want[12:15] = (0, 0, 7)
    assert np.array_equal(got_t, want)
    assert not got_pb.view(np.uint8).any()


# ---- end to end: map ranges on the device ------------------------------------------------------------------------------------

def base_runs(text):
    """[(start, len)] of the maximal ACGT runs of an ascii array"""
    is_base = np.isin(text, np.frombuffer(b"ACGTacgt", dtype=np.uint8))
    edges = np.flatnonzero(np.diff(np.concatenate([[0], is_base.astype(np.int8), [0]])))
    return [(int(a), int(b - a)) for a, b in zip(edges[0::2], edges[1::2])]


@pytest.fixture(scope="module")
def assembly():
    """reads at 8x of a 2 x 10^5 genome, and an assembly of it with errors and N runs (one at the very start), as lookup text"""
    G = 200_000
    g = synth.genome_codes(G, seed=31)
    reads = synth.reads_batch(g, 8 * G // 150, 150, seed=32, err=0.005).tobytes()
    asm = synth.codes_to_ascii(synth.mutate(g, 0.002, seed=33)).copy()
    rng = np.random.default_rng(34)
    asm[:3] = ord("N")
    for at in rng.integers(10, G - 50, 40):
        asm[at:at + int(rng.integers(1, 30))] = ord("N")
    text = np.concatenate([asm, np.frombuffer(b"\n", dtype=np.uint8)])
    segments = base_runs(text)
    assert len(segments) > 30 and segments[0][0] == 3
    return reads, text, segments


@pytest.mark.parametrize("k,map_count,ranges", [(21, 128, ((0, 43), (43, 86), (86, 128))), (31, 128, ((0, 43), (43, 86), (86, 128))),
                                               (21, 100, ((0, 33), (33, 67), (67, 100)))])
def test_map_ranges_accumulate(assembly, k, map_count, ranges):
    import torch

    reads, text, segments = assembly
    total = sum(l for _, l in segments)
    h = KreeqDB(k, map_count, device=0, capacity_hint=2_000_000)
    h.count_batch(reads)
    d_text = torch.from_numpy(text).cuda()
    # one lookup over every map, then kq_per_base_triples_dev
    d_pb = torch.zeros(len(text) * 16, dtype=torch.uint8, device="cuda")
    d_ctr = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_want = torch.zeros(total * 3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    h.lookup_sequence_dev(d_text.data_ptr(), len(text), d_ctr.data_ptr(), per_base_ptr=d_pb.data_ptr())
    h.per_base_triples_dev(d_pb.data_ptr(), segments, d_want.data_ptr())
    h.sync()
    want, want_ctr = d_want.cpu().numpy(), d_ctr.cpu().numpy()
    assert (want.reshape(-1, 3)[:, 0] != 0).mean() > 0.8 and want_ctr[1] > 0 and want_ctr[0] > 0      # most k-mers are found, some are missing
    # range by range into one per-base array that is zeroed once
    d_pb.zero_()
    d_acc = torch.zeros(total * 3, dtype=torch.int32, device="cuda")
    d_sum = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for lo, hi in ranges:
        h.lookup_sequence_dev(d_text.data_ptr(), len(text), d_sum.data_ptr(), map_lo=lo, map_hi=hi, per_base_ptr=d_pb.data_ptr())
        h.per_base_merge_dev(d_pb.data_ptr(), segments, d_acc.data_ptr())
        h.sync()
        assert not bool(d_pb.any())                                                    # consumed: ready for the next range
        assert not np.array_equal(d_acc.cpu().numpy(), want) or (lo, hi) == ranges[-1]      # every range has its share
    assert np.array_equal(d_acc.cpu().numpy(), want)
    assert d_sum.cpu().numpy().tolist() == want_ctr.tolist()
    h.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals(db):
    import torch

    pb = random_entries(np.random.default_rng(3), 64, 0.0)
    d_pb = torch.from_numpy(pb.view(np.uint8).copy()).cuda()
    d_t = torch.full((64 * 3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    f = capi.load().kq_per_base_merge_dev

    def rc_of(segments, handle=db._h, per_base=d_pb.data_ptr(), triples=d_t.data_ptr(), lists=True):
        start = np.array([s for s, _ in segments], dtype=np.uint64)
        length = np.array([n for _, n in segments], dtype=np.uint64)
        sp, lp = (start.ctypes.data_as(C.c_void_p), length.ctypes.data_as(C.c_void_p)) if lists else (None, None)
        return f(handle, C.c_void_p(per_base) if per_base else None, sp, lp, len(segments), C.c_void_p(triples) if triples else None)

    good = [(0, 10), (10, 5), (20, 0), (20, 3)]                                        # touching and empty segments are in order
    assert rc_of(good, handle=None) == ERR_INVALID                                    # null pointers
    assert rc_of(good, per_base=None) == ERR_INVALID
    assert rc_of(good, triples=None) == ERR_INVALID
    assert rc_of(good, lists=False) == ERR_INVALID
    assert rc_of([(0, 10), (5, 10)]) == ERR_INVALID                                   # overlapping
    assert "segment 1" in capi.load().kq_last_error().decode()
    assert rc_of([(0, 10), (9, 1)]) == ERR_INVALID
    assert rc_of([(20, 5), (0, 5)]) == ERR_INVALID                                    # descending
    assert rc_of([(0, 5), (2 ** 64 - 4, 8)]) == ERR_INVALID                           # start + length leaves 64 bits
    assert rc_of([], lists=False) == 0                                                # n_segs = 0
    assert rc_of([(3, 0), (7, 0)]) == 0                                               # only empty ones: no device work
    db.sync()
    assert np.array_equal(d_pb.cpu().numpy(), pb.view(np.uint8)) and bool((d_t == 0x5A5A5A5A).all())      # nothing was touched
    assert rc_of(good) == 0
    db.sync()
    assert not d_pb.cpu().numpy().view(capi.DBGBASE_DTYPE)[listed_mask(64, good)].view(np.uint8).any()
