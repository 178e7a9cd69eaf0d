"""Tile, lane and alignment edges of the sequence scanner (kq_device.h: tile_fetch / tile_store / convert16 /
lane_scan_core) on every entry point that reads bases, exact against the CPU oracle on the same bytes.

The texts come from tests/scan_inputs.py (run ends at and across tile edges, the seam of a two-tile round and lane edges;
tests/test_scan_inputs.py holds them to their design), one per (k, lead): k at the values where the scanner's arithmetic
changes form, lead = the offset of the caller's pointer inside its 16-byte window.  The device copy of a text lies in a
torch tensor (aligned) behind 64 + lead bytes and in front of 64 more, all of them bases, so that a k-mer read past either
end of the text would count; the library gets the pointer to the text itself.  Table classes as in test_gpu_regions.py:
S (hint 0), B (hint 5 M)."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import scan_inputs as S

pytestmark = pytest.mark.gpu

MAP = S.MAP
HINT = {"S": 0, "B": 5_000_000}
REGION_SLOTS = 2048
SLACK = 64
ENTRY = 16                         # sizeof(kq_dbgbase)
GUARD = 64                         # entries
PATTERN = 0xA5
IDS = [f"k{k}-lead{lead}" for k, lead in S.CASES]
_SLACK_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(5).integers(0, 4, 2 * SLACK + 16)]


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


def n_regions_of(k, cls):
    """region count kq_create gives the class (as test_gpu_regions.n_regions_of)"""
    r = max(16, -(-int((HINT[cls] or 1 << 20) / 0.7) // REGION_SLOTS))
    return -(-r // 256) * 256 if r >= 2048 or k >= 29 else r


def handle(kq, k, cls, **opts):
    db = kq.KreeqDB(k, MAP, capacity_hint=HINT[cls])
    assert db.info()["slots_total"] == n_regions_of(k, cls) * REGION_SLOTS
    for o, v in opts.items():
        db.set_option(o, v)
    return db


def dev_text(text, lead):
    """-> (tensor, pointer): the text on the device at an address that is `lead` past a multiple of 16"""
    import torch

    buf = np.concatenate([_SLACK_BASES[:SLACK + lead], np.frombuffer(text, dtype=np.uint8), _SLACK_BASES[SLACK + lead:SLACK + lead + SLACK]])
    t = torch.from_numpy(buf.copy()).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + SLACK + lead


def same_records(keys, edges, ref, what):
    got = np.stack([keys.astype(np.uint64), edges.astype(np.uint64)], axis=1)
    exp = np.stack([ref.keys, ref.edges.astype(np.uint64)], axis=1)
    assert np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], exp[np.lexsort((exp[:, 1], exp[:, 0]))]), what


def unpack_records(recs, k):
    """packed 8-byte records (include/kreeq_amd.h: kq_emit_packed_dev) -> (key, reference edge byte), as
    test_gpu_parity._unpack_records"""
    from kreeq_amd.dist import key_of_hash

    recs = recs.astype(np.uint64)
    key = key_of_hash(recs << np.uint64(8), k)
    f = ((recs >> np.uint64(56)) & np.uint64(7)).astype(np.int64)
    b = ((recs >> np.uint64(59)) & np.uint64(7)).astype(np.int64)
    edge = np.where(f < 4, 1 << (7 - np.minimum(f, 3)), 0) | np.where(b < 4, 1 << (7 - (4 + np.minimum(b, 3))), 0)
    return key, edge.astype(np.uint8)


# ---------------------------------------------------------------------------------- emit
@pytest.mark.parametrize("k,lead", S.CASES, ids=IDS)
def test_emit(kq, k, lead):
    import torch

    ref = S.reference(k, lead)
    n = len(ref.text)
    t, ptr = dev_text(ref.text, lead)
    db = kq.KreeqDB(k, MAP)
    keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    edges = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    counts = db.emit_partitioned_dev(ptr, n, 1, keys.data_ptr(), edges.data_ptr(), n)
    assert int(counts[0]) == len(ref.keys)
    same_records(keys[:len(ref.keys)].cpu().numpy(), edges[:len(ref.keys)].cpu().numpy(), ref, "emit_partitioned_dev")
    if k <= 28:
        recs = torch.zeros(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        counts = db.emit_packed_dev(ptr, n, 1, recs.data_ptr(), n)
        assert int(counts[0]) == len(ref.keys)
        same_records(*unpack_records(recs[:len(ref.keys)].cpu().numpy(), k), ref, "emit_packed_dev")
    db.close()


# ---------------------------------------------------------------------------------- count
def same_table(db, ref, what):
    assert H.entries_equal(db.export(), ref.export), what
    assert db.summary(with_hist=True) == ref.summary, what


@pytest.mark.parametrize("k,lead", S.CASES, ids=IDS)
def test_count(kq, k, lead):
    ref = S.reference(k, lead)
    t, ptr = dev_text(ref.text, lead)
    for path, cls in (("direct", "S"), ("partitioned", "S"), ("partitioned", "B")):
        db = handle(kq, k, cls, count_path=path)
        db.count_batch_dev(ptr, len(ref.text))
        same_table(db, ref, (path, cls))
        assert db.info()["slots_total"] == n_regions_of(k, cls) * REGION_SLOTS
        db.close()
    maps = ref.export["key"] % np.uint64(MAP)
    for lo, hi in ((0, 64), (64, 128)):                    # the filtered scatter, one tile per round
        db = handle(kq, k, "B", count_path="partitioned", count_map_range=(lo, hi))
        db.count_batch_dev(ptr, len(ref.text))
        assert H.entries_equal(db.export(), ref.export[(maps >= lo) & (maps < hi)]), (lo, hi)
        db.close()


SLICED = [(k, lead) for k in (21, 31) for lead in (1, 8, 15)]


@functools.lru_cache(maxsize=None)
def sliced_reference(k, lead):
    from oracle import oracle as O

    text = b"\n".join([S.reference(k, lead).text] * 8)      # ~290 KB; the copies sit at other window offsets
    cpu = O.OracleDB(k, MAP)
    cpu.count_batch(text, threads=4)
    want = cpu.export()
    cpu.close()
    return text, want


@pytest.mark.parametrize("k,lead", SLICED, ids=[f"k{k}-lead{lead}" for k, lead in SLICED])
def test_sliced_count(kq, k, lead):
    """KQ_OPT_SLICE_KMERS with a caller lead: a slice starts one base before its first k-mer (at any offset of the window)
    and masks the starts outside its range (EmitRange)"""
    text, want = sliced_reference(k, lead)
    t, ptr = dev_text(text, lead)
    for path, slice_kmers in (("direct", 1000), ("direct", 123457), ("partitioned", 123457)):   # of test_sliced_resident_batch
        db = kq.KreeqDB(k, MAP)
        db.set_option("count_path", path)
        db.set_option("slice_kmers", slice_kmers)
        db.count_batch_dev(ptr, len(text))
        assert H.entries_equal(db.export(), want), (path, slice_kmers)
        db.close()


# ---------------------------------------------------------------------------------- packed input, device packer
@pytest.mark.parametrize("k,lead", S.CASES, ids=IDS)
def test_packed_input(kq, k, lead):
    """the packed form has no lead, the run ends lie on the same tile and lane edges when lead = 0 and 16 - lead off them
    otherwise"""
    import torch

    from kreeq_amd import capi

    ref = S.reference(k, lead)
    t, ptr = dev_text(ref.text, lead)
    codes, inv = capi.pack_bases(ref.text)
    dc = torch.from_numpy(codes.view(np.int32).copy()).cuda()
    di = torch.from_numpy(inv.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    for path in ("direct", "partitioned"):
        db = handle(kq, k, "S", count_path=path)
        db.count_packed_dev(dc.data_ptr(), di.data_ptr(), len(ref.text))
        same_table(db, ref, path)
        asc = handle(kq, k, "S", count_path=path)
        asc.count_batch_dev(ptr, len(ref.text))
        assert H.entries_equal(db.export(), asc.export()) and db.summary(with_hist=True) == asc.summary(with_hist=True)
        db.close(), asc.close()


@pytest.mark.parametrize("k,lead", S.CASES, ids=IDS)
def test_device_packer(kq, k, lead):
    import torch

    from kreeq_amd import capi

    ref = S.reference(k, lead)
    t, ptr = dev_text(ref.text, lead)
    codes, inv = capi.pack_bases(ref.text)
    units = len(codes)
    assert units == (len(ref.text) + 15) // 16
    dc = torch.full(((units + 16) * 4,), PATTERN, dtype=torch.uint8, device="cuda")       # 8 units of guard on each side
    di = torch.full(((units + 16) * 2,), PATTERN, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    db = kq.KreeqDB(k, MAP)
    db.pack_bases_dev(ptr, len(ref.text), dc.data_ptr() + 32, di.data_ptr() + 16)
    db.sync()
    hc, hi = dc.cpu().numpy(), di.cpu().numpy()
    assert np.array_equal(hc[32:32 + 4 * units].view(np.uint32), codes) and np.array_equal(hi[16:16 + 2 * units].view(np.uint16), inv)
    for host, a, b in ((hc, 32, 32 + 4 * units), (hi, 16, 16 + 2 * units)):
        assert (host[:a] == PATTERN).all() and (host[b:] == PATTERN).all()
    db.close()


# ---------------------------------------------------------------------------------- lookup
def table_of(kq, ref):
    db = kq.KreeqDB(ref.k, MAP)
    db.count_batch(ref.reads)
    assert H.entries_equal(db.export(), ref.table)
    return db


@pytest.mark.parametrize("k,lead", S.CASES, ids=IDS)
def test_lookup_counters(kq, k, lead):
    import torch

    ref = S.reference(k, lead)
    t, ptr = dev_text(ref.text, lead)
    db = table_of(kq, ref)
    for path in ("direct", "partitioned"):
        db.set_option("lookup_path", path)
        for lo, hi in S.RANGES:
            for cut in S.CUTOFFS:
                ctr = torch.zeros(3, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                db.lookup_sequence_dev(ptr, len(ref.text), ctr.data_ptr(), cov_cutoff=cut, map_lo=lo, map_hi=hi)
                db.sync()
                assert ctr.cpu().numpy().astype(np.uint64).tolist() == ref.validate[(lo, hi, cut)][0].tolist(), (path, lo, hi, cut)
    db.close()


class PerBase:
    """n zeroed kq_dbgbase on the device, `shift` bytes past an aligned address, between two bands of GUARD entries (and the
    shift's remainder) filled with a byte pattern"""

    def __init__(self, n, shift):
        import torch

        self.n, self.start = n, GUARD * ENTRY + shift
        self.raw = torch.full(((n + 2 * GUARD + 4) * ENTRY,), PATTERN, dtype=torch.uint8, device="cuda")
        self.raw[self.start:self.start + n * ENTRY] = 0
        torch.cuda.synchronize()
        assert self.raw.data_ptr() % 16 == 0
        self.ptr = self.raw.data_ptr() + self.start

    def read(self):
        from kreeq_amd import capi

        host = self.raw.cpu().numpy()
        end = self.start + self.n * ENTRY
        assert (host[:self.start] == PATTERN).all(), "the guard band in front was written"
        assert (host[end:] == PATTERN).all() and len(host) - end >= GUARD * ENTRY, "the guard band behind was written"
        return host[self.start:end].copy().view(capi.DBGBASE_DTYPE)


def same_per_base(got, want, what):
    for f in ("fw", "bw", "cov", "isFw"):
        assert np.array_equal(got[f], want[f]), (what, f, np.flatnonzero(got[f] != want[f])[:8].tolist())
    assert not got["pad"].any(), what
    idle = (want["fw"] == 0) & (want["bw"] == 0) & (want["cov"] == 0) & (want["isFw"] == 0)
    assert idle.any() and not got[idle].view(np.uint8).any(), what          # what the oracle left alone is still all zero


# bytes the per-base pointer is shifted by: none; 4 (the alignment of kq_dbgbase, with the bases pointer at `lead`); whole entries
PER_BASE_SHIFTS = (0, 4, 3 * ENTRY)


@pytest.mark.parametrize("k,lead", S.CASES, ids=IDS)
def test_lookup_per_base(kq, k, lead):
    import torch

    ref = S.reference(k, lead)
    n = len(ref.text)
    t, ptr = dev_text(ref.text, lead)
    db = table_of(kq, ref)

    def lookup(pb, lo, hi, cut):
        ctr = torch.zeros(3, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        db.lookup_sequence_dev(ptr, n, ctr.data_ptr(), cov_cutoff=cut, map_lo=lo, map_hi=hi, per_base_ptr=pb.ptr)
        db.sync()
        return ctr.cpu().numpy().astype(np.uint64)

    for shift in PER_BASE_SHIFTS:
        for cut in S.CUTOFFS:
            want_c, want_pb = ref.validate[(0, MAP, cut)]
            full = PerBase(n, shift)
            assert lookup(full, 0, MAP, cut).tolist() == want_c.tolist(), (shift, cut)
            same_per_base(full.read(), want_pb, (shift, cut, "full range"))
            halves = PerBase(n, shift)                      # the two half ranges accumulate into one array
            c_lo = lookup(halves, 0, 64, cut)
            assert c_lo.tolist() == ref.validate[(0, 64, cut)][0].tolist()
            same_per_base(halves.read(), ref.validate[(0, 64, cut)][1], (shift, cut, "lower half"))
            c_hi = lookup(halves, 64, MAP, cut)
            assert c_hi.tolist() == ref.validate[(64, MAP, cut)][0].tolist() and (c_lo + c_hi).tolist() == want_c.tolist()
            same_per_base(halves.read(), want_pb, (shift, cut, "both halves"))
    one = PerBase(n, 0)                                     # the upper half alone
    lookup(one, 64, MAP, 0)
    got, want = one.read(), ref.validate[(64, MAP, 0)][1]
    for f in ("fw", "bw", "cov", "isFw"):
        assert np.array_equal(got[f], want[f]), f
    db.close()


# ---------------------------------------------------------------------------------- branch scan
@pytest.mark.parametrize("k,lead", S.BRANCH_CASES, ids=[f"k{k}-lead{lead}" for k, lead in S.BRANCH_CASES])
def test_branch_scan_cutoffs(kq, k, lead):
    """the host entry stages the text at an aligned address: the text of lead 0 has its run ends on the tile and lane edges,
    the others 1, 8 and 15 bytes in front of them"""
    ref = S.reference(k, lead)
    db = table_of(kq, ref)
    for cut in S.BRANCH_CUTOFFS:
        got = db.branch_scan(ref.text, cov_cutoff=cut)
        want = H.branch_flags(ref.table, k, ref.text, cut)
        assert np.array_equal(got, want), (cut, np.flatnonzero(got != want)[:8].tolist())
    db.close()
