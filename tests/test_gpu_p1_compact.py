"""The P1 scatter behind a map-range filter on narrow records (k <= 21, tables of >= 2048 regions): k_p1_scatter_c queues a
tile's survivors per wave ahead of the hash; KQ_OPT_KERNEL_SET bit 128 selects the previous kernel (k_p1_scatter_s), which hashes
and parks every k-mer.  Every case counts with both and compares the export entry for entry with the oracle's table restricted
to the maps of the range (key % 128): full and empty wave queues, filters that keep nearly all or nearly nothing, tile and
slice edges, three values of k, packed input with cached count matrices, the counters-only lookup, the other kernel-set bits."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

MASKS = (0, 128)                          # the shipped scatter, the previous one
TILE = 4032                               # k-mer starts per scanner tile


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


def _restrict(want, rng):
    m = want["key"] % np.uint64(128)
    return want[(m >= rng[0]) & (m < rng[1])]


def _oracle(O, k, batches):
    cpu = O.OracleDB(k, 128)
    for b in batches:
        cpu.count_batch(b, threads=8)
    return cpu.export()


def _handle(kq, k, rng, mask, hint=5_000_000, **opts):
    gpu = kq.KreeqDB(k, 128, capacity_hint=hint)
    gpu.set_option("count_path", "partitioned")
    gpu.set_option("trust_capacity", 1)
    for o, v in opts.items():
        gpu.set_option(o, v)
    if rng:
        gpu.set_option("count_map_range", rng)
    gpu.set_option("kernel_set", mask)
    return gpu


def _export(kq, k, batches, rng, mask, **opts):
    gpu = _handle(kq, k, rng, mask, **opts)
    for b in batches:
        gpu.count_batch(b)
    got = gpu.export()
    gpu.close()
    return got


def _random_batches(seed, n=2):
    return [H.synth_reads(6000 + 250 * i, 150, 300_000, seed=seed + i, err=0.006, n_rate=0.001)[0] for i in range(n)]


@pytest.fixture(scope="module")
def random_job(O):
    """two batches of random reads (223 and 232 tiles) and the oracle's table of them, shared by the cases that need no special input"""
    batches = _random_batches(600)
    return batches, _oracle(O, 21, batches)


def _edge_batch(k, seed=9):
    """random reads, reads shorter than k, runs of N and lower case, a random tail; the length is no multiple of the tile"""
    rng = np.random.default_rng(seed)
    b = H.synth_reads(5000, 149, 200_000, seed=seed, err=0.01, n_rate=0.003)[0]
    b += b"\n" + b"acgtnACGT" * 7 + b"\n" + b"A" * (k - 1) + b"\n" + b"ACGTAC\n" + b"N" * 300 + b"acgtacgtta" * 40 + b"NNNN" + b"\n"
    b += bytes(rng.choice(list(b"ACGTacgtN\n"), size=100_003).tolist())
    assert len(b) % TILE != 0
    return b


def test_full_queue_then_empty_queue(kq, O):
    """homopolymer reads a few tiles long between random reads: every k-mer of them has the canonical key 0 (map 0).  Range
    (0, 64) keeps all 1008 starts of a wave in the tiles inside such a read -- the queue is full to its last entry -- and range
    (64, 128) none of them: the dense phase runs no iteration and the round has no record.  Together the two tables are the
    unfiltered oracle's."""
    r = _random_batches(610)
    batches = [r[0] + b"\n" + b"A" * (3 * TILE + 100) + b"\n" + r[1][:200_000] + b"\n" + b"T" * (3 * TILE + 57) + b"\n" + r[1][200_000:],
               b"A" * (4 * TILE)]
    want = _oracle(O, 21, batches)
    assert want["key"][0] == 0
    for mask in MASKS:
        parts = []
        for rng in ((0, 64), (64, 128)):
            got = _export(kq, 21, batches, rng, mask)
            assert H.entries_equal(got, _restrict(want, rng)), (mask, rng)
            parts.append(got)
        both = np.concatenate(parts)
        assert H.entries_equal(both[np.argsort(both["key"], kind="stable")], want), mask


@pytest.mark.parametrize("rng", [(1, 128), (0, 127), (37, 38)])
def test_nearly_plain_filter_and_one_map(kq, random_job, rng):
    """(1, 128) and (0, 127): almost every start survives; (37, 38): a wave's queue holds a handful of entries, fewer than 64"""
    batches, want = random_job
    for mask in MASKS:
        assert H.entries_equal(_export(kq, 21, batches, rng, mask), _restrict(want, rng)), mask


@pytest.fixture(scope="module")
def edge_job(O):
    batches = [_edge_batch(21), H.synth_reads(20, 150, 5000, seed=77, err=0.01)[0]]       # the second: fewer than 4032 starts
    assert len(batches[1]) < TILE
    return batches, _oracle(O, 21, batches)


@pytest.mark.parametrize("rng", [(0, 64), (64, 128)])
def test_tile_and_slice_edges(kq, edge_job, rng):
    """a batch whose length is no multiple of 4032, reads shorter than k, runs of N and lower case, slices that cut inside a tile
    (four of them), and a batch of less than one tile"""
    batches, want = edge_job
    assert (len(batches[0]) - 20) // 250_001 >= 2                       # at least three slices
    for mask in MASKS:
        assert H.entries_equal(_export(kq, 21, batches, rng, mask, slice_kmers=250_001), _restrict(want, rng)), mask


@pytest.mark.parametrize("k", [11, 17, 21])
def test_k_values(kq, O, random_job, k):
    """the generic instantiation (k = 11, 17) and the constant one (21) on the same reads"""
    batches, want21 = random_job
    want = want21 if k == 21 else _oracle(O, k, batches)
    for mask in MASKS:
        assert H.entries_equal(_export(kq, k, batches, (32, 96), mask), _restrict(want, (32, 96))), mask


def test_packed_input_and_cached_count_matrices(kq, edge_job):
    """kq_count_packed_dev on the kq_pack_bases form of the edge batch gives the table of its ASCII run; with
    KQ_OPT_COUNT_MAP_PASSES = 2 over two resident batches the cached count matrix of the first range's scan drives the
    scatter's cursors in the second range (and, after the clear, in the first again)"""
    import torch

    from kreeq_amd import capi

    batches, want = edge_job
    dev = []
    for b in batches:
        codes, inv = capi.pack_bases(b)
        dev.append((torch.from_numpy(codes.view(np.int32).copy()).cuda(), torch.from_numpy(inv.view(np.int16).copy()).cuda(), len(b)))
    torch.cuda.synchronize()
    for mask in MASKS:
        ascii_run = _export(kq, 21, batches, (0, 64), mask, slice_kmers=250_001)
        gpu = _handle(kq, 21, None, mask, slice_kmers=250_001, count_map_passes=2)
        for cycle, rng in enumerate(((0, 64), (64, 128), (0, 64))):
            gpu.clear()
            gpu.set_option("count_map_range", rng)
            for dc, di, n in dev:
                gpu.count_packed_dev(dc.data_ptr(), di.data_ptr(), n)
            gpu.sync()
            got = gpu.export()
            assert H.entries_equal(got, _restrict(want, rng)), (mask, cycle)
            if cycle == 0:
                assert H.entries_equal(got, ascii_run), mask
        gpu.close()


def test_lookup_with_a_map_range(kq, O):
    """kq_lookup_sequence_dev with a map range and no per-base output takes the partitioned (counters-only) lookup for an
    assembly of this size on this table; its P1 is the filtered narrow scatter.  The three counters equal the oracle's."""
    import torch

    k, G = 21, 3_000_000
    reads, genome = H.synth_reads(12_000, 150, G, seed=700, err=0.005, n_rate=0.001)
    cpu = O.OracleDB(k, 128)
    cpu.count_batch(reads, threads=8)
    g = torch.frombuffer(bytearray(genome), dtype=torch.uint8).cuda()
    for mask in MASKS:
        gpu = _handle(kq, k, None, mask)
        gpu.count_batch(reads)
        assert G - k + 1 >= 1 << 20 and gpu.info()["slots_total"] * 16 <= 64 * (G - k + 1)      # the conditions of the automatic choice
        for path in ("auto", "partitioned"):
            gpu.set_option("lookup_path", path)
            for lo, hi in ((0, 64), (64, 128), (37, 38)):
                ctr = torch.zeros(3, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                gpu.lookup_sequence_dev(g.data_ptr(), len(genome), ctr.data_ptr(), map_lo=lo, map_hi=hi)
                gpu.sync()
                c_cpu, _ = cpu.validate_sequence(genome, map_lo=lo, map_hi=hi)
                assert ctr.cpu().numpy().astype(np.uint64).tolist() == c_cpu.tolist(), (mask, path, lo, hi)
        gpu.close()


def test_other_kernel_set_bits(kq, random_job):
    """bit 128 next to the bits of the last split level (64 = one workgroup per segment wherever it applies, 32 = never) on a
    table with a middle level; 8 stays unassigned, 256 is none"""
    batches, want = random_job
    for mask in (128 | 64, 128 | 32, 64, 32):
        got = _export(kq, 21, batches, (32, 96), mask, hint=100_000_000, narrow_mid=16)
        assert H.entries_equal(got, _restrict(want, (32, 96))), mask
    for bad in (8, 256):
        with pytest.raises(Exception):
            kq.KreeqDB(21, 128).set_option("kernel_set", bad)
