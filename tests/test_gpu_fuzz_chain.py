"""Differential fuzz of the calls that came after tests/test_gpu_fuzz.py: one seed of tests/fuzz_inputs.py goes through count,
kq_branch_scan, kq_search_variants, kq_subgraph_seed / _expand / _best_first / _trim, kq_subgraph_gfa, kq_export_map_images /
kq_import_map_image, the per-base lookup, kq_per_base_triples_dev, kq_format_table, kq_deflate_bgzf and the device inflate, on
ONE pair of handles that is carried from stage to stage.  Every comparison is exact, and what a stage is compared with never
comes from the device: the oracle's table, oracle/variants.py, tests/subgraph_ref.py, tests/gfa_ref.py, the host map writer,
tests/table_ref.py and zlib, all computed in tests/fuzz_inputs.py:expected from the seed alone (a later stage expects what the
restatement made of the restatement's earlier result).  tests/test_fuzz_inputs.py shows, without a GPU, that the seed list
reaches high-copy tables, key 0, repeated window keys, cycles, dropped edges and palindromes."""
import zlib

import numpy as np
import pytest

from tests import fuzz_inputs as F
from tests import helpers as H
from tests import subgraph_ref as R
from tests import table_ref as T
from tests.test_gpu_fastx import on_device

pytestmark = pytest.mark.gpu

GUARD = 0x5A


@pytest.fixture(scope="module")
def kq():
    from kreeq_amd import capi
    assert capi.device_available()
    return capi


def same_table(handle, table, k, what):
    assert H.entries_equal(handle.export(), R.entries_of(table)), what
    want = R.summary(table, k)
    want["missing"] %= 1 << 64                                           # (a 64-bit field: 4^32 of an empty table at k = 32 wraps)
    assert handle.summary() == want, what


def gfa_tuples(segs, edges):
    return ([(int(s["seq_off"]), int(s["head_key"]), int(s["n_kmers"]), int(s["cov"]), int(s["head_rc"])) for s in segs],
            [(int(e["from"]), int(e["to"]), int(e["count"]), int(e["from_rc"]), int(e["to_rc"])) for e in edges])


@pytest.mark.parametrize("seed", F.SEEDS)
def test_chain(kq, tmp_path, seed):
    import torch

    e = F.expected(seed)
    c, k = e.case, e.case.k
    at = "seed %d (k = %d, %s), stage %%s" % (seed, k, c.flavour)
    gpu = kq.KreeqDB(k, F.MAPS, capacity_hint=c.db_hint)
    sub = kq.KreeqDB(k, F.MAPS, capacity_hint=c.sub_hint)
    fresh = kq.KreeqDB(k, F.MAPS, capacity_hint=c.image_hint)
    try:
        # 1. count
        gpu.count_batch(c.reads)
        assert H.entries_equal(gpu.export(), e.entries), at % "1 count"

        # 2. branch scan
        for cutoff, want in e.flags.items():
            assert np.array_equal(gpu.branch_scan(c.asm, cutoff), want), at % ("2 branch scan, cutoff %d" % cutoff)

        # 3. variants
        gpu.set_option("variant_batch", c.var_batch)
        got = gpu.search_variants(c.asm, c.var_depth, c.var_span, c.var_cutoff)
        assert got == e.paths, at % ("3 variants (depth %d, span %d, cutoff %d, batch %d)" % (c.var_depth, c.var_span, c.var_cutoff, c.var_batch))
        rc, n_paths, n_seq, _, _ = gpu.search_variants_raw(c.asm, c.var_depth, c.var_span, c.var_cutoff)
        assert (rc, n_paths, n_seq) == (0, len(e.paths), sum(len(p[4]) for p in e.paths)), at % "3 variants, size query"
        gpu.set_option("variant_batch", 0)

        # 4. subgraph
        gpu.subgraph_seed(sub, c.asm, c.no_reference)
        same_table(sub, e.sub_seed, k, at % ("4 subgraph seed (no_reference %d)" % c.no_reference))
        if c.algorithm == "traversal":
            n_added = gpu.subgraph_expand(sub, c.sub_depth)
        else:
            n_added = gpu.subgraph_best_first(sub, c.sub_depth, c.search_cutoff)
        what = at % ("4 subgraph %s (depth %d, cutoff %d)" % (c.algorithm, c.sub_depth, c.search_cutoff))
        assert n_added == e.n_added, what
        same_table(sub, e.sub_grown, k, what)
        sub.subgraph_trim(c.trim_cutoff)
        same_table(sub, e.sub_trimmed, k, at % ("4 subgraph trim (cutoff %d)" % c.trim_cutoff))

        # 5. GFA
        for no_collapse in (False, True):
            want, what = e.gfa[no_collapse], at % ("5 GFA (no_collapse %d)" % no_collapse)
            segs, seq, edges, counts = sub.subgraph_gfa(no_collapse)
            assert counts == want.counts, what
            got_segs, got_edges = gfa_tuples(segs, edges)
            assert seq.decode() == want.seq, what
            assert got_segs == want.segs, what
            assert got_edges == want.edges, what

        # 6. map images
        want_images, want_hc = H.host_map_files(tmp_path, e.entries, F.MAPS, 0, F.MAPS)
        images, hc = gpu.export_map_images(0, F.MAPS)
        assert len(images) == F.MAPS, at % "6 map images"
        for m, (g, w) in enumerate(zip(images, want_images)):
            assert g.tobytes() == w, at % ("6 map images, map %d" % m)
        assert H.entries_equal(hc, want_hc[np.argsort(want_hc["key"], kind="stable")]), at % "6 map images, high-copy entries"
        n_in = n_tomb = 0
        for m, img in enumerate(images):
            n, t = fresh.import_map_image(m, img)
            n_in, n_tomb = n_in + n, n_tomb + t
        n_hot = int((e.entries["hc"] != 0).sum())
        assert (n_in, n_tomb) == (len(e.entries) - n_hot, n_hot), at % "6 map images, import"
        if n_hot:
            fresh.import_entries(hc)
        assert H.entries_equal(fresh.export(), e.entries), at % "6 map images, import"

        # 7. per-base table
        want_ctr, want_pb = e.lookup
        ctr, pb = gpu.lookup_sequence(c.asm, per_base=True)
        assert np.array_equal(ctr, want_ctr), at % "7 lookup"
        for f in ("fw", "bw", "cov", "isFw"):
            assert np.array_equal(pb[f], want_pb[f]), at % ("7 lookup, per-base " + f)
        d_asm = on_device(c.asm)
        d_ctr = torch.zeros(3, dtype=torch.int64, device="cuda")
        d_pb = torch.zeros(len(c.asm) * kq.DBGBASE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        total = len(e.triples)
        d_triples = torch.full((total * 3 + 16,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        gpu.lookup_sequence_dev(d_asm.data_ptr(), len(c.asm), d_ctr.data_ptr(), per_base_ptr=d_pb.data_ptr())
        gpu.per_base_triples_dev(d_pb.data_ptr(), e.segments, d_triples.data_ptr())
        gpu.sync()
        assert np.array_equal(d_ctr.cpu().numpy().view(np.uint64), want_ctr), at % "7 device lookup"
        triples = d_triples.cpu().numpy().view(np.uint32)
        assert np.array_equal(triples[:total * 3].reshape(-1, 3), e.triples), at % "7 triples"
        assert (triples[total * 3:] == 0xFFFFFFFF).all(), at % "7 triples, behind the end"
        piece_segs, names = T.pack_pieces(e.pieces)
        text = gpu.format_table(c.table_format, triples[:total * 3].reshape(-1, 3), piece_segs, names)
        assert text == e.text, at % ("7 table text (format %d)" % c.table_format)
        data = gpu.deflate_bgzf(text)
        assert len(data) <= kq.bgzf_bound(len(text)), at % "7 deflate, bound"
        blocks, used = kq.bgzf_scan(data)
        assert used == len(data), at % "7 deflate, block walk"
        members = [zlib.decompress(data[int(b["off"]):int(b["off"]) + int(b["size"])], 31) for b in blocks]
        assert b"".join(members) == e.text and all(members), at % "7 deflate, zlib"
        if data:
            comp = on_device(data)
            n = gpu.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, None, 0)
            assert n == len(e.text), at % "7 device inflate, size query"
            out = torch.full((n + 16,), GUARD, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert gpu.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, out.data_ptr(), n) == n, at % "7 device inflate"
            host = out.cpu().numpy()
            assert host[:n].tobytes() == e.text and (host[n:] == GUARD).all(), at % "7 device inflate"
        else:
            assert e.text == b"", at % "7 deflate"
    finally:
        for handle in (fresh, sub, gpu):
            handle.close()
