"""<db>/.map.<m>.bin images built and parsed on the GPU (kq_export_map_images / kq_import_map_image).  The reference for
every byte is the host writer (kreeq_amd/host/kreeq_db.cpp through hostdb.write_maps) fed with kq_export's entries, or the
reference project's own fixture files; the device code is never its own reference."""
import os
import struct

import numpy as np
import pytest

from kreeq_amd import capi, hostdb
from tests import helpers as H
from tests.test_host_db import DBS, findable, mix

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -6
EMPTY_MAP = struct.pack("<Q", 256) + struct.pack("<QQQ", 0xFFFFFFFFFFFFFFF5, 0, 0) * 256        # 6152 bytes
M64 = (1 << 64) - 1


def submap_of(key):
    h = mix(int(key))
    return ((h >> 8) ^ (h >> 16) ^ (h >> 24)) & 255


def np_submap(keys):
    """submap of every key (u64 array): the 64 x 64 -> 128 bit product from 32-bit halves, high + low word"""
    a = keys.astype(np.uint64)
    m_lo, m_hi, lo32 = np.uint64(0xde5fb9d2630458e9 & 0xFFFFFFFF), np.uint64(0xde5fb9d2630458e9 >> 32), np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    a_lo, a_hi = a & lo32, a >> s32
    ll, lh, hl, hh = a_lo * m_lo, a_lo * m_hi, a_hi * m_lo, a_hi * m_hi
    mid = (ll >> s32) + (lh & lo32) + (hl & lo32)
    hi = hh + (lh >> s32) + (hl >> s32) + (mid >> s32)
    h = hi + a * np.uint64(0xde5fb9d2630458e9)
    return ((h >> np.uint64(8)) ^ (h >> np.uint64(16)) ^ (h >> np.uint64(24))) & np.uint64(255)


host_files = H.host_map_files


def check_range(db, tmp, lo, hi, entries=None):
    """images of [lo, hi) == the host writer's files; the size query agrees with the filled call.  -> (images, hc)"""
    entries = db.export() if entries is None else entries
    want, want_hc = host_files(tmp, entries, db.map_count, lo, hi)
    offsets, n_hc = db.export_map_images(lo, hi, sizes_only=True)
    got, hc = db.export_map_images(lo, hi)
    assert len(got) == hi - lo == len(offsets) - 1
    assert [len(g) for g in got] == np.diff(offsets.astype(np.int64)).tolist() and offsets[0] == 0
    for m, (g, w) in enumerate(zip(got, want), lo):
        assert g.tobytes() == w, f"map {m}"
    assert n_hc == len(hc) == len(want_hc)
    assert H.entries_equal(hc, want_hc[np.argsort(want_hc["key"], kind="stable")])
    return got, hc


def random_entries(keys, seed, max_cov=254):
    rng = np.random.default_rng(seed)
    e = np.zeros(len(keys), dtype=capi.ENTRY_DTYPE)
    e["key"] = keys
    e["cov"] = rng.integers(1, max_cov + 1, len(keys))
    for f in ("fw", "bw"):
        e[f] = (rng.random((len(keys), 4)) * (e["cov"][:, None] + 1)).astype(np.uint32) * (rng.random((len(keys), 4)) < 0.6)
    return e[np.argsort(e["key"], kind="stable")]


# ---- writer == host writer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DBS)
def test_golden_database_images(golden_dbs, tmp_path, name):
    src = os.path.join(golden_dbs, name + ".kreeq")
    entries, k, mc = hostdb.read_db(src)
    assert mc == 128
    db = capi.KreeqDB(k, mc)
    db.import_entries(entries)
    exported = db.export()
    assert H.entries_equal(exported, entries)
    got, _ = check_range(db, tmp_path, 0, 128, exported)
    for m, g in enumerate(got):
        assert len(g) == os.path.getsize(os.path.join(src, f".map.{m}.bin")), m      # the reference's own capacity choices
        p = str(tmp_path / f"img.{m}.bin")
        g.tofile(p)
        findable(p, 9)
    for lo, hi in ((0, 1), (5, 9), (127, 128)):
        sub, _ = check_range(db, tmp_path, lo, hi, exported)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(sub, got[lo:hi]))


# ---- edges of the build kernel -----------------------------------------------------------------------------------------
EDGE_MAP, BIG_SUBMAP, BIG_N = 5, 200, 3000
EDGE_SIZES = {1: 1, 2: 2, 3: 3, 4: 4, 5: 7, 6: 8, 7: 14, 8: 15, 9: 28, 10: 29, 11: 56, 12: 57, 13: 113}      # submap -> entries


@pytest.fixture(scope="module")
def edge_entries():
    """k = 21, map 5 only: submaps 1..13 with both sides of every capacity step from 1 to 127, submap 200 with 3 000"""
    rng = np.random.default_rng(2024)
    want = dict(EDGE_SIZES)
    want[BIG_SUBMAP] = BIG_N
    picked = {s: [] for s in want}
    while any(len(picked[s]) < n for s, n in want.items()):
        keys = rng.integers(0, (1 << 42) // 128, 1 << 20, dtype=np.uint64) * np.uint64(128) + np.uint64(EDGE_MAP)
        keys = np.unique(keys[H.canonical_keys_of(keys, 21) == keys])
        sub = np_submap(keys)
        for s, n in want.items():
            have = set(picked[s])
            picked[s] += [int(x) for x in keys[sub == s].tolist() if int(x) not in have][:n - len(picked[s])]
    keys = np.array(sorted(x for s in want for x in picked[s]), dtype=np.uint64)
    return random_entries(keys, 7)


@pytest.fixture(scope="module")
def edge_db(edge_entries):
    db = capi.KreeqDB(21, 128)
    db.import_entries(edge_entries)
    return db


def test_edge_table_is_what_was_intended(edge_entries):
    sizes = {}
    for key in edge_entries["key"].tolist():
        assert key % 128 == EDGE_MAP
        sizes[submap_of(key)] = sizes.get(submap_of(key), 0) + 1
    assert sizes == {**EDGE_SIZES, BIG_SUBMAP: BIG_N}


def test_build_kernel_edges(edge_db, edge_entries, tmp_path):
    assert H.entries_equal(edge_db.export(), edge_entries)
    got, hc = check_range(edge_db, tmp_path, EDGE_MAP - 1, EDGE_MAP + 2, edge_entries)
    assert got[0].tobytes() == EMPTY_MAP == got[2].tobytes() and len(EMPTY_MAP) == 6152      # the neighbours hold nothing
    assert len(hc) == 0
    # the submap sizes and capacities as the image states them
    img, off, caps = got[1].tobytes(), 8, {}
    for s in range(256):
        ver, size, cap = struct.unpack_from("<QQQ", img, off)
        off += 24 + ((cap + 17) + cap * 24 + 8 if size else 0)
        if size:
            caps[s] = (size, cap)
    assert off == len(img)
    assert caps == {s: (n, c) for (s, n), c in zip(sorted(EDGE_SIZES.items()), (1, 3, 3, 7, 7, 15, 15, 31, 31, 63, 63, 127, 255))} | {BIG_SUBMAP: (BIG_N, 4095)}
    p = str(tmp_path / "edge.bin")
    got[1].tofile(p)
    assert findable(p, 9) == len(edge_entries)
    check_range(edge_db, tmp_path, 0, 128, edge_entries)


def test_bad_ranges_and_capacity(edge_db):
    L = capi.load()
    off = np.zeros(130, dtype=np.uint64)
    n_hc = capi.C.c_uint64(0)
    p_off = off.ctypes.data_as(capi.C.c_void_p)
    assert L.kq_export_map_images(edge_db.handle, 0, 129, None, 0, p_off, None, 0, capi.C.byref(n_hc)) == INVALID
    assert L.kq_export_map_images(edge_db.handle, 6, 5, None, 0, p_off, None, 0, capi.C.byref(n_hc)) == INVALID
    assert L.kq_export_map_images(edge_db.handle, 5, 5, None, 0, p_off, None, 0, capi.C.byref(n_hc)) == 0 and off[0] == 0


# ---- key order is unsigned ---------------------------------------------------------------------------------------------
def test_k32_keys_on_both_sides_of_2_63(tmp_path):
    rng = np.random.default_rng(32)
    keys = np.concatenate([rng.integers(0, 1 << 62, 1 << 17, dtype=np.uint64), rng.integers(1 << 63, M64, 1 << 17, dtype=np.uint64, endpoint=True)])
    keys = np.unique(keys[H.canonical_keys_of(keys, 32) == keys])
    keys = keys[keys % np.uint64(128) == 4]          # (a map whose keys end in A: a key above 2^63 can be the canonical strand)
    sub = np_submap(keys)
    s_best = int(np.argmax(np.bincount(sub.astype(np.int64), minlength=256)))
    keys = keys[sub == s_best]
    assert (keys < np.uint64(1 << 63)).sum() >= 2 and (keys >= np.uint64(1 << 63)).sum() >= 2 and len(keys) >= 5
    entries = random_entries(keys, 5)
    db = capi.KreeqDB(32, 128)
    db.import_entries(entries)
    check_range(db, tmp_path, 0, 128, entries)


def test_k2_whole_key_space(tmp_path):
    keys = np.array(H.all_canonical_keys(2), dtype=np.uint64)
    entries = random_entries(keys, 6)
    db = capi.KreeqDB(2, 128)
    db.import_entries(entries)
    check_range(db, tmp_path, 0, 128, entries)


# ---- high-copy ---------------------------------------------------------------------------------------------------------
def test_high_copy_tombstones_and_capacity_errors(tmp_path):
    k = 21
    _, hot = H.hot_kmer_reads(k, 11)
    reads, _ = H.synth_reads(300, 100, 5000, 3)
    db = capi.KreeqDB(k, 128)
    db.count_batch(b"\n".join(hot) + b"\n" + reads)
    entries = db.export()
    hc_want = entries[entries["hc"] != 0]
    assert len(hc_want) >= 1
    got, hc = check_range(db, tmp_path, 0, 128, entries)
    assert H.entries_equal(hc, hc_want)
    for e in hc_want:                                       # the slot of a high-copy k-mer: key, no edges, cov 255, zero padding
        img = got[int(e["key"]) % 128].tobytes()
        assert struct.pack("<Q", int(e["key"])) + b"\0" * 8 + b"\xff" + b"\0" * 7 in img
    # capacity errors report the sizes
    L, C = capi.load(), capi.C
    offsets, n_hc = db.export_map_images(0, 128, sizes_only=True)
    total = int(offsets[-1])
    buf, hcb = np.zeros(total, dtype=np.uint8), np.zeros(n_hc, dtype=capi.ENTRY_DTYPE)
    for cap, hc_cap in ((total - 1, n_hc), (total, n_hc - 1)):
        off2, n2 = np.zeros_like(offsets), C.c_uint64(0)
        rc = L.kq_export_map_images(db.handle, 0, 128, buf.ctypes.data_as(C.c_void_p), cap, off2.ctypes.data_as(C.c_void_p),
                                    hcb.ctypes.data_as(C.c_void_p), hc_cap, C.byref(n2))
        assert rc == CAPACITY and np.array_equal(off2, offsets) and n2.value == n_hc


# ---- windowed handle, pending records -----------------------------------------------------------------------------------
def test_windowed_handles_export_their_window(tmp_path):
    batch, _ = H.synth_reads(400, 120, 20000, 21)
    whole = capi.KreeqDB(21, 128, capacity_hint=1 << 20)
    whole.count_batch(batch)
    want = whole.export()
    parts = []
    for lo, hi in ((0, 100), (100, 256)):
        w = capi.KreeqDB(21, 128, capacity_hint=1 << 20)
        w.set_option("shard_window", lo | (hi << 16))
        w.count_batch(batch)
        ent = w.export()
        assert 0 < len(ent) < len(want)
        check_range(w, tmp_path, 0, 128, ent)
        check_range(w, tmp_path, 40, 50, ent)
        parts.append(ent)
    both = np.concatenate(parts)
    assert H.entries_equal(both[np.argsort(both["key"], kind="stable")], want)


def test_pending_records_are_flushed():
    """two batches left pending (KQ_OPT_PENDING_BYTES): the call applies them itself -- in ONE table pass, so both were
    still pending when it began -- and gives the images of the synchronised table"""
    batches = [H.synth_reads(6000, 150, 300_000, seed)[0] for seed in (22, 23)]
    out = []
    for synced in (False, True):
        db = capi.KreeqDB(21, 128, capacity_hint=5_000_000)
        db.set_option("count_path", "partitioned")
        db.set_option("trust_capacity", 1)          # no state read (which applies what is pending) between the batches
        db.set_option("pending_bytes", (64 << 20) if not synced else 0)      # room for both record sets (4 MB each) / none
        for b in batches:
            db.count_batch(b)
        if synced:
            db.sync()
        out.append(db.export_map_images(0, 128))
        assert db.info()["table_passes"] == (2 if synced else 1)
    (a, ahc), (b, bhc) = out
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and H.entries_equal(ahc, bhc)
    assert sum(len(x) for x in a) > 24 * 300_000


# ---- reader ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DBS)
def test_reader_takes_the_reference_files(golden_dbs, name):
    """files the reference wrote: placed in thread-timing order, a layout our sequential writer never produces"""
    src = os.path.join(golden_dbs, name + ".kreeq")
    want = H.load_db_table(name)
    k = int(open(os.path.join(src, ".index")).read().split()[0])
    db = capi.KreeqDB(k, 128)
    n_sum = t_sum = 0
    for m in range(128):
        n, t = db.import_map_image(m, open(os.path.join(src, f".map.{m}.bin"), "rb").read())
        n_sum, t_sum = n_sum + n, t_sum + t
    assert t_sum == int((want["hc"] != 0).sum()) == 0
    assert n_sum == len(want) == db.info()["slots_used"]
    assert H.entries_equal(db.export(), want)


def test_reader_round_trip_is_additive(edge_db, edge_entries):
    images, _ = edge_db.export_map_images(0, 128)
    db = capi.KreeqDB(21, 128)
    counts = [db.import_map_image(m, img) for m, img in enumerate(images)]
    assert sum(n for n, _ in counts) == len(edge_entries) and counts[EDGE_MAP][0] == len(edge_entries) and all(t == 0 for _, t in counts)
    assert H.entries_equal(db.export(), edge_entries)
    assert db.import_map_image(EDGE_MAP, images[EDGE_MAP].tobytes()) == (len(edge_entries), 0)
    twice = db.export()
    assert np.array_equal(twice["key"], edge_entries["key"]) and np.array_equal(twice["cov"], 2 * edge_entries["cov"])
    assert np.array_equal(twice["fw"], 2 * edge_entries["fw"]) and np.array_equal(twice["bw"], 2 * edge_entries["bw"])


def test_reader_counts_and_skips_tombstones():
    keys = np.array(H.all_canonical_keys(4), dtype=np.uint64)
    entries = random_entries(keys, 8)
    hot = np.arange(len(entries)) % 9 == 0
    entries["cov"][hot] = 1000
    entries["hc"][hot] = 1
    src = capi.KreeqDB(4, 128)
    src.import_entries(entries)
    images, hc = src.export_map_images(0, 128)
    assert len(hc) == hot.sum()
    db = capi.KreeqDB(4, 128)
    counts = [db.import_map_image(m, img) for m, img in enumerate(images)]
    assert sum(n for n, _ in counts) == (~hot).sum() and sum(t for _, t in counts) == hot.sum()
    assert H.entries_equal(db.export(), entries[~hot])
    db.import_entries(hc)
    assert H.entries_equal(db.export(), entries)


def _patch(img, off, data):
    return img[:off] + data + img[off + len(data):]


def test_reader_refuses_malformed_images(edge_db, edge_entries):
    images, _ = edge_db.export_map_images(EDGE_MAP, EDGE_MAP + 1)
    img = images[0].tobytes()
    # the first occupied slot of submap 1 (one entry, capacity 1): header at 8 + 24, then 18 control bytes, then the slot
    hdr = 8 + 24
    assert struct.unpack_from("<QQQ", img, hdr) == (0xFFFFFFFFFFFFFFF5, 1, 1) and img[hdr + 24] < 0x80
    slot = hdr + 24 + 18
    key, = struct.unpack_from("<Q", img, slot)
    cov = img[slot + 16]
    assert key in edge_entries["key"] and cov > 0
    bad = {
        "one byte short": (EDGE_MAP, img[:-1]),
        "one trailing byte": (EDGE_MAP, img + b"\0"),
        "version word changed": (EDGE_MAP, _patch(img, hdr, struct.pack("<Q", 0xFFFFFFFFFFFFFFF4))),
        "size one too large": (EDGE_MAP, _patch(img, 8 + 24 * 6 + sum(24 + n_c + 17 + 24 * n_c + 8 - 24 for n_c in (1, 3, 3, 7, 7)) + 8, struct.pack("<Q", 9))),
        "wrong map": (EDGE_MAP + 1, img),
        "edge counter above cov": (EDGE_MAP, _patch(img, slot + 8, bytes([cov + 1]))),
        "cov 0 under an occupied control byte": (EDGE_MAP, _patch(img, slot + 8, b"\0" * 9)),
    }
    # (the size patch must have hit the size word of submap 6: 8 entries, capacity 15)
    size_off = 8 + 24 * 6 + sum(24 + n_c + 17 + 24 * n_c + 8 - 24 for n_c in (1, 3, 3, 7, 7)) + 8
    assert struct.unpack_from("<QQ", img, size_off) == (8, 15)
    db = capi.KreeqDB(21, 128)
    db.import_map_image(EDGE_MAP, img)
    before, used = db.export(), db.info()["slots_used"]
    assert used == len(edge_entries)
    for what, (m, data) in bad.items():
        with pytest.raises(capi.KqError) as e:
            db.import_map_image(m, data)
        assert e.value.code == INVALID, what
        assert db.info()["slots_used"] == used, what
        assert H.entries_equal(db.export(), before), what
    fresh = capi.KreeqDB(21, 128)
    assert fresh.import_map_image(0, EMPTY_MAP) == (0, 0) and fresh.info()["slots_used"] == 0
