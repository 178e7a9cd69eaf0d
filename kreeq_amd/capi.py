"""ctypes binding of the C ABI (include/kreeq_amd.h).  Thin: argument marshalling and error
translation only -- all compute happens in libkreeq_amd.so on the GPU.  There is no fallback:
if the library is missing or no gfx950 device is visible, calls raise."""
import ctypes as C
import os

import numpy as np

from . import build as _build

ENTRY_DTYPE = np.dtype([("key", "<u8"), ("fw", "<u4", 4), ("bw", "<u4", 4), ("cov", "<u4"), ("hc", "<u4")])
DBGBASE_DTYPE = np.dtype([("fw", "<u4"), ("bw", "<u4"), ("cov", "<u4"), ("isFw", "u1"), ("pad", "u1", 3)])
VARIANT_PATH_DTYPE = np.dtype([("pos", "<u8"), ("seg_start", "<u8"), ("seq_off", "<u8"), ("seq_len", "<u2"), ("ref_len", "<u2"), ("type", "u1"), ("pad", "u1", 3)])      # kq_variant_path
VAR_SNV, VAR_INS, VAR_DEL, VAR_COM = 0, 1, 2, 3      # KQ_VAR_*
ERR_CAPACITY = -6                        # KQ_ERR_CAPACITY

# every symbol include/kreeq_amd.h declares
SYMBOLS = ["kq_create", "kq_destroy", "kq_clear", "kq_set_option", "kq_get_profile", "kq_set_stream", "kq_get_stream", "kq_sync", "kq_flush", "kq_get_info", "kq_last_error",
           "kq_abi_version", "kq_device_available", "kq_device_memory", "kq_count_batch", "kq_count_batch_dev", "kq_host_alloc", "kq_host_free", "kq_count_batch_async", "kq_host_wait", "kq_pack_bases", "kq_count_packed_dev", "kq_count_packed_async",
           "kq_pack_bases_dev", "kq_parse_fastx_dev", "kq_count_fastx_dev", "kq_count_fastx_async", "kq_bgzf_scan", "kq_inflate_bgzf_dev", "kq_count_bgzf_dev", "kq_bgzf_bound", "kq_deflate_bgzf_dev", "kq_deflate_bgzf", "kq_emit_records",
           "kq_emit_partitioned_dev", "kq_emit_packed_dev", "kq_insert_packed_dev", "kq_emit_sharded_dev", "kq_insert_sharded_dev", "kq_emit_sharded8_dev", "kq_insert_sharded8_dev", "kq_insert_records", "kq_insert_records_dev", "kq_summary", "kq_histogram",
           "kq_lookup_sequence", "kq_lookup_sequence_dev", "kq_dev_alloc", "kq_dev_free", "kq_copy_async", "kq_per_base_triples_dev", "kq_per_base_merge_dev", "kq_format_table_dev", "kq_format_table", "kq_lookup_keys", "kq_branch_scan", "kq_search_variants", "kq_merge", "kq_import", "kq_export",
           "kq_export_map_images", "kq_import_map_image", "kq_subgraph_seed", "kq_subgraph_seed_dev", "kq_subgraph_expand", "kq_subgraph_best_first", "kq_subgraph_trim", "kq_subgraph_gfa"]

FASTX_FASTQ, FASTX_FASTA = 1, 2          # KQ_FASTX_FASTQ / KQ_FASTX_FASTA
BGZF_END = 1                             # KQ_BGZF_END
BGZF_EOF = 2                             # KQ_BGZF_EOF
BGZF_MEMBER_TEXT = 0xff00                # text bytes per member written by deflate_bgzf
BGZF_BLOCK_DTYPE = np.dtype([("off", "<u8"), ("size", "<u4"), ("data_off", "<u4"), ("data_len", "<u4"), ("crc32", "<u4"), ("isize", "<u4"), ("pad", "<u4")])      # kq_bgzf_block
TABLE_KWIG, TABLE_BED, TABLE_CSV = 1, 2, 3      # KQ_TABLE_*
TABLE_SEG_HEADER = 1                     # KQ_TABLE_SEG_HEADER
TABLE_SEG_DTYPE = np.dtype([("first", "<u8"), ("n", "<u8"), ("abs_pos", "<u8"), ("name_off", "<u4"), ("name_len", "<u4"), ("n_ctx", "<u4"), ("flags", "<u4")])      # kq_table_seg
SUBGRAPH_NO_REFERENCE = 1                # KQ_SUBGRAPH_NO_REFERENCE
GFA_NO_COLLAPSE = 1                      # KQ_GFA_NO_COLLAPSE
GFA_SEGMENT_DTYPE = np.dtype([("seq_off", "<u8"), ("head_key", "<u8"), ("n_kmers", "<u4"), ("cov", "<u4"), ("head_rc", "u1"), ("pad", "u1", 7)])      # kq_gfa_segment
GFA_EDGE_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4"), ("count", "<u4"), ("from_rc", "u1"), ("to_rc", "u1"), ("pad", "u1", 2)])      # kq_gfa_edge


class KqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"kreeq_amd error {code}: {msg}")
        self.code = code


class Stats(C.Structure):
    _fields_ = [("total", C.c_uint64), ("unique", C.c_uint64), ("distinct", C.c_uint64), ("missing", C.c_uint64),
                ("edges", C.c_uint64)]


class GfaCounts(C.Structure):
    _fields_ = [("n_segments", C.c_uint64), ("n_seq", C.c_uint64), ("n_edges", C.c_uint64), ("n_dropped_edges", C.c_uint64), ("n_cycles", C.c_uint64)]


class Info(C.Structure):
    _fields_ = [("kmers_counted", C.c_uint64), ("slots_used", C.c_uint64), ("slots_total", C.c_uint64), ("hc_used", C.c_uint64),
                ("hc_total", C.c_uint64), ("table_bytes", C.c_uint64), ("table_passes", C.c_uint64)]


_lib = None


def lib_path():
    return _build.LIB


def _preload_process_hip_runtime():
    """One process must hold ONE HIP/HSA runtime.  PyTorch-ROCm wheels bundle their own
    libamdhip64.so.7; if /opt/rocm's copy gets loaded first (through this library's NEEDED entry)
    and torch's afterwards, the second runtime sees no GPU.  So when torch is installed, load its
    copy first: this library's NEEDED soname then resolves to it, and torch later reuses it."""
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.origin:
        return
    d = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            try:
                C.CDLL(p, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def load():
    """Loads libkreeq_amd.so (must have been built: __graft_entry__.build() / kreeq_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("KQ_LIB") or _build.LIB          # KQ_LIB: a tuning variant built by kreeq_amd.build.build_lib(out=...)
    if not os.path.exists(path):
        raise KqError(-2, f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the product has no CPU fallback)")
    _preload_process_hip_runtime()
    L = C.CDLL(path)
    vp, u64, u32, u16, ci = C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint16, C.c_int
    L.kq_create.argtypes = [C.POINTER(vp), ci, ci, ci, u64]
    L.kq_destroy.argtypes = [vp]
    L.kq_destroy.restype = None
    L.kq_clear.argtypes = [vp]
    L.kq_set_stream.argtypes = [vp, vp]
    L.kq_set_option.argtypes = [vp, ci, C.c_int64]
    L.kq_get_profile.argtypes = [vp, C.c_char_p, u64]
    L.kq_get_stream.argtypes = [vp]
    L.kq_get_stream.restype = vp
    L.kq_sync.argtypes = [vp]
    L.kq_flush.argtypes = [vp]
    L.kq_get_info.argtypes = [vp, C.POINTER(Info)]
    L.kq_last_error.restype = C.c_char_p
    L.kq_device_memory.argtypes = [ci, C.POINTER(u64), C.POINTER(u64)]
    L.kq_count_batch.argtypes = [vp, vp, u64]
    L.kq_count_batch_dev.argtypes = [vp, vp, u64]
    L.kq_host_alloc.argtypes = [u64]
    L.kq_host_alloc.restype = vp
    L.kq_host_free.argtypes = [vp]
    L.kq_host_free.restype = None
    L.kq_count_batch_async.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.kq_host_wait.argtypes = [vp, u64]
    L.kq_pack_bases.argtypes = [vp, u64, vp, vp]
    L.kq_pack_bases.restype = None
    L.kq_count_packed_dev.argtypes = [vp, vp, vp, u64]
    L.kq_count_packed_async.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    L.kq_pack_bases_dev.argtypes = [vp, vp, u64, vp, vp]
    L.kq_parse_fastx_dev.argtypes = [vp, vp, u64, ci, vp, u64, C.POINTER(u64)]
    L.kq_count_fastx_dev.argtypes = [vp, vp, u64, ci]
    L.kq_count_fastx_async.argtypes = [vp, vp, u64, ci, C.POINTER(u64)]
    L.kq_bgzf_scan.argtypes = [vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.kq_inflate_bgzf_dev.argtypes = [vp, vp, u64, vp, u64, vp, u64, C.POINTER(u64)]
    L.kq_count_bgzf_dev.argtypes = [vp, vp, u64, vp, u64, ci, u32]
    L.kq_bgzf_bound.argtypes = [u64, u32]
    L.kq_bgzf_bound.restype = u64
    L.kq_deflate_bgzf_dev.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32]
    L.kq_deflate_bgzf.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32]
    L.kq_emit_records.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(u64)]
    L.kq_emit_partitioned_dev.argtypes = [vp, vp, u64, ci, vp, vp, u64, vp]
    L.kq_emit_packed_dev.argtypes = [vp, vp, u64, ci, vp, u64, vp]
    L.kq_insert_packed_dev.argtypes = [vp, vp, u64]
    L.kq_emit_sharded_dev.argtypes = [vp, vp, u64, ci, vp, vp, u64, vp, vp]
    L.kq_insert_sharded_dev.argtypes = [vp, vp, vp, u64, ci, vp]
    L.kq_emit_sharded8_dev.argtypes = [vp, vp, u64, ci, vp, u64, vp, vp]
    L.kq_insert_sharded8_dev.argtypes = [vp, vp, u64, ci, vp]
    L.kq_insert_records.argtypes = [vp, vp, vp, u64]
    L.kq_insert_records_dev.argtypes = [vp, vp, vp, u64]
    L.kq_summary.argtypes = [vp, C.POINTER(Stats)]
    L.kq_histogram.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    L.kq_lookup_sequence.argtypes = [vp, vp, u64, u32, u16, u16, vp, vp]
    L.kq_lookup_sequence_dev.argtypes = [vp, vp, u64, u32, u16, u16, vp, vp]
    L.kq_dev_alloc.argtypes = [vp, u64]
    L.kq_dev_alloc.restype = vp
    L.kq_dev_free.argtypes = [vp, vp]
    L.kq_dev_free.restype = None
    L.kq_copy_async.argtypes = [vp, vp, vp, u64, ci]
    L.kq_per_base_triples_dev.argtypes = [vp, vp, vp, vp, u64, vp]
    L.kq_per_base_merge_dev.argtypes = [vp, vp, vp, vp, u64, vp]
    L.kq_format_table_dev.argtypes = [vp, ci, vp, u64, vp, u64, vp, u64, vp, u64, C.POINTER(u64)]
    L.kq_format_table.argtypes = [vp, ci, vp, u64, vp, u64, vp, u64, vp, u64, C.POINTER(u64)]
    L.kq_lookup_keys.argtypes = [vp, vp, u64, vp]
    L.kq_branch_scan.argtypes = [vp, vp, u64, u32, vp]
    L.kq_search_variants.argtypes = [vp, vp, u64, ci, ci, u32, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64)]
    L.kq_merge.argtypes = [vp, vp]
    L.kq_import.argtypes = [vp, vp, u64]
    L.kq_export.argtypes = [vp, u16, u16, vp, u64, C.POINTER(u64)]
    L.kq_export_map_images.argtypes = [vp, u16, u16, vp, u64, vp, vp, u64, C.POINTER(u64)]
    L.kq_import_map_image.argtypes = [vp, u16, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.kq_subgraph_seed.argtypes = [vp, vp, vp, u64, u32]
    L.kq_subgraph_seed_dev.argtypes = [vp, vp, vp, u64, u32]
    L.kq_subgraph_expand.argtypes = [vp, vp, ci, C.POINTER(u64)]
    L.kq_subgraph_best_first.argtypes = [vp, vp, ci, u32, C.POINTER(u64)]
    L.kq_subgraph_trim.argtypes = [vp, u32]
    L.kq_subgraph_gfa.argtypes = [vp, u32, vp, u64, vp, u64, vp, u64, C.POINTER(GfaCounts)]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise KqError(rc, load().kq_last_error().decode(errors="replace"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def pack_bases(bases: bytes):
    """-> (codes u32[ceil(n/16)], inv u16[ceil(n/16)]): the 2-bit packed form of a batch (kq_pack_bases; host only)"""
    buf = np.frombuffer(bases, dtype=np.uint8)
    units = (len(buf) + 15) // 16
    codes, inv = np.zeros(max(units, 1), dtype=np.uint32), np.zeros(max(units, 1), dtype=np.uint16)
    load().kq_pack_bases(_p(buf) if len(buf) else None, len(buf), _p(codes), _p(inv))
    return codes[:units], inv[:units]


def bgzf_bound(n_text, flags=0):
    """the largest output deflate_bgzf / deflate_bgzf_dev can produce for n_text bytes (kq_bgzf_bound; host only)"""
    return int(load().kq_bgzf_bound(n_text, flags))


def bgzf_scan(data: bytes, cap=None):
    """the BGZF members that lie wholly inside data (kq_bgzf_scan; host only) -> (blocks as BGZF_BLOCK_DTYPE, consumed bytes).
    Raises KqError -1 for a member that is not BGZF (KqError.consumed = its offset, KqError.n_blocks = the blocks before it) and
    -6 when cap is given and too small (KqError.n_blocks = the number needed)"""
    buf = np.frombuffer(data, dtype=np.uint8)
    n, used = C.c_uint64(0), C.c_uint64(0)
    L = load()
    room = len(buf) // 26 + 1 if cap is None else cap          # no member is shorter than 26 bytes
    blocks = np.zeros(max(room, 1), dtype=BGZF_BLOCK_DTYPE)
    rc = L.kq_bgzf_scan(_p(buf) if len(buf) else None, len(buf), _p(blocks) if room else None, room, C.byref(n), C.byref(used))
    if rc != 0:
        e = KqError(rc, L.kq_last_error().decode(errors="replace"))
        e.n_blocks, e.consumed = n.value, used.value
        raise e
    return blocks[:n.value], used.value


def device_available():
    return bool(load().kq_device_available())


def device_memory(device=0):
    """(free, total) HBM bytes"""
    f, t = C.c_uint64(0), C.c_uint64(0)
    _check(load().kq_device_memory(device, C.byref(f), C.byref(t)))
    return f.value, t.value


class KreeqDB:
    """One k-mer database resident on one GPU (mirrors the reference's DBG object for the hot path)."""

    def __init__(self, k=21, map_count=128, device=0, capacity_hint=0):
        self.k, self.map_count, self.device = k, map_count, device
        self._h = C.c_void_p()
        _check(load().kq_create(C.byref(self._h), device, k, map_count, capacity_hint))

    def close(self, _load=load):                 # bound at definition: module globals may be gone at interpreter exit
        if getattr(self, "_h", None):
            _load().kq_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def handle(self):
        return self._h

    # -- stream / state
    def set_stream(self, hip_stream_ptr):
        _check(load().kq_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def sync(self):
        _check(load().kq_sync(self._h))

    def flush(self):
        """apply pending record sets now (asynchronous)"""
        _check(load().kq_flush(self._h))

    def set_option(self, option, value):
        """option: 'trust_capacity' | 'count_path' ('auto'|'direct'|'partitioned') | 'slice_kmers' | 'count_map_range' ((lo, hi)) |
        'kernel_set' (measurement only: mask of bits 1, 2, 4, 16, 32, 64, 128 -- KQ_OPT_KERNEL_SET in include/kreeq_amd.h; 32 / 64 = the last
        split level never / wherever possible with one workgroup per segment; 128 = the previous P1 scatter behind a map-range filter) | ..."""
        opt = {"trust_capacity": 1, "count_path": 2, "slice_kmers": 3, "count_map_range": 4, "profile": 5, "lookup_path": 6, "merge_path": 7, "narrow_mid": 8, "pending_bytes": 9, "bucket_window": 10, "overlap": 11, "count_map_passes": 12, "kernel_set": 13, "shard_window": 14, "subgraph_batch": 15, "variant_batch": 16, "test_fail_plan": 100, "test_export": 101}[option]
        if option == "count_map_range":
            value = int(value[0]) | (int(value[1]) << 16)
        if option in ("count_path", "lookup_path", "merge_path"):
            value = {"auto": 0, "direct": 1, "partitioned": 2}[value]
        _check(load().kq_set_option(self._h, opt, int(value)))

    def clear(self):
        _check(load().kq_clear(self._h))

    def profile(self):
        """{stage: ms} of the last partitioned count (needs set_option('profile', 1))"""
        buf = C.create_string_buffer(1024)
        _check(load().kq_get_profile(self._h, buf, 1024))
        return {k: float(v) for k, v in (kv.split("=") for kv in buf.value.decode().split(";") if kv)}

    def info(self):
        i = Info()
        _check(load().kq_get_info(self._h, C.byref(i)))
        return {f: getattr(i, f) for f, _ in Info._fields_}

    # -- count
    def count_batch(self, bases: bytes):
        buf = np.frombuffer(bases, dtype=np.uint8)
        _check(load().kq_count_batch(self._h, _p(buf), len(buf)))

    def count_batch_async(self, host_ptr, n):
        """pipelined ingest: enqueue copy + count of a host batch (pinned memory from host_alloc); returns the ticket to wait
        on before the buffer is refilled"""
        t = C.c_uint64(0)
        _check(load().kq_count_batch_async(self._h, C.c_void_p(host_ptr), n, C.byref(t)))
        return t.value

    def count_packed_dev(self, codes_ptr, inv_ptr, n_bases):
        _check(load().kq_count_packed_dev(self._h, C.c_void_p(codes_ptr), C.c_void_p(inv_ptr), n_bases))

    def count_packed_async(self, codes_ptr, inv_ptr, n_bases):
        """pipelined ingest of a 2-bit packed batch (pack_bases); returns the ticket to wait on before the arrays are refilled"""
        t = C.c_uint64(0)
        _check(load().kq_count_packed_async(self._h, C.c_void_p(codes_ptr), C.c_void_p(inv_ptr), n_bases, C.byref(t)))
        return t.value

    def pack_bases_dev(self, bases_ptr, n, codes_ptr, inv_ptr):
        """device ASCII -> the packed form (kq_pack_bases' layout: ceil(n / 16) u32 + u16), asynchronous on the handle's stream"""
        _check(load().kq_pack_bases_dev(self._h, C.c_void_p(bases_ptr), n, C.c_void_p(codes_ptr), C.c_void_p(inv_ptr)))

    def parse_fastx_dev(self, text_ptr, n, fmt, out_ptr, cap):
        """device FASTQ / FASTA text (whole records) -> the read batch at out_ptr (room for cap bytes); returns its size.
        out_ptr None / 0: the size only.  Raises KqError -6 when cap is too small (KqError.needed holds the size), -1 for
        malformed text"""
        nb = C.c_uint64(0)
        rc = load().kq_parse_fastx_dev(self._h, C.c_void_p(text_ptr), n, fmt, C.c_void_p(out_ptr) if out_ptr else None, cap, C.byref(nb))
        if rc != 0:
            e = KqError(rc, load().kq_last_error().decode(errors="replace"))
            e.needed = nb.value
            raise e
        return nb.value

    def count_fastx_dev(self, text_ptr, n, fmt):
        """parse device text + count it, like count_batch_dev of its read batch"""
        _check(load().kq_count_fastx_dev(self._h, C.c_void_p(text_ptr), n, fmt))

    def count_fastx_async(self, host_ptr, n, fmt):
        """pipelined ingest of raw FASTQ / FASTA text (pinned memory from host_alloc): copy, parse and count on the device;
        returns the ticket to wait on before the buffer is refilled (host_wait raises for malformed text)"""
        t = C.c_uint64(0)
        _check(load().kq_count_fastx_async(self._h, C.c_void_p(host_ptr), n, fmt, C.byref(t)))
        return t.value

    def inflate_bgzf_dev(self, comp_ptr, comp_len, blocks, out_ptr, cap):
        """BGZF members in device memory (blocks: BGZF_BLOCK_DTYPE, offsets relative to comp_ptr) -> their text at out_ptr (room
        for cap bytes); returns its size.  out_ptr None / 0: the size only.  Raises KqError -6 when cap is too small
        (KqError.needed holds the size), -1 for a bad list or a corrupt member (the message names the first one)"""
        blocks = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        nt = C.c_uint64(0)
        rc = load().kq_inflate_bgzf_dev(self._h, C.c_void_p(comp_ptr), comp_len, _p(blocks) if len(blocks) else None, len(blocks),
                                        C.c_void_p(out_ptr) if out_ptr else None, cap, C.byref(nt))
        if rc != 0:
            e = KqError(rc, load().kq_last_error().decode(errors="replace"))
            e.needed = nt.value
            raise e
        return nt.value

    def deflate_bgzf_dev(self, text_ptr, n_text, out_ptr, cap, flags=0):
        """device text -> BGZF members at out_ptr (device, room for cap bytes); returns the bytes written.  flags = BGZF_EOF
        appends the end-of-file marker.  Raises KqError -6 when cap is below bgzf_bound(n_text, flags) (KqError.needed holds it)"""
        no = C.c_uint64(0)
        rc = load().kq_deflate_bgzf_dev(self._h, C.c_void_p(text_ptr) if text_ptr else None, n_text, C.c_void_p(out_ptr) if out_ptr else None, cap, C.byref(no), flags)
        if rc != 0:
            e = KqError(rc, load().kq_last_error().decode(errors="replace"))
            e.needed = no.value
            raise e
        return no.value

    def deflate_bgzf(self, text: bytes, flags=0, cap=None):
        """host text -> its BGZF members as bytes (kq_deflate_bgzf: staging, the device call, the copy back)"""
        src = np.frombuffer(text, dtype=np.uint8)
        room = bgzf_bound(len(src), flags) if cap is None else cap
        out = np.empty(max(room, 1), dtype=np.uint8)
        no = C.c_uint64(0)
        rc = load().kq_deflate_bgzf(self._h, _p(src) if len(src) else None, len(src), _p(out) if room else None, room, C.byref(no), flags)
        if rc != 0:
            e = KqError(rc, load().kq_last_error().decode(errors="replace"))
            e.needed = no.value
            raise e
        return out[:no.value].tobytes()

    def count_bgzf_dev(self, comp_ptr, comp_len, blocks, fmt, flags=0):
        """one piece of a BGZF stream from device memory: inflate behind the carry, count the whole records, keep the rest;
        flags = BGZF_END on the last piece"""
        blocks = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        _check(load().kq_count_bgzf_dev(self._h, C.c_void_p(comp_ptr), comp_len, _p(blocks) if len(blocks) else None, len(blocks), fmt, flags))

    def host_wait(self, ticket):
        _check(load().kq_host_wait(self._h, ticket))

    def count_batch_dev(self, ptr, n):
        _check(load().kq_count_batch_dev(self._h, C.c_void_p(ptr), n))

    def emit_records(self, bases: bytes):
        buf = np.frombuffer(bases, dtype=np.uint8)
        n = C.c_uint64(0)
        _check(load().kq_emit_records(self._h, _p(buf), len(buf), None, None, 0, C.byref(n)))
        keys = np.empty(n.value, dtype=np.uint64)
        edges = np.empty(n.value, dtype=np.uint8)
        if n.value:
            _check(load().kq_emit_records(self._h, _p(buf), len(buf), _p(keys), _p(edges), n.value, C.byref(n)))
        return keys, edges

    def emit_partitioned_dev(self, bases_ptr, n, n_parts, keys_ptr, edges_ptr, cap):
        counts = np.zeros(n_parts, dtype=np.uint64)
        _check(load().kq_emit_partitioned_dev(self._h, C.c_void_p(bases_ptr), n, n_parts, C.c_void_p(keys_ptr), C.c_void_p(edges_ptr),
                                              cap, _p(counts)))
        return counts

    def emit_packed_dev(self, bases_ptr, n, n_parts, recs_ptr, cap):
        counts = np.zeros(n_parts, dtype=np.uint64)
        _check(load().kq_emit_packed_dev(self._h, C.c_void_p(bases_ptr), n, n_parts, C.c_void_p(recs_ptr), cap, _p(counts)))
        return counts

    def insert_packed_dev(self, recs_ptr, n):
        _check(load().kq_insert_packed_dev(self._h, C.c_void_p(recs_ptr), n))

    def emit_sharded_dev(self, bases_ptr, n, n_parts, recs_ptr, aux_ptr, cap, bucket_counts_ptr, sync=True):
        """sync=False: only enqueues and returns None (the part sizes are the row sums of the device bucket counts)"""
        counts = np.zeros(n_parts, dtype=np.uint64) if sync else None
        _check(load().kq_emit_sharded_dev(self._h, C.c_void_p(bases_ptr), n, n_parts, C.c_void_p(recs_ptr), C.c_void_p(aux_ptr), cap,
                                          C.c_void_p(bucket_counts_ptr), _p(counts)))
        return counts

    def insert_sharded_dev(self, recs_ptr, aux_ptr, n, n_peers, bucket_counts_ptr):
        _check(load().kq_insert_sharded_dev(self._h, C.c_void_p(recs_ptr), C.c_void_p(aux_ptr), n, n_peers, C.c_void_p(bucket_counts_ptr)))

    def emit_sharded8_dev(self, bases_ptr, n, n_parts, recs_ptr, cap, bucket_counts_ptr, sync=True):
        """k = 29..32: bucket-sorted 8-byte hash-remainder records (one u64 array); sync=False only enqueues and returns None"""
        counts = np.zeros(n_parts, dtype=np.uint64) if sync else None
        _check(load().kq_emit_sharded8_dev(self._h, C.c_void_p(bases_ptr), n, n_parts, C.c_void_p(recs_ptr), cap,
                                           C.c_void_p(bucket_counts_ptr), _p(counts)))
        return counts

    def insert_sharded8_dev(self, recs_ptr, n, n_peers, bucket_counts_ptr):
        _check(load().kq_insert_sharded8_dev(self._h, C.c_void_p(recs_ptr), n, n_peers, C.c_void_p(bucket_counts_ptr)))

    def insert_records(self, keys, edges):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        edges = np.ascontiguousarray(edges, dtype=np.uint8)
        assert len(keys) == len(edges)
        _check(load().kq_insert_records(self._h, _p(keys), _p(edges), len(keys)))

    def insert_records_dev(self, keys_ptr, edges_ptr, n):
        _check(load().kq_insert_records_dev(self._h, C.c_void_p(keys_ptr), C.c_void_p(edges_ptr), n))

    # -- summary
    def summary(self, with_hist=False):
        st = Stats()
        _check(load().kq_summary(self._h, C.byref(st)))
        d = {f: getattr(st, f) for f, _ in Stats._fields_}
        if with_hist:
            n = C.c_uint64(0)
            _check(load().kq_histogram(self._h, None, None, 0, C.byref(n)))
            cov = np.zeros(n.value, dtype=np.uint64)
            cnt = np.zeros(n.value, dtype=np.uint64)
            _check(load().kq_histogram(self._h, _p(cov), _p(cnt), n.value, C.byref(n)))
            d["hist"] = dict(zip(cov.tolist(), cnt.tolist()))
        return d

    # -- lookup
    def lookup_sequence(self, bases: bytes, cov_cutoff=0, map_lo=0, map_hi=None, per_base=False, per_base_buf=None):
        if map_hi is None:
            map_hi = self.map_count
        buf = np.frombuffer(bases, dtype=np.uint8)
        ctr = np.zeros(3, dtype=np.uint64)
        pb = per_base_buf if per_base_buf is not None else (np.zeros(len(buf), dtype=DBGBASE_DTYPE) if per_base else None)
        _check(load().kq_lookup_sequence(self._h, _p(buf), len(buf), cov_cutoff, map_lo, map_hi, _p(pb), _p(ctr)))
        return ctr, pb

    def lookup_sequence_dev(self, bases_ptr, n, counters_ptr, cov_cutoff=0, map_lo=0, map_hi=None, per_base_ptr=None):
        if map_hi is None:
            map_hi = self.map_count
        _check(load().kq_lookup_sequence_dev(self._h, C.c_void_p(bases_ptr), n, cov_cutoff, map_lo, map_hi,
                                             C.c_void_p(per_base_ptr) if per_base_ptr else None, C.c_void_p(counters_ptr)))

    # -- per-base tables
    def per_base_triples_dev(self, per_base_ptr, segments, triples_ptr):
        """segments = [(start, len)] inside the device per-base array -> their oriented triples at triples_ptr (device, 12 bytes
        per position); asynchronous on the handle's stream"""
        start = np.array([s for s, _ in segments], dtype=np.uint64)
        length = np.array([n for _, n in segments], dtype=np.uint64)
        _check(load().kq_per_base_triples_dev(self._h, C.c_void_p(per_base_ptr), _p(start), _p(length), len(segments), C.c_void_p(triples_ptr)))

    def per_base_merge_dev(self, per_base_ptr, segments, triples_ptr):
        """one map-range pass folded into the accumulated triples at triples_ptr: the stored (non-zero) entries of the listed
        segments overwrite their triples and are zeroed, zero entries leave theirs alone; asynchronous on the handle's stream"""
        start = np.array([s for s, _ in segments], dtype=np.uint64)
        length = np.array([n for _, n in segments], dtype=np.uint64)
        _check(load().kq_per_base_merge_dev(self._h, C.c_void_p(per_base_ptr), _p(start), _p(length), len(segments), C.c_void_p(triples_ptr)))

    def format_table_raw(self, fmt, triples, n_triples, segs, n_segs, names, names_len, out, cap, n_out=True, dev=False):
        """kq_format_table(_dev) as it is; every pointer a ctypes pointer / address or None -> (return code, *n_out)"""
        n = C.c_uint64(0)
        f = load().kq_format_table_dev if dev else load().kq_format_table
        rc = f(self._h, fmt, triples, n_triples, segs, n_segs, names, names_len, out, cap, C.byref(n) if n_out else None)
        return rc, n.value

    def format_table(self, fmt, triples, segs, names: bytes):
        """triples: uint32 [n, 3] (the .bkwig payload), segs: TABLE_SEG_DTYPE array, names: the bytes name_off / name_len point
        into -> the table text (size query, then the text)"""
        t = np.ascontiguousarray(triples, dtype=np.uint32).reshape(-1, 3)
        segs = np.ascontiguousarray(segs, dtype=TABLE_SEG_DTYPE)
        nb = np.frombuffer(names, dtype=np.uint8)
        args = (fmt, _p(t) if len(t) else None, len(t), _p(segs) if len(segs) else None, len(segs), _p(nb) if len(nb) else None, len(nb))
        rc, need = self.format_table_raw(*args, None, 0)
        _check(rc)
        out = np.zeros(max(need, 1), dtype=np.uint8)
        rc, need = self.format_table_raw(*args, _p(out), need)
        _check(rc)
        return out[:need].tobytes()

    def lookup_keys(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(len(keys), dtype=ENTRY_DTYPE)
        _check(load().kq_lookup_keys(self._h, _p(keys), len(keys), _p(out)))
        return out

    def branch_scan(self, bases: bytes, cov_cutoff=0):
        buf = np.frombuffer(bases, dtype=np.uint8)
        flags = np.zeros(len(buf), dtype=np.uint8)
        _check(load().kq_branch_scan(self._h, _p(buf), len(buf), cov_cutoff, _p(flags)))
        return flags

    def search_variants_raw(self, bases: bytes, depth, max_span, cov_cutoff=0, path_cap=None, seq_cap=None):
        """kq_search_variants as it is: path_cap None = the two counts only -> (return code, n_paths, n_seq, records, sequence bytes)"""
        buf = np.frombuffer(bases, dtype=np.uint8)
        n_paths, n_seq = C.c_uint64(0), C.c_uint64(0)
        paths = np.zeros(max(path_cap, 1), dtype=VARIANT_PATH_DTYPE) if path_cap is not None else None
        seq = np.zeros(max(seq_cap, 1), dtype=np.uint8) if path_cap is not None else None
        rc = load().kq_search_variants(self._h, _p(buf) if len(buf) else None, len(buf), depth, max_span, cov_cutoff, _p(paths), path_cap or 0, C.byref(n_paths),
                                       _p(seq), seq_cap or 0, C.byref(n_seq))
        return rc, n_paths.value, n_seq.value, paths, seq

    def search_variants(self, bases: bytes, depth, max_span, cov_cutoff=0):
        """The candidate-error searches of `validate -o vcf` on the device (kq_search_variants): -> [(pos, seg_start, type,
        ref_len, sequence)] in ascending pos, destination order within one position.  Modest buffers first; when they are
        too small the call is repeated ONCE with the sizes it reported (the searches run again)."""
        path_cap, seq_cap = 1 << 12, 1 << 16
        rc, n_paths, n_seq, paths, seq = self.search_variants_raw(bases, depth, max_span, cov_cutoff, path_cap, seq_cap)
        if rc == ERR_CAPACITY:
            rc, n_paths, n_seq, paths, seq = self.search_variants_raw(bases, depth, max_span, cov_cutoff, n_paths, n_seq)
        _check(rc)
        text = seq.tobytes()
        return [(int(p["pos"]), int(p["seg_start"]), int(p["type"]), int(p["ref_len"]), text[int(p["seq_off"]):int(p["seq_off"]) + int(p["seq_len"])].decode())
                for p in paths[:n_paths]]

    # -- union / io
    def merge(self, other):
        _check(load().kq_merge(self._h, other._h))

    def import_entries(self, entries):
        entries = np.ascontiguousarray(entries, dtype=ENTRY_DTYPE)
        _check(load().kq_import(self._h, _p(entries), len(entries)))

    def export(self, map_lo=0, map_hi=None):
        if map_hi is None:
            map_hi = self.map_count
        n = C.c_uint64(0)
        _check(load().kq_export(self._h, map_lo, map_hi, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=ENTRY_DTYPE)
        if n.value:
            _check(load().kq_export(self._h, map_lo, map_hi, _p(out), n.value, C.byref(n)))
        return out

    def export_map_images(self, map_lo=0, map_hi=None, sizes_only=False):
        """-> (images, hc): images[i] = the bytes of <db>/.map.<map_lo + i>.bin (uint8 arrays), hc = the high-copy entries of
        the range in key order.  sizes_only: -> (offsets u64[n_maps + 1], n_hc) from the size query alone"""
        if map_hi is None:
            map_hi = self.map_count
        offsets = np.zeros(map_hi - map_lo + 1, dtype=np.uint64)
        n_hc = C.c_uint64(0)
        _check(load().kq_export_map_images(self._h, map_lo, map_hi, None, 0, _p(offsets), None, 0, C.byref(n_hc)))
        if sizes_only:
            return offsets, n_hc.value
        buf = np.zeros(max(int(offsets[-1]), 1), dtype=np.uint8)
        hc = np.zeros(max(n_hc.value, 1), dtype=ENTRY_DTYPE)
        filled = np.zeros_like(offsets)
        _check(load().kq_export_map_images(self._h, map_lo, map_hi, _p(buf), int(offsets[-1]), _p(filled), _p(hc), n_hc.value, C.byref(n_hc)))
        return [buf[int(filled[i]):int(filled[i + 1])] for i in range(map_hi - map_lo)], hc[:n_hc.value]

    def import_map_image(self, map_index, image):
        """adds the k-mers of one <db>/.map.<m>.bin (bytes or a uint8 array); -> (entries added, tombstones skipped)"""
        buf = np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray, memoryview)) else np.ascontiguousarray(image, dtype=np.uint8)
        n, t = C.c_uint64(0), C.c_uint64(0)
        _check(load().kq_import_map_image(self._h, map_index, _p(buf), len(buf), C.byref(n), C.byref(t)))
        return n.value, t.value

    # -- subgraph (reference src/subgraph.cpp): `sub` is a second KreeqDB with this one's k, map_count and device
    def subgraph_seed(self, sub, bases: bytes, no_reference=False):
        """adds the k-mers of a sequence batch (segments = ACGT runs) to `sub`: database entries, or constructed k-mers"""
        buf = np.frombuffer(bases, dtype=np.uint8)
        _check(load().kq_subgraph_seed(self._h, sub._h, _p(buf) if len(buf) else None, len(buf), SUBGRAPH_NO_REFERENCE if no_reference else 0))

    def subgraph_seed_dev(self, sub, bases_ptr, n, no_reference=False):
        _check(load().kq_subgraph_seed_dev(self._h, sub._h, C.c_void_p(bases_ptr), n, SUBGRAPH_NO_REFERENCE if no_reference else 0))

    def subgraph_expand(self, sub, depth):
        """`depth` rounds of the traversal from the k-mers of `sub` through this database; -> k-mers added"""
        n = C.c_uint64(0)
        _check(load().kq_subgraph_expand(self._h, sub._h, depth, C.byref(n)))
        return n.value

    def subgraph_best_first(self, sub, depth, cov_cutoff=0):
        """one best-first search of at most depth + 1 pops per k-mer of `sub` through this database, every search on the GPU
        (set_option('subgraph_batch', n) on this handle fixes the searches per batch); -> k-mers added"""
        n = C.c_uint64(0)
        _check(load().kq_subgraph_best_first(self._h, sub._h, depth, cov_cutoff, C.byref(n)))
        return n.value

    def subgraph_trim(self, cov_cutoff=0):
        """clears the edge counters > cov_cutoff of THIS table (a subgraph) that lead to k-mers outside it"""
        _check(load().kq_subgraph_trim(self._h, cov_cutoff))

    def subgraph_gfa_raw(self, no_collapse=False, caps=None, flags=None):
        """kq_subgraph_gfa as it is on THIS table (a subgraph): caps None = the counts only, else (seg_cap, seq_cap, edge_cap)
        -> (return code, counts dict, segs, seq, edges); the buffers hold one element more than their cap, for the tests"""
        cnt = GfaCounts()
        flags = (GFA_NO_COLLAPSE if no_collapse else 0) if flags is None else flags
        segs = seq = edges = None
        if caps is not None:
            segs, seq, edges = np.zeros(caps[0] + 1, dtype=GFA_SEGMENT_DTYPE), np.zeros(caps[1] + 1, dtype=np.uint8), np.zeros(caps[2] + 1, dtype=GFA_EDGE_DTYPE)
        rc = load().kq_subgraph_gfa(self._h, flags, _p(segs), caps[0] if caps else 0, _p(seq), caps[1] if caps else 0, _p(edges), caps[2] if caps else 0, C.byref(cnt))
        return rc, {name: int(getattr(cnt, name)) for name, _ in GfaCounts._fields_}, segs, seq, edges

    def subgraph_gfa(self, no_collapse=False):
        """THIS table (a trimmed subgraph) as a graph, built on the device (kq_subgraph_gfa): unitigs, or with no_collapse one
        segment per k-mer -> (segs GFA_SEGMENT_DTYPE[], sequence bytes, edges GFA_EDGE_DTYPE[], counts dict).  Two calls: the
        sizes, then the arrays."""
        rc, counts, _, _, _ = self.subgraph_gfa_raw(no_collapse)
        _check(rc)
        rc, counts, segs, seq, edges = self.subgraph_gfa_raw(no_collapse, (counts["n_segments"], counts["n_seq"], counts["n_edges"]))
        _check(rc)
        return segs[:counts["n_segments"]], seq[:counts["n_seq"]].tobytes(), edges[:counts["n_edges"]], counts

    def subgraph(self, seq: bytes, depth, algorithm="traversal", no_reference=False, cov_cutoff=0):
        """seed + expand + trim -> the subgraph as a new KreeqDB.  Only the traversal runs through this binding (best-first is
        the CLI's: `kreeq subgraph`)."""
        if algorithm != "traversal":
            raise ValueError(f"algorithm {algorithm!r}: only 'traversal' is available here (best-first: the kreeq CLI)")
        sub = KreeqDB(self.k, self.map_count, self.device, capacity_hint=len(seq) + 1024)
        self.subgraph_seed(sub, seq, no_reference)
        self.subgraph_expand(sub, depth)
        sub.subgraph_trim(cov_cutoff)
        return sub
