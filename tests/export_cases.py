"""Constructed tables for the tests of kq_export (tests/test_gpu_export.py; checked without a GPU by tests/test_export_cases.py).

A case is (k, n, modes).  Its table is entries(k, n): n distinct canonical keys with a payload that is a function of the key, so
that an entry gathered through a wrong index, or a payload that travelled with another key, cannot compare equal:

  cov      1 + key % 300: both tiers (the 8-bit one up to 254, the high-copy side table from 255)
  fw, bw   one 16-bit field of a 64-bit mix of the key per counter (a different field for each of the 8), modulo cov + 1
  hc       cov > 254

From n = 4 every key set holds key 0 (A^k), the largest canonical key of k, a pair that differs in bit 0 only (0 and 1: A^k and
CA^(k-1)) and a pair that differs in bit 2k - 1 only (0 and 2^(2k-1): A^k and A^(k-1)G; at k = 32 that key is 2^63); from
n = 64 eight more pairs of each kind.  The reference of an export is this array itself, filtered by key % map_count and sorted
by key with numpy.

What the sizes are chosen against (read from the installed rocPRIM, rocprim/device/device_radix_sort.hpp and
detail/config/device_radix_sort_onesweep.hpp, default configuration, u64 keys with u32 values on gfx950):

  n <= 1024              one workgroup sorts everything (radix_sort_block_sort, 256 threads x 4 items)
  1024 < n <= 1 048 576  block sorts of 1024 items, then merge passes (radix_sort_merge_impl; merge_sort_limit = 1024 * 1024);
                         the comparison looks at bits [0, 2k)
  n > 1 048 576          onesweep: ceil(2k / 8) digit passes of 8 bits (the last one narrower), blocks of 512 x 16 = 8192 items;
                         with an odd number of passes the first one writes the caller's output arrays, with an even number the
                         temporary ones; the result always ends in the output arrays

and the copy out (kreeq_amd/csrc/kq_export_host.h): one hipMemcpy up to 64 MiB = 1 398 101 entries of 48 bytes, from 1 398 102
entries chunks of 16 MiB through two pinned buffers.  Test mode bit 0 sorts on the host, bit 1 takes chunks of 4096 bytes at
any size (85 entries and a third: entries straddle chunks)."""
import functools

import numpy as np

from tests import helpers as H

ENTRY_DTYPE = np.dtype([("key", "<u8"), ("fw", "<u4", 4), ("bw", "<u4", 4), ("cov", "<u4"), ("hc", "<u4")])      # kq_entry, 48 bytes
ENTRY_BYTES = 48
LARGEST = (1 << 32) - 1
EMPTY_KEY = (1 << 64) - 1

MODES = {"default": 0, "host_sort": 1, "bounced": 2, "host_sort_bounced": 3}      # values of KQ_OPT_TEST_EXPORT
ALL_MODES = tuple(MODES)

# sort algorithm and copy path of an export of n entries in default mode
BLOCK_SORT_MAX, MERGE_SORT_MAX, ONESWEEP_BITS = 1024, 1 << 20, 8
DIRECT_MAX_BYTES, CHUNK_BYTES, TEST_CHUNK_BYTES = 64 << 20, 16 << 20, 4096

SIZE_KS = (11, 21)
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537)       # all four modes
BIG_SIZES = (1_048_576,          # the largest merge sort; 48 MiB: three chunks' worth in one copy
             1_398_101,          # the last direct size; onesweep from here
             1_398_102,          # the first bounced size: 5 chunks, the last one 32 bytes
             2_097_152)          # 6 chunks exactly; at k = 11 every canonical 11-mer
SWEEP_KS = (2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 31, 32)      # 2k on both sides of every multiple of 8
SWEEP_N = 70_000                 # merge sort (or less where k has fewer keys)
SWEEP_BIG_KS = (12, 13, 16, 17, 24, 25, 28, 29, 32)      # onesweep passes: 3, 4, 4, 5, 6, 7, 7, 8, 8
SWEEP_BIG_N = 1_500_000


def sort_algorithm(n):
    return "block" if n <= BLOCK_SORT_MAX else "merge" if n <= MERGE_SORT_MAX else "onesweep"


def sort_passes(k):
    return -(-2 * k // ONESWEEP_BITS)


def copy_plan(n, mode):
    """-> ("direct" | "bounced", chunks, bytes of the last chunk) of an export of n entries"""
    nbytes = n * ENTRY_BYTES
    chunk = TEST_CHUNK_BYTES if MODES[mode] & 2 else CHUNK_BYTES
    if not (nbytes > 0 if MODES[mode] & 2 else nbytes > DIRECT_MAX_BYTES):
        return "direct", 0, nbytes
    chunks = -(-nbytes // chunk)
    return "bounced", chunks, nbytes - (chunks - 1) * chunk


def cases():
    """[(k, n, modes)] in the order the GPU test runs them"""
    out = [(k, n, ALL_MODES) for k in SIZE_KS for n in SIZES]
    out += [(k, n, ("default",)) for k in SIZE_KS for n in BIG_SIZES]
    out += [(k, min(H.n_canonical(k), SWEEP_N), ALL_MODES) for k in SWEEP_KS]
    out += [(k, SWEEP_BIG_N, ("default",)) for k in SWEEP_BIG_KS]
    return out


def case_id(case):
    return f"k{case[0]}-n{case[1]}"


# ---- keys ------------------------------------------------------------------------------------------------------------------
def required_keys(k):
    """key 0, the largest canonical key, the partner of 0 in bit 0 and its partner in bit 2k - 1"""
    return [0, H.max_canonical_key(k), 1, 1 << (2 * k - 1)]


def pair_keys(k, seed, n_pairs=8):
    """-> (keys that come with their partner in bit 0, keys that come with their partner in bit 2k - 1), the partners not included.
    A k-mer that begins with A and ends with A or C is canonical (its reverse complement ends with T), and stays so with C as its
    first base (then its reverse complement ends with G); one that begins and ends with A stays so with G as its last base"""
    if k < 3:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    rng = np.random.default_rng([k, seed, 77])
    mid = np.unique(rng.integers(1, 1 << (2 * k - 4), 2 * n_pairs, dtype=np.uint64))      # the bases between the first and the last
    low = (mid[:len(mid) // 2] << np.uint64(2)) | (rng.integers(0, 2, len(mid) // 2, dtype=np.uint64) << np.uint64(2 * k - 2))
    top = mid[len(mid) // 2:] << np.uint64(2)
    return low, top


@functools.lru_cache(maxsize=2)
def keys_of(k, n, seed=0):
    """n distinct canonical keys of k, unsorted (in a fixed random order)"""
    total = H.n_canonical(k)
    assert n <= total, (k, n, total)
    rng = np.random.default_rng([k, n, seed])
    must = list(required_keys(k))
    if n >= 64:
        low, top = pair_keys(k, seed)
        must += low.tolist() + (low ^ np.uint64(1)).tolist() + top.tolist() + (top | np.uint64(1 << (2 * k - 1))).tolist()
    must = np.array(list(dict.fromkeys(must))[:n], dtype=np.uint64)
    if k <= 11:                                             # a random subset of the whole key space
        pool = H.all_canonical_keys(k)
        pool = pool[~np.isin(pool, must)]
        rest = pool if n - len(must) == len(pool) else rng.choice(pool, n - len(must), replace=False)
    else:                                                   # random k-mers, made canonical
        rest = np.zeros(0, dtype=np.uint64)
        while len(rest) < n - len(must):
            want = n - len(must) - len(rest)
            x = rng.integers(0, 1 << (2 * k), want + want // 4 + 64, dtype=np.uint64) if k < 32 else rng.integers(0, EMPTY_KEY, want + want // 4 + 64, dtype=np.uint64, endpoint=True)
            x = H.canonical_keys_of(x, k)
            rest = np.unique(np.concatenate([rest, x[~np.isin(x, must)]]))
            if len(rest) > n - len(must):
                rest = rng.choice(rest, n - len(must), replace=False)
    keys = np.concatenate([must, rest.astype(np.uint64)])
    keys = keys[rng.permutation(len(keys))]
    keys.setflags(write=False)
    return keys


# ---- payload ---------------------------------------------------------------------------------------------------------------
def _mix(x, mult):
    x = x * np.uint64(mult)
    x ^= x >> np.uint64(29)
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    return x ^ (x >> np.uint64(32))


def entries_from_keys(keys):
    """the entry of every key, in the order of `keys`"""
    keys = np.asarray(keys, dtype=np.uint64)
    e = np.zeros(len(keys), dtype=ENTRY_DTYPE)
    e["key"] = keys
    cov = np.uint64(1) + keys % np.uint64(300)
    e["cov"] = cov
    with np.errstate(over="ignore"):
        h_fw, h_bw = _mix(keys + np.uint64(1), 0x9E3779B97F4A7C15), _mix(keys + np.uint64(1), 0xD6E8FEB86659FD93)
    for w in range(4):
        e["fw"][:, w] = ((h_fw >> np.uint64(16 * w)) & np.uint64(0xFFFF)) % (cov + np.uint64(1))
        e["bw"][:, w] = ((h_bw >> np.uint64(16 * w)) & np.uint64(0xFFFF)) % (cov + np.uint64(1))
    e["hc"] = cov > np.uint64(254)
    return e


@functools.lru_cache(maxsize=2)
def entries(k, n, seed=0):
    e = entries_from_keys(keys_of(k, n, seed))
    e.setflags(write=False)
    return e


def saturated_entries(k=21, n=600):
    """cov and counters at the tier boundary and at the clamp: cov cycles through 254, 255, 256 and 2^32 - 1 by key rank; counter w
    of an entry is cov, cov - 1, 255, 254, 1, 0, ... in a rotation that depends on the key"""
    e = entries_from_keys(np.sort(keys_of(k, n, seed=5)))
    cov = np.array([254, 255, 256, LARGEST], dtype=np.uint64)[np.arange(n) % 4]
    menu = np.stack([cov, cov - np.uint64(1), np.minimum(cov, np.uint64(255)), np.minimum(cov, np.uint64(254)), np.ones(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64),
                     np.minimum(cov, np.uint64(256)), cov // np.uint64(2)], axis=1)
    rot = (e["key"] % np.uint64(8)).astype(np.int64)
    for w in range(4):
        e["fw"][:, w] = menu[np.arange(n), (rot + w) % 8]
        e["bw"][:, w] = menu[np.arange(n), (rot + w + 4) % 8]
    e["cov"] = cov
    e["hc"] = cov > np.uint64(254)
    return e


# ---- the reference ---------------------------------------------------------------------------------------------------------
def expected(e, map_count=128, lo=0, hi=None):
    """what kq_export(lo, hi) returns for a table that holds the entries e"""
    hi = map_count if hi is None else hi
    m = e["key"] % np.uint64(map_count)
    sel = e[(m >= np.uint64(lo)) & (m < np.uint64(hi))]
    return sel[np.argsort(sel["key"], kind="stable")]


def doubled(e):
    """the table after the same entries came in twice: sums in 64 bits, clamped at 2^32 - 1"""
    out = e.copy()
    for f in ("fw", "bw", "cov"):
        out[f] = np.minimum(e[f].astype(np.uint64) * np.uint64(2), np.uint64(LARGEST))
    out["hc"] = out["cov"] > 254
    return out


def first_difference(got, want):
    """None when equal in every field, else a short description of the first difference"""
    if len(got) != len(want):
        return f"{len(got)} entries, expected {len(want)}"
    for f in ("key", "fw", "bw", "cov", "hc"):
        ne = got[f] != want[f]
        if ne.ndim > 1:
            ne = ne.any(axis=1)
        if ne.any():
            i = int(np.argmax(ne))
            return f"field {f} of entry {i}: got {got[i]}, expected {want[i]}"
    return None
