"""Table geometry restated in numpy, and inputs that crowd chosen table regions (tests/test_gpu_regions.py).

The k-mer table is n_regions regions of 2048 slots (kreeq_amd/csrc/kq_device.h).  A canonical key's TABLE HASH is an
invertible mix of its 2k bits, left-aligned in 64 bits: a three-round Feistel network on the two k-bit halves for k <= 24,
xorshift-multiply-xorshift above.  Its region is mulhi(top 32 hash bits, n_regions); inside the region the key is probed
linearly from its HOME QUAD, the low 11 bits of the 2k-bit hash value rounded down to a multiple of four.  Because the
hash is a bijection, keys are made for a region by choosing hash values there and inverting them.  Everything here is
written from that description, independently of the library's own code: the GPU tests pin it to the device (the hash
bits of packed records, and a region that takes exactly 2048 keys and not one more)."""
import numpy as np

REGION_SLOTS = 2048
QUAD_MASK = REGION_SLOTS - 4
FEISTEL_MAX_K = 24
FEI_C = (0x9E3779, 0x85EBCB, 0xC2B2AF)
MIX_MUL = 0x9E3779B97F4A7C15
MIX_INV = pow(MIX_MUL, -1, 1 << 64)
U64 = np.uint64
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _fei(r, c, k):
    """round function: bits 8 .. 8+k-1 of the low 32 bits of the 24 x 24-bit product r * c"""
    return (((r * U64(c)) & U64(0xFFFFFFFF)) >> U64(8)) & U64((1 << k) - 1)


def table_hash(keys, k):
    """left-aligned 64-bit table hash of canonical keys (any shape)"""
    keys = np.asarray(keys, dtype=U64)
    pad = U64(64 - 2 * k)
    if k <= FEISTEL_MAX_K:
        m = U64((1 << k) - 1)
        l, r = keys & m, keys >> U64(k)
        for c in FEI_C:                                   # (l, r) -> (r, l ^ F(r))
            l, r = r, l ^ _fei(r, c, k)
        return ((l << U64(k)) | r) << pad
    with np.errstate(over="ignore"):
        x = keys ^ (keys >> U64(k))
        x = (x * U64(MIX_MUL)) << pad
    return x ^ ((x >> U64(k)) & U64(((1 << 64) - 1) ^ ((1 << (64 - 2 * k)) - 1)))


def key_of_hash(h, k):
    """inverse of table_hash"""
    h = np.asarray(h, dtype=U64)
    pad = U64(64 - 2 * k)
    if k <= FEISTEL_MAX_K:
        m = U64((1 << k) - 1)
        x = h >> pad
        l, r = x >> U64(k), x & m
        for c in reversed(FEI_C):                         # undo (l, r) -> (r, l ^ F(r))
            l, r = r ^ _fei(l, c, k), l
        return (r << U64(k)) | l                          # the key's low half is l, as in table_hash
    top = U64(((1 << 64) - 1) ^ ((1 << (64 - 2 * k)) - 1))
    with np.errstate(over="ignore"):
        x = (h ^ ((h >> U64(k)) & top)) >> pad           # the xorshift by >= half the width is its own inverse
        x = ((x * U64(MIX_INV)) << pad) >> pad
    return x ^ (x >> U64(k))


def hash_region(h, n_regions):
    return ((np.asarray(h, dtype=U64) >> U64(32)) * U64(n_regions)) >> U64(32)


def hash_offset(h, k):
    """first slot of the home quad inside the region"""
    return ((np.asarray(h, dtype=U64) >> U64(64 - 2 * k)) & U64(QUAD_MASK)).astype(np.int64)


def revcomp_keys(keys, k):
    x = ~np.asarray(keys, dtype=U64)
    x = ((x >> U64(2)) & U64(0x3333333333333333)) | ((x & U64(0x3333333333333333)) << U64(2))
    x = ((x >> U64(4)) & U64(0x0F0F0F0F0F0F0F0F)) | ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4))
    return x.byteswap() >> U64(64 - 2 * k)


def canonical(keys, k):
    keys = np.asarray(keys, dtype=U64)
    return np.minimum(keys, revcomp_keys(keys, k))


def is_canonical(keys, k):
    keys = np.asarray(keys, dtype=U64)
    return keys <= revcomp_keys(keys, k)


def region_of_keys(keys, k, n_regions):
    return hash_region(table_hash(keys, k), n_regions).astype(np.int64)


def home_of_keys(keys, k):
    return hash_offset(table_hash(keys, k), k)


def value_range(region, n_regions, k):
    """[lo, hi): the 2k-bit hash values (the hash shifted right by 64 - 2k) that fall into `region`"""
    a = -(-(region << 32) // n_regions)                   # ceil(r 2^32 / n): first top-32 value of the region
    b = -(-((region + 1) << 32) // n_regions)
    if 2 * k >= 32:
        return a << (2 * k - 32), b << (2 * k - 32)
    s = 32 - 2 * k
    return -(-a >> s), -(-b >> s)


def region_capacity(region, n_regions, k):
    """(canonical keys of `region`, of which in each home quad: dict quad -> count) -- exhaustive, for small key spaces"""
    keys = all_region_keys(region, n_regions, k)
    homes = home_of_keys(keys, k)
    return len(keys), dict(zip(*np.unique(homes, return_counts=True)))


ENUM_MAX = 1 << 23


def all_region_keys(region, n_regions, k):
    """every canonical key of `region`, sorted (small key spaces: the region's hash values are enumerated)"""
    lo, hi = value_range(region, n_regions, k)
    assert hi - lo <= ENUM_MAX, "key space too large to enumerate"
    v = np.arange(lo, hi, dtype=U64)
    keys = key_of_hash(v << U64(64 - 2 * k), k)
    return np.sort(keys[is_canonical(keys, k)])


def region_keys(region, n_regions, k, n, rng, home=None, exclude=()):
    """n distinct canonical keys of `region` (fewer when the region or the home quad has fewer), optionally all with the
    home quad `home` (a multiple of four); keys in `exclude` are not chosen.  Enumerated where the region holds few hash
    values, sampled through key_of_hash elsewhere."""
    lo, hi = value_range(region, n_regions, k)
    pad = U64(64 - 2 * k)
    excl = np.asarray(exclude, dtype=U64)
    if hi - lo <= ENUM_MAX:
        v = np.arange(lo, hi, dtype=U64)
        if home is not None:
            v = v[((v & U64(QUAD_MASK)) == U64(home))]
        keys = key_of_hash(v << pad, k)
        keys = keys[is_canonical(keys, k) & ~np.isin(keys, excl)]
        return np.sort(rng.permutation(keys)[:n])
    got = np.zeros(0, dtype=U64)
    for _ in range(200):
        v = rng.integers(lo, hi - 1, 4 * n + 64, dtype=U64, endpoint=True)
        if home is not None:
            v = (v & ~U64(QUAD_MASK)) | U64(home)
            v = v[(v >= U64(lo)) & (v <= U64(hi - 1))]
        keys = key_of_hash(v << pad, k)
        keys = keys[is_canonical(keys, k) & ~np.isin(keys, excl)]
        got = np.unique(np.concatenate([got, keys]))
        if len(got) >= n:
            return np.sort(rng.permutation(got)[:n])
    raise AssertionError(f"could not sample {n} keys of region {region} (home {home})")


def full_region_keys(region, n_regions, k, rng, layout, n=REGION_SLOTS):
    """n keys of `region` laid out as `layout`:
       'quad'  : as many as the region has with one home quad (all n where the key space allows), the rest random
       'wrap'  : likewise with the last home quad (2044): their probe chains run past slot 2047 and wrap to slot 0
       'random': random homes
    -> (keys, number that share the chosen home quad)"""
    if layout == "random":
        return region_keys(region, n_regions, k, n, rng), 0
    home = QUAD_MASK if layout == "wrap" else int(rng.integers(0, REGION_SLOTS // 4)) * 4
    same = region_keys(region, n_regions, k, n, rng, home=home)
    rest = region_keys(region, n_regions, k, n - len(same), rng, exclude=same) if len(same) < n else np.zeros(0, dtype=U64)
    return np.sort(np.concatenate([same, rest])), len(same)


# ---------------------------------------------------------------------------------- keys -> reads
def key_codes(keys, k):
    """base codes of packed keys, first base in the low bits: (n, k) uint8"""
    keys = np.asarray(keys, dtype=U64)
    return ((keys[:, None] >> (U64(2) * np.arange(k, dtype=U64))[None, :]) & U64(3)).astype(np.uint8)


def neighbour_keys(keys, k):
    """canonical keys of the k-mers a one-base flank adds: (prev[n, 4], next[n, 4]) for the flank bases A, C, G, T"""
    keys = np.asarray(keys, dtype=U64)
    mask = U64((1 << (2 * k)) - 1) if k < 32 else ~U64(0)
    b = np.arange(4, dtype=U64)[None, :]
    prev = ((keys[:, None] << U64(2)) & mask) | b                           # base b, then the first k - 1 bases of the key
    nxt = (keys[:, None] >> U64(2)) | (b << U64(2 * k - 2))                 # the last k - 1 bases, then base b
    return canonical(prev, k), canonical(nxt, k)


def keys_to_reads(keys, copies, k, rng, n_regions=None, avoid=()):
    """one short read per copy of each key: [prev base] key [next base], on a random strand.  Over the copies of a key the
    flanks cycle through A, C, G, T and none (a read end), each side with its own phase, so every edge lane and the missing
    neighbour both occur.  A flank whose neighbouring k-mer would land in a region of `avoid` is not used (the key's copies
    then cycle through the remaining flanks), so that the designed occupancy of those regions is exact.
    -> bytes, reads separated by newlines"""
    keys = np.asarray(keys, dtype=U64)
    copies = np.asarray(copies, dtype=np.int64)
    n = len(keys)
    ok_prev = np.ones((n, 4), dtype=bool)
    ok_next = np.ones((n, 4), dtype=bool)
    if len(avoid):
        p, q = neighbour_keys(keys, k)
        av = np.asarray(list(avoid), dtype=np.int64)
        ok_prev = ~np.isin(region_of_keys(p, k, n_regions), av)
        ok_next = ~np.isin(region_of_keys(q, k, n_regions), av)
    # choice lists per key: the allowed bases, then 4 = none; copy j takes entry (j + phase) % len
    idx = np.repeat(np.arange(n), copies)
    j = np.arange(len(idx)) - np.repeat(np.cumsum(copies) - copies, copies)

    def pick(ok, phase):
        opts = np.sort(np.where(ok, np.arange(4)[None, :], 9), axis=1)     # the allowed bases first
        opts = np.concatenate([opts, np.full((n, 1), 9)], axis=1)
        n_ok = ok.sum(axis=1)
        opts[np.arange(n), n_ok] = 4                                        # then none, which is always allowed
        return opts[idx, (j + phase[idx]) % (n_ok[idx] + 1)]

    phase = rng.integers(0, 5, (2, n))
    pb = pick(ok_prev, phase[0])
    nb = pick(ok_next, phase[1])
    codes = key_codes(keys, k)[idx]
    rows = np.full((len(idx), k + 3), ord("\n"), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT\n", dtype=np.uint8)
    rows[:, 0] = lut[pb]
    rows[:, 1:k + 1] = ACGT[codes]
    rows[:, k + 1] = lut[nb]
    rev = rng.random(len(idx)) < 0.5
    comp = np.arange(256, dtype=np.uint8)
    for a, c in (b"AT", b"TA", b"CG", b"GC"):
        comp[a] = c
    rows[rev, :k + 2] = comp[rows[rev, :k + 2][:, ::-1]]
    rows = rows[rng.permutation(len(rows))]
    return rows.tobytes()[:-1]


def region_occupancy(O, batches, k, n_regions):
    """distinct canonical keys per region over every k-mer of the batches (the oracle's k-mer walk): int64[n_regions]"""
    keys = np.unique(np.concatenate([O.emit_records(k, b)[0] for b in batches] + [np.zeros(0, dtype=U64)]))
    return np.bincount(region_of_keys(keys, k, n_regions), minlength=n_regions)
