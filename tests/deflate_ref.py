"""The LZ77 parse of k_bgzf_deflate (kreeq_amd/csrc/kq_deflate.h) restated as plain serial code from that file's header comment:
the tokens of ONE member (<= 0xff00 bytes of text) are a function of the text alone, and this module says which.

The text is walked in steps of 64 positions.  Within a step every position is measured against the hash table as the EARLIER
steps left it (or, failing that, against the lowest position of its own step with the same hash), then the whole step is
inserted (the highest position wins a slot), then the step is parsed greedily from the first position no earlier match covers.
A token is (literal,) or (length, distance)."""
import functools

import numpy as np

MEMBER = 0xff00
STEP = 64
MIN_MATCH, MAX_MATCH, WINDOW = 3, 258, 32768
QUICK = 32                      # a measured length of QUICK means "QUICK or more": the parse measures the rest of a match it takes
TOO_FAR = 4096                  # a 3-byte match further back costs more than 3 literals
HASH_BITS = 12


def hashes(text):
    """the 12-bit hash of the 3 bytes at every position p with p + 3 <= n"""
    t = np.frombuffer(text, dtype=np.uint8).astype(np.uint64)
    if len(t) < 3:
        return []
    w = t[:-2] | t[1:-1] << np.uint64(8) | t[2:] << np.uint64(16)
    return ((w * np.uint64(0x9E3779B1) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)).tolist()


def common(text, a, b, cap):
    """how many of the `cap` bytes at a and at b are equal from the front (a < b, b + cap <= n)"""
    x = int.from_bytes(text[a:a + cap], "little") ^ int.from_bytes(text[b:b + cap], "little")
    return cap if x == 0 else ((x & -x).bit_length() - 1) >> 3


def measure(text, n, p, cand):
    """the match of p against the earlier position cand as a step sees it: (quick length, distance) or None"""
    length = common(text, cand, p, min(QUICK, n - p))
    if length < MIN_MATCH or (length == MIN_MATCH and p - cand > TOO_FAR):
        return None
    return length, p - cand


def parse_steps(text):
    """the tokens of one member with the text position each starts at: [(position, token)]"""
    text = bytes(text)
    n = len(text)
    assert n <= MEMBER
    h = hashes(text)
    table = {}                                                      # slot -> position, as the steps so far left it
    out = []
    covered = 0                                                     # positions below it lie inside a match already taken
    for base in range(0, n, STEP):
        last = min(base + STEP, n)                                  # the step's positions are base .. last - 1
        can = range(base, min(last, max(n - 2, base)))              # those with three bytes left
        found = {}
        if covered < last:
            lowest = {}
            for p in can:
                lowest.setdefault(h[p], p)
            for p in can:
                if p < covered:
                    continue
                m = None
                cand = table.get(h[p])
                if cand is not None and p - cand <= WINDOW:
                    m = measure(text, n, p, cand)
                if m is None and lowest[h[p]] < p:                 # nothing older: the start of a run inside the step
                    m = measure(text, n, p, lowest[h[p]])
                if m is not None:
                    found[p] = m
        for p in can:                                               # ascending: the highest position of the step wins its slot
            table[h[p]] = p
        p = max(covered, base)
        while p < last:
            if p not in found:
                out.append((p, (text[p],)))
                p += 1
                continue
            length, dist = found[p]
            cap = min(MAX_MATCH, n - p)
            if length == QUICK and cap > QUICK:
                length = QUICK + common(text, p - dist + QUICK, p + QUICK, cap - QUICK)
            out.append((p, (length, dist)))
            p += length
        covered = max(covered, p)
    return out


@functools.lru_cache(maxsize=None)
def _parse_cached(text):
    return tuple(parse_steps(text))


def parse_at(text):
    """parse_steps, cached per text"""
    return list(_parse_cached(bytes(text)))


def parse(text):
    """the tokens of one member"""
    return [t for _, t in parse_at(text)]


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if len(t) == 1:
            out.append(t[0])
        else:
            length, dist = t
            assert 1 <= dist <= len(out), "a distance of %d after %d bytes" % (dist, len(out))
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)


def check_tokens(text, tokens):
    """the tokens are DEFLATE's, the parse's own rule holds, and they spell the text"""
    for t in tokens:
        if len(t) == 1:
            assert 0 <= t[0] <= 255
            continue
        length, dist = t
        assert MIN_MATCH <= length <= MAX_MATCH, t
        assert 1 <= dist <= WINDOW, t
        assert not (length == MIN_MATCH and dist > TOO_FAR), t
    assert expand(tokens) == bytes(text)


def members(text):
    """the member texts of a whole text"""
    return [text[i:i + MEMBER] for i in range(0, len(text), MEMBER)]


def first_difference(text, want, got):
    """where two token lists for `text` part ways: a line for an assertion message, or None"""
    pos = 0
    for i, (a, b) in enumerate(zip(want, got)):
        if a != b:
            return "token %d at text position %d: restated %r, device %r" % (i, pos, a, b)
        pos += 1 if len(a) == 1 else a[0]
    if len(want) != len(got):
        return "token %d at text position %d: %d tokens restated, %d on the device" % (min(len(want), len(got)), pos, len(want), len(got))
    return None
