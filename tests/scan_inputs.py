"""Texts that put run ends on the edges of the sequence tile scanner (kreeq_amd/csrc/kq_device.h: tile_fetch / tile_store /
convert16 / lane_scan_core), and the reads a table is counted from to look such a text up.  Pure numpy, no GPU.

The scanner sees a device byte string through a 16-byte aligned window: the caller's pointer p becomes the aligned base
p - lead (lead = p & 15) and byte i of the text sits at WINDOW position w = lead + i.  A tile is T = 4032 consecutive k-mer
starts of the window, a lane takes 16 of them; the kernels that split two tiles per round have a second kind of seam at every
other tile edge.  Everything below is placed in window coordinates, so the same (k, lead) must be used for the text and for
the pointer that is handed to the library (tests/test_gpu_scan_edges.py: aligned tensor + 64 + lead).

edge_text(k, lead, seed) -> (text, events).  Tile edge s is window position s * T.  With rot = seed % 3 and
off(s) = (s + rot) % 3 - 1, every text has all three offsets -1, 0, +1 at an odd and at an even tile edge, twice:
  edges 1..3   a lone separator at s * T + off(s), long runs on both sides (lower-case bases around edge 2)
  edges 4..6   the separator at s * T + off(s) bounds a run of EXACTLY k bases: off -1: the run starts at s * T (its k-mer
               has no prev); off 0: it ends at s * T - 1 (no next); off +1: it has k - 1 bases before the edge and one after
  edge 7       a run of exactly k bases with one base before the edge
  edge 8       a run of k - 1 bases across the edge: no k-mer
  tile 0       runs of exactly k and of k - 1 bases that start at a lane edge (w = 0 mod 16) and that end in front of one
  tiles 1..6   two planted motifs each (see below)
Separators alternate between a newline and an N.  seed % 2 makes the first byte a separator or a base; the last run ends at
the last byte; the window length lead + len is 9 T + (0, 1, 15, 16, 17, k - 1, k)[seed % 7].

Lookup needs k-mers of the text that the table lacks, k-mers it holds whose two edges it lacks, and k-mers below a coverage
cut-off -- for k = 2 and 3 as well, where 36 000 random bases hold every k-mer many times.  So the random background of a
text never contains the k-mers of forbidden(k), and they are planted:
  motif 1   C G^k C: the k-mers C G^(k-1) and G^(k-1) C are forbidden, G^k is not.  The reads have other bases than C around G^k there, so the
            table lacks the two outer k-mers, and holds G^k without the edges C <- G^k -> C: edge-missing.
  motif 2   T A^(k-1), forbidden: of all its sites in both copies the reads keep one, so its count is 1.
edge_table_reads(text, seed, k, events): two copies of the text with those changes and ~1 % random substitutions that never
create a forbidden k-mer, then 300 copies of one repeat: a k-mer of the text that is read on the reverse strand, with its
previous base and a WRONG next base -- the k-mer, its incoming edge (counts > 254: the high-copy tier) and an outgoing
edge of count exactly 300 that the text does not follow (kq_branch_scan's cut-off, oracle/variants.py:255).

walk(k, text) is the plain restatement the tests hold the oracle against: one pass, run length + rolled words.
"""
import itertools

import numpy as np

T = 4032                            # kq_device.h TILE_STARTS
N_TILES = 9
K_EDGES = [2, 3, 15, 16, 17, 21, 24, 25, 28, 29, 31, 32]
LEADS = [0, 1, 8, 15]
ALL_LEADS_K = (21, 32)
BRANCH_K = [16, 17, 21, 31, 32]     # key spaces in which the text's k-mers are (nearly) unique: a graph with few branches
REPEAT_COPIES = 300

ACGT = b"ACGT"
CODE = [4] * 256
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = CODE[_c | 0x20] = _i


def leads_of(k):
    return list(range(16)) if k in ALL_LEADS_K else LEADS


CASES = [(k, lead) for k in K_EDGES for lead in leads_of(k)]
BRANCH_CASES = [(k, lead) for k in BRANCH_K for lead in LEADS]

# (k, lead) -> seed.  The default walks through all 42 combinations of window length, offset rotation and first byte; an
# entry here replaces a seed whose text does not have the properties tests/test_scan_inputs.py asks for.
SEED_OVERRIDE = {}


def seed_for(k, lead):
    return SEED_OVERRIDE.get((k, lead), 16 * k + lead)


def tail_of(k, seed):
    return (0, 1, 15, 16, 17, k - 1, k)[seed % 7]


def revcomp(seq: bytes):
    return seq[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def forbidden(k):
    """k-mers (upper case, both strands) that occur in a text only where edge_text plants them"""
    f = {b"C" + b"G" * (k - 1), b"G" * (k - 1) + b"C", b"T" + b"A" * (k - 1)}
    return f | {revcomp(x) for x in f}


def _hits(buf, lo, hi, k, forb):
    """number of forbidden k-mers that start in [lo, hi)"""
    lo, hi = max(lo, 0), min(hi, len(buf) - k + 1)
    return sum(bytes(buf[s:s + k]).upper() in forb for s in range(lo, hi))


def _scrub(buf, forb, rng):
    """redraw a base of every forbidden k-mer until none is left"""
    while True:
        hit = False
        for f in forb:
            i = buf.find(f)
            while i >= 0:
                hit = True
                buf[i + int(rng.integers(len(f)))] = ACGT[int(rng.integers(4))]
                i = buf.find(f, i + 1)
        if not hit:
            return


def _plant(buf, at, core, k, forb, n_forbidden):
    """core at buf[at:], between two flank bases chosen so that the k-mers around it are the n_forbidden planted ones only"""
    for left, right in itertools.product(ACGT, ACGT):
        new = bytes([left]) + core + bytes([right])
        old = bytes(buf[at - 1:at - 1 + len(new)])
        buf[at - 1:at - 1 + len(new)] = new
        if _hits(buf, at - k, at + len(core) + 1, k, forb) == n_forbidden:
            return
        buf[at - 1:at - 1 + len(new)] = old
    raise AssertionError("no flanks keep the surroundings of a planted motif clean")


def edge_text(k, lead, seed):
    """-> (text, events); events = dicts {kind, at, n, name}, `at` an index into text (window position - lead):
    sep (at), run_k / run_k1 (a run of n = k / k - 1 bases at `at`, separators on both sides), lower (n lower-case bytes),
    motif1 (at = the G^k between C and C), motif2 (at = the T A^(k-1))"""
    assert 2 <= k <= 32 and 0 <= lead < 16
    rng = np.random.default_rng([seed, k, lead])
    forb = forbidden(k)
    total = N_TILES * T + tail_of(k, seed)                   # window length
    win = bytearray(np.frombuffer(ACGT, dtype=np.uint8)[rng.integers(0, 4, total)].tobytes())     # indexed by window position
    _scrub(win, forb, rng)
    events = []

    def ev(kind, w, n, name):
        events.append({"kind": kind, "at": w - lead, "n": n, "name": name})

    # planted motifs, in the middle of tiles 1..6
    for s in range(1, 7):
        w = s * T + 500 + 37 * s
        _plant(win, w - 1, b"C" + b"G" * k + b"C", k, forb, 2)
        ev("motif1", w, k, f"C G^k C in tile {s}")
        w = s * T + 1900 + 29 * s
        _plant(win, w, b"T" + b"A" * (k - 1), k, forb, 1)
        ev("motif2", w, k, f"T A^(k-1) in tile {s}")
    n_sep = [seed // 2]

    def sep(w, name):
        win[w] = b"\nN"[n_sep[0] & 1]
        n_sep[0] += 1
        ev("sep", w, 1, name)

    def run(w, n, name):
        """a run of exactly n bases at w"""
        sep(w - 1, "in front of " + name)
        sep(w + n, "behind " + name)
        ev("run_k" if n == k else "run_k1", w, n, name)

    rot = seed % 3
    for s in range(1, 7):
        off = (s + rot) % 3 - 1
        e = s * T
        if s <= 3:
            sep(e + off, f"lone separator at {s}T{off:+d}")
        elif off == -1:
            run(e, k, f"k bases from {s}T on: no prev")
        elif off == 0:
            run(e - k, k, f"k bases up to {s}T-1: no next")
        else:
            run(e - (k - 1), k, f"k bases, k-1 of them before {s}T")
    run(7 * T - 1, k, "k bases, one of them before 7T")
    run(8 * T - max(1, (k - 1) // 2), k - 1, "k-1 bases across 8T")
    run(1600, k, "k bases from a lane edge on")
    run(2016 - k, k, "k bases up to a lane edge")
    run(2400, k - 1, "k-1 bases from a lane edge on")
    run(2816 - (k - 1), k - 1, "k-1 bases up to a lane edge")
    for w in range(2 * T - 24, 2 * T + 24):
        if CODE[win[w]] < 4:
            win[w] |= 0x20
    ev("lower", 2 * T - 24, 48, "lower case across 2T")
    text = win[lead:]
    if seed % 2:
        text[0] = ord("\n")
        events.append({"kind": "sep", "at": 0, "n": 1, "name": "first byte"})
    assert CODE[text[-1]] < 4 and len(text) < 40000
    return bytes(text), events


def _substitute(buf, i, k, forb, rng):
    """another base at i that creates no forbidden k-mer (the byte stays when there is none)"""
    old = buf[i]
    for c in rng.permutation(4).tolist():
        if c == CODE[old]:
            continue
        buf[i] = ACGT[c]
        if _hits(buf, i - k + 1, i + 1, k, forb) == 0:
            return
    buf[i] = old


def edge_table_reads(text, seed, k, events):
    """the reads a table is counted from to look `text` up (see the module docstring)"""
    rng = np.random.default_rng([seed, 77])
    forb = forbidden(k)
    codes = np.array([CODE[c] for c in text], dtype=np.uint8)
    m1 = [e["at"] for e in events if e["kind"] == "motif1"]
    m2 = [e["at"] for e in events if e["kind"] == "motif2"]
    keep = np.ones(len(text), dtype=bool)                   # bytes that random substitutions leave alone
    for at in m1 + m2:
        keep[max(0, at - k - 2):at + 2 * k + 2] = False
    # the repeat: a k-mer read on the reverse strand, away from everything placed, bases on both sides
    rec = {r[0]: r for r in walk(k, text)}
    for q in rng.permutation(np.arange(k + 2, len(text) - 2 * k - 2)).tolist():
        r = rec.get(q)
        if r is not None and not r[2] and r[3] < 4 and r[4] < 4 and keep[q - k - 2:q + 2 * k + 2].all():
            wrong = [c for c in rng.permutation(4).tolist() if c != r[4] and
                     (text[q + 1:q + k].upper() + bytes([ACGT[c]])) not in forb]
            if wrong:
                break
    else:
        raise AssertionError("no reverse-strand k-mer for the repeat")
    repeat = text[q - 1:q + k].upper() + bytes([ACGT[wrong[0]]])
    keep[q - k - 2:q + 2 * k + 2] = False
    copies = []
    for c in range(2):
        buf = bytearray(text)
        for at in m1:                                       # other bases than C around G^k
            _substitute(buf, at - 1, k, forb, rng)
            _substitute(buf, at + k, k, forb, rng)
            assert _hits(buf, at - k, at + k + 1, k, forb) == 0
        for j, at in enumerate(m2):
            if (c, j) != (0, 0):
                _substitute(buf, at, k, forb, rng)
                assert _hits(buf, at - k, at + k + 1, k, forb) == 0
        for i in np.flatnonzero((rng.random(len(text)) < 0.01) & keep & (codes < 4)).tolist():
            _substitute(buf, i, k, forb, rng)
        copies.append(bytes(buf))
    return b"\n".join(copies + [repeat] * REPEAT_COPIES)


def edge_byte(is_fw, prev, nxt):
    """reference edge byte (bit 7 - e; e 0..3 = fw[ACGT], 4..7 = bw[ACGT] of the canonical k-mer) from the neighbours in
    sequence order, 4 = none"""
    b = 0
    if is_fw:
        if nxt < 4:
            b |= 1 << (7 - nxt)
        if prev < 4:
            b |= 1 << (7 - (4 + prev))
    else:
        if prev < 4:
            b |= 1 << (7 - (3 - prev))
        if nxt < 4:
            b |= 1 << (7 - (4 + 3 - nxt))
    return b


def walk(k, text):
    """every k-mer of `text` in sequence order: [(start, canonical key, is_fw, prev, next)] -- prev / next = the neighbouring
    base codes, 4 where the run ends.  Keys as in oracle/kreeq_oracle.c kqo_hash: first base in the low bits, canonical =
    min(forward, reverse complement), a palindrome counts as not forward."""
    codes = [CODE[c] for c in text]
    n, mask, top = len(codes), (1 << (2 * k)) - 1, 2 * k - 2
    out, run, fw, rv = [], 0, 0, 0
    for i, c in enumerate(codes):
        if c == 4:
            run = fw = rv = 0
            continue
        run += 1
        fw = (fw >> 2) | (c << top)
        rv = ((rv << 2) | (3 - c)) & mask
        if run >= k:
            s = i - k + 1
            prev = codes[s - 1] if run > k else 4
            nxt = codes[i + 1] if i + 1 < n else 4
            out.append((s, min(fw, rv), fw < rv, prev, nxt))
    return out


def walk_records(k, text):
    """walk() as the (keys, edge bytes) arrays of oracle.emit_records"""
    w = walk(k, text)
    return (np.array([r[1] for r in w], dtype=np.uint64),
            np.array([edge_byte(r[2], r[3], r[4]) for r in w], dtype=np.uint8))


# ---------------------------------------------------------------------------------- the oracle's view, once per (k, lead)
MAP = 128
RANGES = ((0, 128), (0, 64), (64, 128))
CUTOFFS = (0, 3)
BRANCH_CUTOFFS = (0, 2, 300)
_REFERENCES = {}


def reference(k, lead):
    """text, events and reads of (k, lead) with everything the CPU oracle says about them:
    keys / edges (emit_records of the text), export / summary (the text counted), table (export of the reads counted),
    validate[(lo, hi, cutoff)] = (counters, per-base array) of the text looked up in that table"""
    import types

    from oracle import oracle as O

    if (k, lead) in _REFERENCES:
        return _REFERENCES[(k, lead)]
    seed = seed_for(k, lead)
    r = types.SimpleNamespace(k=k, lead=lead, seed=seed)
    r.text, r.events = edge_text(k, lead, seed)
    r.reads = edge_table_reads(r.text, seed, k, r.events)
    r.keys, r.edges = O.emit_records(k, r.text)
    cpu = O.OracleDB(k, MAP)
    cpu.count_batch(r.text)
    r.export, r.summary = cpu.export(), cpu.summary(with_hist=True)
    cpu.close()
    cpu = O.OracleDB(k, MAP)
    cpu.count_batch(r.reads, threads=4)
    r.table = cpu.export()
    r.validate = {(lo, hi, cut): cpu.validate_sequence(r.text, cov_cutoff=cut, map_lo=lo, map_hi=hi, per_base=True)
                  for lo, hi in RANGES for cut in CUTOFFS}
    cpu.close()
    _REFERENCES[(k, lead)] = r
    return r
