"""Inputs of the subgraph tests at every k (tests/test_subgraph_inputs.py on the CPU, tests/test_gpu_subgraph_kmatrix.py and
tests/test_gpu_subgraph_seed_edges.py on the GPU) -- TEST INFRASTRUCTURE ONLY.  Pure numpy, no GPU.

graph_case(k), 2 <= k <= 32 -> a namespace with
  reads    the batch the database is counted from
  batch    the seed batch (segments separated by N / n / newline)
  cutoff   a coverage cutoff between the planted counts (see below)
  hot      the high-copy k-mer that only an expansion reaches (ACGT bytes)
  w, w2    k >= 8: the k-mers of the two reverse-complement repeats, absent from the reads
  pal      even k >= 8: the palindrome planted inside the seed

k >= 8: a random genome of 400 bases read at ~35x, and planted on it or next to it
  bubble   a second haplotype with one SNP; a seed stretch ends 2 k-mers before the bubble opens
  gap      two seed stretches of the genome with k // 2 k-mers between them, which a best-first search of depth k joins
  cycle    a tandem repeat of ceil((k + 8) / 7) + 4 units of 7 bases between two pieces of the genome; the seed holds
           ceil((k + 8) / 7) units, so it has k-mers inside the cycle at every k
  hot      helpers.hot_kmer_reads: 320 copies of one k-mer; the seed holds the k-mers one step before and one step behind
           it, so it comes in by expansion (traversal depth 1, best-first at cutoff 0) with cov >= 255
  century  a stretch read exactly CENTURY = 100 times.  30 + k bases of it, from its 6th base on, are three segments of the
           seed (database cov <= 254, subgraph cov 300: packed adds, then the add that crosses 254); k // 2 k-mers further
           on a fourth segment follows, so a best-first search joins the two at every cutoff < 100, and the stretch goes on
           behind it: an edge of count 100 leaves the subgraph.  The 5 k-mers in front of the three segments lead nowhere:
           no best-first search adds them, and the trim behind it clears a counter of 300 -- 200 in the 8-bit lane, 100 in
           the high-copy entry.  cutoff = CENTURY - 1: above every count of the genome, below this one
  branch   a core read 4 times whose 10th k-mer has three other next bases read 1, 2 and 3 times, each with 6 more
           bases behind it, and which goes on behind the seed: edges of count 1, 2, 3 and 4 leave the seed, and after an
           expansion of depth d the k-mers d steps down the branches have them
  rc       a segment A w C ... G rc(w) T: the second occurrence of w's k-mer is on the other strand.  G rc(w) T is the
           reverse complement of A w C, so both occurrences construct the same edges; the segment C w2 A ... C rc(w2) A
           next to it has a second occurrence on the other strand whose edges differ, and the first one decides
  pal      A pal C in the reads (helpers.plant_palindromes) and in the seed

k < 8: helpers.de_bruijn_linear(k), the whole key space, with three parts of it read more often (CENTURY, 320 and 1..4
times) and short seed pieces, one of them three times; SMALL_K lists the pieces.  Which facts hold there is what
tests/test_subgraph_inputs.py asserts from the restatement.
"""
import types

import numpy as np

from tests import helpers as H

CENTURY = 100
UNIT = b"ACGGTCA"
SNP = 230
_CASES = {}


def rand_bases(rng, n):
    return H.ACGT[rng.integers(0, 4, n)].tobytes()


def _absent(rng, n, text):
    """n random bases that occur in `text` on neither strand"""
    while True:
        w = rand_bases(rng, n)
        if w not in text and H.revcomp_bases(w) not in text and w != H.revcomp_bases(w):
            return w


def _large_case(k):
    rng = np.random.default_rng([k, 20])
    reads, genome = H.synth_reads(150, 100, 400, seed=500 + k, err=0.0)
    reads = [reads.upper()]
    # bubble
    s = SNP
    alt = genome[:s] + bytes([H.ACGT[(list(b"ACGT").index(genome[s]) + 1) & 3]]) + genome[s + 1:]
    reads += [alt[i:i + 2 * k + 20] for i in range(s - k - 19, s - k + 1, 3)]
    segs = [genome[s - 2 - k - 30:s - 2]]
    # gap: k-mer starts 20..30 and 31 + g..36 + g
    g = k // 2
    segs += [genome[20:30 + k], genome[31 + g:36 + g + k]]
    # cycle
    m = -(-(k + 8) // 7)
    rep = genome[320:350] + UNIT * (m + 4) + genome[350:380]
    reads += [rep[i:i + 2 * k + 30] for i in range(0, max(1, len(rep) - 2 * k - 29), 2)]
    segs.append(UNIT * m)
    # hot
    hot, hot_reads = H.hot_kmer_reads(k, seed=700 + k)
    reads += hot_reads
    segs += [hot_reads[0][:k], hot_reads[0][2:]]
    # century
    cen = rand_bases(rng, 35 + k + g + 6 + k + 10)
    reads += [cen] * CENTURY
    segs += [cen[5:35 + k]] * 3 + [cen[36 + g:41 + g + k]]
    # branch
    core = rand_bases(rng, k + 45)
    reads += [core] * 4
    for copies, b in zip((1, 2, 3), [b for b in b"ACGT" if b != core[9 + k]]):
        reads += [core[5:9 + k] + bytes([b]) + rand_bases(rng, 6)] * copies
    segs.append(core[:k + 19])
    # palindrome
    pal = None
    if k % 2 == 0:
        pal = H.palindromes(k, 1, seed=k)[0]
        reads += H.plant_palindromes(k, [pal], seed=k, hot_copies=3)
        segs.append(b"A" + pal + b"C")
    # the reverse-complement repeat, of bases the reads do not have
    text = b"\n".join(reads).upper()
    w = _absent(rng, k, text)
    segs.append(b"A" + w + b"C" + _absent(rng, 7, b"") + b"G" + H.revcomp_bases(w) + b"T")
    w2 = _absent(rng, k, text + b"\n" + segs[-1])
    segs.append(b"C" + w2 + b"A" + _absent(rng, 7, b"") + b"C" + H.revcomp_bases(w2) + b"A")
    seps = [b"N", b"n", b"\n", b"NN"]
    batch = b"".join(seg + seps[i % 4] for i, seg in enumerate(segs)) + segs[0][:k - 1].lower()      # ends with k - 1 bases: no k-mer
    return types.SimpleNamespace(k=k, reads=b"\n".join(reads), batch=batch, cutoff=CENTURY - 1, hot=hot, w=w, w2=w2, pal=pal)


# k < 8, positions in the de Bruijn text: `absent` = the k-mer the reads lack (on both strands), `hot` = the one read 320 more
# times, `century` = the [a, b) read CENTURY - 1 more times, `seed` = the [a, b) of the seed batch.  k = 2 and 3 are laid out by
# hand so that the properties of tests/test_subgraph_inputs.py hold in the restatement.
def _small_layout(k, dh=0):
    n, g = 4 ** k + k - 1, k // 2
    h, x = n // 2 + dh, n // 3
    return {"absent": x, "hot": h, "century": [(0, 40)], "half": 3,
            "seed": [(0, 12 + k)] * 3 + [(13 + g, 16 + g + k), (h - 1, h - 1 + k), (h + 1, h + 1 + k), (x - 3, x + k + 3)]}


SMALL_K = {
    2: {"absent": 0, "hot": 7, "century": [(10, 17)], "seed": [(10, 12)] * 3 + [(15, 17), (13, 17), (2, 5), (1, 6)]},
    3: {"absent": 60, "hot": 41, "century": [(0, 12)], "seed": [(0, 5)] * 3 + [(6, 11), (43, 47), (45, 49), (8, 13)]},
    4: _small_layout(4, dh=9),                               # (the k-mer in the middle of B(4, 4) is in the seed's first piece)
    5: _small_layout(5), 6: _small_layout(6), 7: _small_layout(7),
}


def _without(read, kmers, k):
    """the pieces of `read` that hold every k-mer of it but those of `kmers`"""
    out, prev = [], 0
    for i in range(len(read) - k + 1):
        if read[i:i + k] in kmers:
            out.append(read[prev:i + k - 1])
            prev = i + 1
    out.append(read[prev:])
    return [p for p in out if len(p) >= k]


def _small_case(k):
    text = H.de_bruijn_linear(k)
    p = SMALL_K[k]
    w = text[p["absent"]:p["absent"] + k]
    assert w != H.revcomp_bases(w)
    hot = text[p["hot"]:p["hot"] + k]
    reads = [text] + [text[len(text) // 2:]] * p.get("half", 0)         # counters of 1 and 2, and larger ones in the second half
    reads += [text[a:b] for a, b in p["century"]] * (CENTURY - 1)       # CENTURY with the text (+ the other strand's occurrences)
    reads += [text[p["hot"] - 1:p["hot"] + k + 1]] * 320
    reads = [piece for r in reads for piece in _without(r, (w, H.revcomp_bases(w)), k)]
    segs = [text[a:b] for a, b in p["seed"]]
    seps = [b"N", b"n", b"\n", b"NN"]
    batch = b"".join((seg.lower() if i == 1 else seg) + seps[i % 4] for i, seg in enumerate(segs))[:-1]
    return types.SimpleNamespace(k=k, reads=b"\n".join(reads), batch=batch, cutoff=CENTURY - 1, hot=hot, w=w, w2=None, pal=None)


def graph_case(k):
    assert 2 <= k <= 32
    if k not in _CASES:
        _CASES[k] = _small_case(k) if k < 8 else _large_case(k)
    return _CASES[k]


def key_of(kmer):
    """canonical key of a k-mer given as ACGT bytes"""
    k = len(kmer)
    return int(H.canonical_keys_of([H.key_of_codes([b"ACGT".index(x) for x in kmer.upper()])], k)[0])


def constructed(prev, kmer, nxt):
    """the entry a k-mer absent from the database gets from its occurrence prev + kmer + nxt (one base each, or b"" where the
    segment ends), on strings: read the three on the strand on which the k-mer is canonical (keys order k-mers by their
    reversed strings, and a palindrome counts as the other strand); the base behind the k-mer is its forward edge, the base
    in front of it its backward edge -> (key, fw, bw)"""
    if not kmer[::-1] < H.revcomp_bases(kmer)[::-1]:
        prev, kmer, nxt = H.revcomp_bases(nxt), H.revcomp_bases(kmer), H.revcomp_bases(prev)
    f, b = [0] * 4, [0] * 4
    if nxt:
        f[b"ACGT".index(nxt)] = 1
    if prev:
        b[b"ACGT".index(prev)] = 1
    return H.key_of_codes([b"ACGT".index(x) for x in kmer]), f, b


# ------------------------------------------------------------------------------------------------------------- saturation
LARGEST = 2 ** 32 - 1
NEAR = LARGEST - 5


def saturation_case(k):
    """counters that saturate at 2^32 - 1 when the seed sums them.  S = P X Q with 8 random bases P and Q around a k-mer X; the
    reads hold every k-mer of S but X (P X[:-1] and X[1:] Q, twice each), a third neighbour of X (X[1:] c Q2, twice) and a
    background.  `entry` = what kq_import adds for X: cov and the two counters along S at NEAR = 2^32 - 6, the counter towards c
    at 7.  The seed batch holds X in two segments (NEAR + NEAR saturates; 7 + 7 does not) and the two ends of S and the end of
    the branch, 6 k-mers away from X each.  -> namespace(reads, entry, batch, key, along = the two (fw?, base) edges along S)"""
    from tests import subgraph_ref as R

    rng = np.random.default_rng([k, 32])
    bg, _ = H.synth_reads(100, 100, 500, seed=900 + k, err=0.0)
    p, q, q2 = rand_bases(rng, 8), rand_bases(rng, 8), rand_bases(rng, 8)
    x = _absent(rng, k, bg.upper())
    c = bytes([next(b for b in b"ACGT" if b != q[0])])
    s, s2 = p + x + q, x[1:] + c + q2
    reads = [bg.upper()] + [p + x[:-1]] * 2 + [x[1:] + q] * 2 + [s2] * 2
    key = key_of(x)
    fw, bw = [0] * 4, [0] * 4
    along = []
    for nb, count in ((x[1:] + q[:1], NEAR), (p[-1:] + x[:-1], NEAR), (x[1:] + c, 7)):
        hits = [(f, i) for f in (True, False) for i in range(4) if R.next_key(key, i, f, k)[0] == key_of(nb)]
        assert len(hits) == 1
        (fw if hits[0][0] else bw)[hits[0][1]] = count
        if count == NEAR:
            along.append(hits[0])
    batch = b"N".join([x, x.lower(), s[:k + 1], s[15:], s2[7:]])
    return types.SimpleNamespace(k=k, reads=b"\n".join(reads), entry=(key, fw, bw, NEAR), batch=batch, key=key, along=along)


# ------------------------------------------------------------------------------- a repeat across a tile edge of the scanner
TILE = 4032                         # kq_device.h TILE_STARTS (tests/scan_inputs.py: T)
PERIOD = 20


def tile_repeat_text(k, lead):
    """-> (text, plants): one segment of 3 tiles in which, at the tile edges 1 and 2 of the scanner's window (window position =
    lead + index, tests/scan_inputs.py), a k-mer w of period PERIOD < k starts 10 positions before the edge -- in the last lane
    of the tile -- and again PERIOD positions later -- in the first lane of the next one.  The two occurrences overlap; the first
    has the bases a in front and w[k - PERIOD] behind it, the second w[PERIOD - 1] and b, with a != w[PERIOD - 1] and
    b != w[k - PERIOD].  plants = [(w, a, b, index of the first occurrence)]"""
    assert k > PERIOD and 0 <= lead < 16
    rng = np.random.default_rng([k, lead, 4032])
    win = bytearray(rand_bases(rng, 3 * TILE))
    plants = []
    for s in (1, 2):
        while True:
            unit = rand_bases(rng, PERIOD)
            w = (unit * 3)[:k]
            if all(unit[i:] + unit[:i] != unit for i in range(1, PERIOD)) and w != H.revcomp_bases(w):
                break
        a = bytes([next(x for x in b"ACGT" if x != w[PERIOD - 1])])
        b = bytes([next(x for x in b"TGCA" if x != w[k - PERIOD])])
        at = s * TILE - 10
        stretch = a + (unit * 4)[:PERIOD + k] + b
        win[at - 1:at - 1 + len(stretch)] = stretch
        plants.append((w, a, b, at - lead))
    text = bytes(win[lead:])
    for w, _, _, at in plants:                                          # exactly the two occurrences, on this strand only
        assert [i for i in range(len(text) - k + 1) if text[i:i + k] == w] == [at, at + PERIOD] and H.revcomp_bases(w) not in text
    return text, plants


def copy_of(table):
    return {key: (list(v[0]), list(v[1]), v[2]) for key, v in table.items()}


def outside_counters(sub, k):
    """the non-zero edge counters of `sub` whose neighbour is not in it, sorted"""
    from tests import subgraph_ref as R

    return sorted(c for key, (f, b, _) in sub.items() for fw, cs in ((True, f), (False, b)) for i, c in enumerate(cs)
                  if c and R.next_key(key, i, fw, k)[0] not in sub)


def crossed_and_trimmed(table, before, after):
    """the k-mers of the low tier of the database (cov <= 254) whose sums took them across 254 in the subgraph `before` and
    of which the trim that gave `after` cleared a counter: the 8-bit lane and the high-copy counter go together"""
    return [key for key, v in before.items() if key in table and table[key][2] <= 254 < v[2] and (v[0], v[1]) != (after[key][0], after[key][1])]


def n_counters(sub):
    return sum(c != 0 for f, b, _ in sub.values() for c in f + b)
