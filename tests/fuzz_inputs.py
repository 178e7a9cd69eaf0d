"""Inputs of the differential fuzz chain (tests/test_gpu_fuzz_chain.py) and everything it expects, from the oracle and the
restatements alone -- TEST INFRASTRUCTURE ONLY.  tests/test_fuzz_inputs.py holds both to the design below, without a GPU.

case(seed) is a pure function of the seed (np.random.default_rng): k, reads, asm and the parameters of every stage.
  k         2 + seed % 31: every k from 2 to 32 four times over the 124 seeds
  genome    150-400 bases (k + 3 in the short case) of one low- or full-complexity alphabet; about every second one with a tandem
            repeat of period 1-11 over 60 bases; about every second one at even k with a planted palindromic k-mer
  reads     fragments of 40, 70 or 100 bases (at least k + 16) every 16 bases, reverse-complemented at random, each `copies`
            (1, 3, 130, 300) times, so some tables and edge counters pass 254; about every second time a second haplotype
            (three substitutions) at one copy: branches with small counters; joined by one of four separators
  asm       the genome with 1-5 edits: substitution, deletion, lower-case insertion, or a byte that cuts the segment
Three flavours steer the draw, so that no stage is compared on nothing (the conditions of tests/test_fuzz_inputs.py):
  circular  seed % 8 == 3.  Reads run round the end of the genome, asm = genome + its first k - 1 + TAIL bases again, and the
            edits fall into the last TAIL bases, whose k-mers the front of asm holds already: full alphabet, one haplotype, no
            repeat, no constructed k-mers, so the subgraph is the closed ring and the GFA has a cycle to cut
  plain     one seed per k (the first of its four, the second where the first is circular): full alphabet, two haplotypes, at
            least two edits, the first a substitution in the middle third, variant depth >= k and span >= 5, constructed k-mers
            and at least one round of subgraph search: what a variant path and a branching subgraph need, at every k
  free      everything else: all draws as listed above

expected(seed) computes the answers once per process; both test files share them and leave them unchanged."""
import functools
import types

import numpy as np
import pytest

from oracle import variants as V
from tests import gfa_ref as G
from tests import helpers as H
from tests import subgraph_ref as R
from tests import table_ref as T
from tests import variant_cases as C

N_SEEDS = 124
SEEDS = tuple(range(N_SEEDS))
MAPS = 128
ALPHABETS = [b"ACGT", b"ACGTacgt", b"AAAAAAAC", b"ACACACAG", b"AC", b"ACGTTTTT"]
SEPARATORS = [b"\n", b"N", b"\x00", b"\n\n"]
CUTS = b"N\n-*"
STEP, TAIL = 16, 40
HINTS = [0, 1, 5000, 3_000_000]
HIGH = 254                                                               # counters above it live in the second tier


def k_of(seed):
    return 2 + seed % 31


def is_circular(seed):
    return seed % 8 == 3


def is_plain(seed):
    return (seed < 31 and not is_circular(seed)) or (31 <= seed < 62 and is_circular(seed - 31))


def _draw(rng, alphabet, n):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _other(rng, base):
    return bytes([[c for c in b"ACGT" if c != base[0] & 0xDF][int(rng.integers(0, 3))]])


def _fragments(rng, genome, frag, circular):
    n = len(genome)
    if circular:
        text, starts = genome + genome[:frag], list(range(0, n, STEP))
    else:
        text, starts = genome, list(range(0, max(1, n - frag + 1), STEP)) + [max(0, n - frag)]
    out = [text[s:s + frag] for s in starts]
    return [H.revcomp_bases(r) if rng.random() < 0.5 else r for r in out]


def case(seed):
    rng = np.random.default_rng(77_000 + seed)
    k = k_of(seed)
    circular, plain = is_circular(seed), is_plain(seed)
    full = circular or plain
    alphabet = ALPHABETS[int(rng.integers(0, 2 if full else len(ALPHABETS)))]
    short = not full and rng.random() < 0.1
    n = k + 3 if short else int(rng.integers(150, 401))
    genome = bytearray(_draw(rng, alphabet, n))
    tandem = 0
    if not short and not circular and rng.random() < 0.5:
        tandem = int(rng.integers(1, 12))
        at = int(rng.integers(0, n - 60))
        genome[at:at + 60] = (_draw(rng, alphabet, tandem) * 60)[:60]
    palindrome = False
    if not short and not circular and k % 2 == 0 and rng.random() < 0.5:
        half = _draw(rng, b"ACGT", k // 2)
        at = int(rng.integers(0, n - k))
        genome[at:at + k] = half + H.revcomp_bases(half)
        palindrome = True
    genome = bytes(genome)

    copies = int(rng.choice([1, 3, 130, 300]))
    frag = max(k + STEP, int(rng.choice([40, 70, 100])))                 # neighbours overlap by k bases: no k-mer falls between two
    reads = [r for f in _fragments(rng, genome, frag, circular) for r in [f] * copies]
    hap2 = plain or (not circular and rng.random() < 0.5)
    if hap2:
        alt = bytearray(genome)
        for p in rng.integers(0, n, 3).tolist():
            alt[p:p + 1] = _other(rng, alt[p:p + 1])
        reads += _fragments(rng, bytes(alt), frag, False)
    sep = SEPARATORS[int(rng.integers(0, 4))]
    reads = sep.join(reads)

    source = genome + genome[:k - 1 + TAIL] if circular else genome
    asm = [source[i:i + 1] for i in range(len(source))]
    n_edits = int(rng.integers(2 if plain else 1, 6))
    lo, hi = (len(source) - TAIL, len(source)) if circular else (0, len(source))
    edits = []
    for e in range(n_edits):
        p = int(rng.integers(lo, hi))
        kind = int(rng.integers(0, 4))
        if plain and e == 0:
            p, kind = int(rng.integers(len(source) // 3, 2 * len(source) // 3)), 0
        if kind == 0:
            asm[p] = _other(rng, source[p:p + 1])
        elif kind == 1:
            asm[p] = b""
        elif kind == 2:
            asm[p] = _draw(rng, b"acgt", 1) + asm[p]
        else:
            asm[p] = CUTS[int(rng.integers(0, 4)):][:1]
        edits.append((p, kind))
    asm = b"".join(asm)
    assert len(asm) < 500

    return types.SimpleNamespace(
        seed=seed, k=k, reads=reads, asm=asm, genome=genome, flavour="circular" if circular else "plain" if plain else "free",
        alphabet=alphabet, tandem=tandem, palindrome=palindrome, copies=copies, hap2=hap2, edits=edits,
        db_hint=int(rng.choice(HINTS)), sub_hint=int(rng.choice(HINTS)), image_hint=int(rng.choice(HINTS)),
        var_depth=int(rng.choice([k, 40, 253] if plain else [0, 1, k, 40, 253])),
        var_span=int(rng.choice([5, 32, 255] if plain else [0, 1, 5, 32, 255])),
        var_cutoff=int(rng.choice([0, 0, 2, 5])), var_batch=int(rng.choice([0, 1, 7])),
        algorithm="traversal" if circular or rng.random() < 0.5 else "best-first",
        sub_depth=min(k, 8) if circular else int(rng.integers(1 if plain else 0, min(k, 8) + 1)),
        no_reference=circular or bool(not plain and rng.random() < 0.5),
        search_cutoff=int(rng.choice([0, 2])), trim_cutoff=0 if circular else int(rng.choice([0, 2])),
        table_format=int(rng.choice([T.KWIG, T.BED, T.CSV])))


# ---- the answers -------------------------------------------------------------------------------------------------------

def graph_of_entries(entries, k):
    g = V.Graph(entries, k)
    g.nodes = C.ZeroNodes(g.nodes)
    return g


def variant_paths(g, asm, depth, span, cutoff):
    """[(pos, seg_start, type, refLen, sequence)] of kq_search_variants for `asm` on graph g"""
    with pytest.MonkeyPatch.context() as m:
        C.with_cutoff(m, cutoff)
        return C.want_of(g, asm.decode("latin-1"), depth, span)


def first_tier_only(entries):
    """the table as the 8-bit tier alone shows it: a high-copy k-mer is a tombstone there, cov 255 and no edge counters"""
    e = entries.copy()
    hot = e["cov"] > HIGH
    e["cov"][hot] = 255
    e["fw"][hot] = 0
    e["bw"][hot] = 0
    return e


def clamped(entries):
    """every counter of the high-copy entries cut down to 254"""
    e = entries.copy()
    hot = e["cov"] > HIGH
    for f in ("cov", "fw", "bw"):
        e[f][hot] = np.minimum(e[f][hot], HIGH)
    return e


def copy_table(table):
    return {key: (list(f), list(b), cov) for key, (f, b, cov) in table.items()}


def runs_of(asm):
    """the ACGTacgt runs of the text -> [(start, length)]"""
    return [(start, len(seg)) for start, seg in V.segments_of(asm.decode("latin-1"))]


def table_pieces(c):
    """one piece per run of at least k bases: its k-mer positions, named by the run's number"""
    pieces, segments, first = [], [], 0
    for i, (start, n) in enumerate(runs_of(c.asm)):
        if n >= c.k:
            pieces.append(T.Piece(first, n - c.k + 1, start, b"seq%d" % i, 0, c.table_format == T.KWIG))
            segments.append((start, n - c.k + 1))
            first += n - c.k + 1
    return pieces, segments


@functools.lru_cache(maxsize=None)
def expected(seed):
    from oracle import oracle as O

    c = case(seed)
    k = c.k
    db = O.OracleDB(k, MAPS)
    db.count_batch(c.reads)
    entries = db.export()
    e = types.SimpleNamespace(case=c, entries=entries)
    e.flags = {cut: H.branch_flags(entries, k, c.asm, cut) for cut in {0, c.var_cutoff}}
    e.graph = graph_of_entries(entries, k)
    e.paths = variant_paths(e.graph, c.asm, c.var_depth, c.var_span, c.var_cutoff)

    table = R.table_of(entries)
    sub = R.seed(table, [c.asm], k, c.no_reference)
    e.sub_seed = copy_table(sub)
    if c.algorithm == "traversal":
        e.n_added = R.traversal(table, sub, k, c.sub_depth)
    else:
        e.n_added = R.best_first(table, sub, k, c.sub_depth, c.search_cutoff)
    e.sub_grown = copy_table(sub)
    R.trim(sub, k, c.trim_cutoff)
    e.sub_trimmed = sub
    e.gfa = {no_collapse: G.build(sub, k, no_collapse) for no_collapse in (False, True)}

    e.lookup = db.validate_sequence(c.asm, per_base=True)
    e.pieces, e.segments = table_pieces(c)
    e.triples = T.triples_of(e.lookup[1], e.segments)
    e.text = T.format_table(c.table_format, k, e.triples, e.pieces)
    db.close()
    return e
