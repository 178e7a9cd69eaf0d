"""Inputs of the candidate-error search tests (tests/test_variant_core_host.py on the CPU, tests/test_gpu_variants.py on the
GPU) and the expected paths from oracle/variants.py -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import oracle as O
from oracle import variants as V
from tests import helpers as H

MAPS = 128
TYPE_CODE = {V.SNV: 0, V.INS: 1, V.DEL: 2, V.COM: 3}      # KQ_VAR_* of include/kreeq_amd.h


class ZeroNodes(dict):
    """Graph.nodes with an all-zero entry for every key it lacks (the reference dereferences end() there; the engine makes
    such a neighbour a node without edges).  `key in nodes` still tells whether the k-mer is in the table."""

    def __missing__(self, key):
        return ([0] * 4, [0] * 4, 0)


def graph_of(k, reads):
    db = O.OracleDB(k, MAPS)
    db.count_batch(reads if isinstance(reads, bytes) else reads.encode())
    g = V.Graph(db.export(), k)
    g.nodes = ZeroNodes(g.nodes)
    return g


def with_cutoff(monkeypatch, cov_cutoff):
    """dbg_to_variants calls search_variants without a cutoff: pass one"""
    if not cov_cutoff:
        return
    orig = V.search_variants
    monkeypatch.setattr(V, "search_variants", lambda *a, **kw: orig(*a, cov_cutoff=cov_cutoff, **kw))


def expected(g, segments, depth, span):
    """-> [(segment index, pos, type code, refLen, sequence)] in segment, position and destination order"""
    out = []
    for si, seg in enumerate(segments):
        for paths in V.dbg_to_variants(g, seg, depth, span):
            out += [(si, p["pos"], TYPE_CODE[p["type"]], p["refLen"], p["sequence"]) for p in paths]
    return out


def want_of(g, text, depth, span):
    """the oracle over the segments of `text` -> [(pos, seg_start, type, refLen, sequence)] in the ABI's coordinates"""
    text = text.decode() if isinstance(text, bytes) else text
    out = []
    for start, seg in V.segments_of(text):
        out += [(start + pos, start, t, r, s) for _, pos, t, r, s in expected(g, [seg], depth, span)]
    return out


def window_stats(k, segment, span):
    """the targets of every position of a segment, by the reference's own queue / map steps (oracle/variants.py:326-341) ->
    (positions whose queue holds a key twice, positions where a queued key is missing from the map: the erase quirk)"""
    from collections import deque

    codes = [V.CTOI[ch] for ch in segment]
    kcount = len(segment) - k + 1
    keys = [V.hash_kmer(codes[t:t + k], k)[0] for t in range(kcount)]
    queue, tmap = deque(), {}
    for pos in range(span):
        if pos + k < kcount:
            queue.append(keys[pos + k])
            tmap[keys[pos + k]] = True
    twice = erased = 0
    for c in range(kcount):
        if queue:
            tmap.pop(queue[0], None)
            queue.popleft()
        if c + k + span < kcount:
            tmap[keys[c + k + span]] = True
            queue.append(keys[c + k + span])
        twice += len(set(queue)) < len(queue)
        erased += any(key not in tmap for key in queue)
    return twice, erased


def random_text(n, seed):
    return H.ACGT[np.random.default_rng(seed).integers(0, 4, n)].tobytes().decode()


def tiled_reads(genome, read_len=100, step=8, copies=1):
    """error-free reads over the whole string, both strands alternating"""
    reads = []
    for j, s in enumerate(list(range(0, max(1, len(genome) - read_len + 1), step)) + [max(0, len(genome) - read_len)]):
        r = genome[s:s + read_len]
        if j & 1:
            r = r[::-1].translate(str.maketrans("ACGT", "TGCA"))
        reads += [r] * copies
    return "\n".join(reads)


def other_base(ch, by=1):
    return "ACGT"[("ACGT".index(ch) + by) % 4]


def planted(k=21, n=700, seed=5):
    """-> (reads of a random genome, the genome with a substitution, a 1-base insertion, a 1-base deletion and two
    substitutions 5 bases apart -- closer than a max_span of 32, one COM record)"""
    genome = random_text(n, seed)
    a = list(genome)
    a[120] = other_base(a[120])
    a.insert(250, other_base(a[250], 2))
    del a[380]
    a[500] = other_base(a[500])
    a[505] = other_base(a[505], 3)
    return tiled_reads(genome), "".join(a), genome


def tandem(k=21, seed=9):
    """a 7-base unit repeated 12 times between random flanks, with a substitution just in front of the repeat: the k-mers of
    the repeat recur with period 7 inside one window, so the erase quirk decides which are targets and a target key occurs
    several times in the queue (first-occurrence refLen)"""
    left, unit, right = random_text(150, seed), "ACGGTCA", random_text(150, seed + 1)
    genome = left + unit * 12 + right
    a = list(genome)
    a[140] = other_base(a[140])
    a[150 + 7 * 5 + 3] = other_base(a[150 + 7 * 5 + 3], 2)
    return tiled_reads(genome), "".join(a), genome


def thin(k=21, seed=21):
    """reads at about 4x with 2 % errors: edge counters of 1 .. 4, so cutoffs 0, 1 and 3 follow different backward edges"""
    reads, genome = H.synth_reads(32, 100, 800, seed=seed, err=0.02)
    return reads.decode(), genome.decode()
