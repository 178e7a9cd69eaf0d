"""Inputs of the graph tests (tests/test_gfa_ref.py on the CPU, tests/test_gpu_subgraph_gfa.py and
tests/test_gpu_subgraph_gfa_cli.py on the GPU) -- TEST INFRASTRUCTURE ONLY.  Pure Python / numpy, no GPU.

  golden_table(idx)    the trimmed subgraph table the restatement (tests/subgraph_ref.py) gives for validateFiles/test.<idx>.tst
  input_table(k)       the same for tests/subgraph_inputs.graph_case(k): a traversal of depth 2 from its seed batch
  hand_case(name, k)   hand-made tables, one structure each (HAND_CASES lists them with the k they exist at)
Tables are {key: (fw[4], bw[4], cov)}; every one is a valid kq_import input (cov > 0, counters <= cov).
"""
import os

import numpy as np

from tests import helpers as H
from tests import subgraph_inputs as SI
from tests import subgraph_ref as R
from tests.test_subgraph_ref import K as GOLDEN_K, parse_subgraph_cmd

SUBGRAPH_TESTS = list(range(36, 48))
_golden, _inputs, _hand = {}, {}, {}
_db_tables = {}


def golden_argv(idx):
    return H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", f"test.{idx}.tst"))


def golden_table(idx):
    """-> (table, no_collapse, expected stdout lines)"""
    if idx not in _golden:
        argv, expected = golden_argv(idx)
        o = parse_subgraph_cmd(argv)
        if o["db"] not in _db_tables:
            _db_tables[o["db"]] = R.table_of(H.load_db_table(o["db"]))
        seqs = [s for _, s in H.read_fastx(o["fasta"])]
        sub = R.subgraph(_db_tables[o["db"]], seqs, GOLDEN_K, o["depth"], o["algorithm"], o["no_reference"], o["cov_cutoff"])
        _golden[idx] = (sub, "--no-collapse" in argv, expected)
    return _golden[idx]


def count_table(k, seqs):
    """the table a count of `seqs` (ACGT strings) gives: cov per occurrence, one edge per neighbour inside the sequence"""
    t = {}
    mask = (1 << (2 * k)) - 1
    for s in seqs:
        codes = ["ACGT".index(c) for c in s]
        fwd = rev = 0
        for end, c in enumerate(codes):
            fwd = (fwd >> 2) | (c << (2 * k - 2))
            rev = ((rev << 2) | (3 - c)) & mask
            if end < k - 1:
                continue
            p = end - k + 1
            key, is_fw = (fwd, True) if fwd < rev else (rev, False)
            f, b, cov = t.setdefault(key, ([0] * 4, [0] * 4, [0]))
            cov[0] += 1
            nxt = codes[p + k] if p + k < len(codes) else None
            prv = codes[p - 1] if p > 0 else None
            if is_fw:
                if nxt is not None:
                    f[nxt] += 1
                if prv is not None:
                    b[prv] += 1
            else:
                if prv is not None:
                    f[3 - prv] += 1
                if nxt is not None:
                    b[3 - nxt] += 1
    return {key: (f, b, cov[0]) for key, (f, b, cov) in t.items()}


def key_of(kmer):
    k = len(kmer)
    fwd = sum("ACGT".index(c) << (2 * i) for i, c in enumerate(kmer))
    rev = sum((3 - "ACGT".index(c)) << (2 * (k - 1 - i)) for i, c in enumerate(kmer))
    return min(fwd, rev)


def rc(s):
    return "".join("ACGT"[3 - "ACGT".index(c)] for c in reversed(s))


def _rand(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _simple(k, s):
    """every k-mer of s occurs once, on one strand, and none is a palindrome"""
    kmers = [s[i:i + k] for i in range(len(s) - k + 1)]
    keys = {key_of(x) for x in kmers}
    return len(keys) == len(kmers) and all(x != rc(x) for x in kmers)


def _draw(rng, k, n, ok=lambda s: True):
    for _ in range(10000):
        s = _rand(rng, n)
        if _simple(k, s) and ok(s):
            return s
    raise AssertionError("no such sequence")


def _cycle(rng, k, n_kmers):
    """a circular string of n_kmers bases whose n_kmers k-mers are distinct -> it, read twice round (every edge present)"""
    for _ in range(10000):
        c = _rand(rng, n_kmers)
        if _simple(k, (c * (k // n_kmers + 2))[:n_kmers + k - 1]):
            return c
    raise AssertionError("no such cycle")


def _unroll(c, k, turns=2):
    return (c * (turns + k // len(c) + 1))[:turns * len(c) + k - 1]


def _make(name, k):
    rng = np.random.default_rng([k, sum(name.encode())])
    short = 9 if k < 8 else 30                                           # bases of a random stretch: few enough k-mers at k = 5
    if name == "pure_cycle":
        return count_table(k, [_unroll(_cycle(rng, k, 7 if k < 8 else 40), k)])
    if name == "cycle_with_tail":
        c = _cycle(rng, k, 7 if k < 8 else 40)
        body = _unroll(c, k)
        tail = _draw(rng, k, short, lambda s: _simple(k, s + body[:len(c) + k - 1]))
        return count_table(k, [tail + body])
    if name == "hairpin":                                                # x = c P with a palindrome P of k - 1 bases: x -> rc(x)
        half = _rand(rng, (k - 1) // 2)
        pal = half + rc(half)
        pre = _draw(rng, k, short, lambda s: _simple(k, s + "A" + pal))
        s = pre + "A" + pal
        return count_table(k, [s + rc(s)[k - 1:]])
    if name == "homopolymer":
        pre, post = _draw(rng, k, short, lambda s: s[-1] != "A"), _draw(rng, k, short, lambda s: s[0] != "A")
        return count_table(k, [pre + "A" * (k + 2) + post])
    if name == "palindrome":                                             # even k: a k-mer that is its own reverse complement inside a path
        seqs = []
        for same in (False, True):                                       # same: the k-mer behind it is the reverse complement of the one in front
            half = _rand(rng, k // 2)
            pre, post = _rand(rng, short), _rand(rng, short)
            behind = rc(pre[-1]) if same else next(c for c in "ACGT" if c != rc(pre[-1]))
            seqs.append(pre + half + rc(half) + behind + post[1:])
        return count_table(k, seqs)
    if name == "isolated":
        return count_table(k, [_draw(rng, k, k), _draw(rng, k, short)])
    if name == "two_kmer_unitig":                                        # a1 / a2 -> m (k + 1 bases: two k-mers) -> b1 / b2
        m = _draw(rng, k, k + 1)
        a1, a2 = _rand(rng, short - 1) + "A", _rand(rng, short - 1) + "C"
        b1, b2 = "G" + _rand(rng, short - 1), "T" + _rand(rng, short - 1)
        return count_table(k, [a1 + m + b1, a2 + m + b2])
    if name == "asymmetric":                                             # e -> w has a counter, w knows nothing of e; w lies inside a unitig
        for _ in range(1000):
            path = _draw(rng, k, 3 * short)
            j = short
            w = path[j:j + k]
            lead = next(c for c in "ACGT" if c != path[j - 1])
            e = lead + w[:k - 1]
            other = _rand(rng, short)
            if _simple(k, other + e) and _simple(k, path) and not {key_of((other + e)[i:i + k]) for i in range(short + 1)} & set(count_table(k, [path])):
                break
        else:
            raise AssertionError("no such pair")
        t = count_table(k, [path, other + e])
        f, b, _ = t[key_of(e)]
        base = "ACGT".index(w[-1])                                       # e's string appends w's last base
        if _kmer(key_of(e), k) == e:
            f[base] = 1
        else:
            b[3 - base] = 1
        return t
    if name == "trimmed_counter":                                        # the k-mer a counter points to is gone (a cutoff trim keeps small counters)
        path = _draw(rng, k, 2 * short)
        t = count_table(k, [path])
        del t[key_of(path[short:short + k])]
        return t
    if name == "cov300":
        path = _draw(rng, k, short)
        return {key: (f, b, 300) for key, (f, b, _) in count_table(k, [path]).items()}
    if name == "long_unitig":
        return count_table(k, [_draw(rng, k, 5000 + k - 1)])
    if name == "long_cycle":
        c = _cycle(rng, k, 3000)
        return count_table(k, [(c * 2)[:len(c) + k]])                     # once round, and the first k-mer again: the closing edge
    raise KeyError(name)


def _kmer(key, k):
    return "".join("ACGT"[(key >> (2 * c)) & 3] for c in range(k))


# name -> the k it is built at.  A palindromic k-mer needs an even k; 5000 distinct k-mers do not exist at k = 5 (512 keys)
HAND_CASES = {"pure_cycle": (5, 21), "cycle_with_tail": (5, 21), "hairpin": (5, 21), "homopolymer": (5, 21), "palindrome": (6, 20),
              "isolated": (5, 21), "two_kmer_unitig": (5, 21), "asymmetric": (5, 21), "trimmed_counter": (5, 21), "cov300": (5, 21),
              "long_unitig": (21,), "long_cycle": (21,)}
HAND_IDS = [(name, k) for name, ks in HAND_CASES.items() for k in ks]


def hand_case(name, k):
    if (name, k) not in _hand:
        _hand[(name, k)] = _make(name, k)
    return _hand[(name, k)]


INPUT_KS = (4, 8, 21, 31, 32)


def input_table(k):
    """the trimmed subgraph of tests/subgraph_inputs.graph_case(k): its reads counted, its batch seeded, one traversal round"""
    if k not in _inputs:
        case = SI.graph_case(k)
        db = count_table(k, [s for r in case.reads.decode().upper().split("\n") for s in R.segments_of(r)])
        _inputs[k] = R.subgraph(db, [case.batch], k, 2, "traversal")
    return _inputs[k]
