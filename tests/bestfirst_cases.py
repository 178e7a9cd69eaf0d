"""Inputs of the best-first tests (tests/test_bestfirst_core_host.py on the CPU, tests/test_gpu_subgraph_bestfirst.py on the
GPU) and what tests/subgraph_ref.py gives on them -- TEST INFRASTRUCTURE ONLY.  Every case is (reads, seed sequence)."""
import numpy as np

from tests import helpers as H

# k-mers added over all seeds by R.best_first at cov_cutoff 0, {k: {depth: added}}
DENSE_ADDED = {4: {1: 1, 2: 1, 4: 12, 12: 40, 40: 87, 255: 92}, 5: {1: 0, 2: 0, 5: 4, 12: 18, 40: 62, 255: 194}}
DENSE_CUTOFFS = (0, 2)
# bubble_genome(21) of tests/test_gpu_subgraph.py, {(depth, cutoff): added}; 58 seeds
BUBBLE_SEEDS = 58
BUBBLE_ADDED = {(0, 0): 0, (1, 0): 0, (2, 0): 0, (5, 0): 0, (21, 0): 42, (30, 0): 42, (255, 0): 42, (255, 2): 163}
BUBBLE_DEPTHS = (0, 1, 2, 5, 21, 30, 255)
# linear path, k = 21, depth 255, cutoff 0: {genome seed: added for gap 253..257}
SATURATED_GAPS = (253, 254, 255, 256, 257)
SATURATED_ADDED = {1: [252, 253, 1, 0, 0], 3: [252, 253, 1, 1, 0]}


def dense(k):
    """a random 300-base string counted at k = 4 / 5: most k-mers have several edges in both directions, the queue reaches
    30 nodes at k = 4 and consolidation links several degrees; even k brings k-mers that are their own reverse complement"""
    g = H.ACGT[np.random.default_rng(k).integers(0, 4, 300)].tobytes()
    return g, g[:12] + b"N" + g[100:110]


def dense_depths(k):
    return (1, 2, k, 12, 40, 255)


def saturated(s, gap):
    """a linear path whose two seed stretches are `gap` bases apart: dist saturates at 255 and leaves a node without prev"""
    _, genome = H.synth_reads(10, 100, 700, seed=s, err=0.0)
    return genome, genome[:21] + b"N" + genome[gap:gap + 21]


def two_stretches(k, seed):
    """reads of a random 400-base genome; the last k-mer of the first seed stretch and the first of the second are 30
    k-mers apart, which a search of depth k >= 31 bridges"""
    reads, genome = H.synth_reads(120, 100, 400, seed=seed, err=0.0)
    a = 100
    return reads, genome[a:a + k + 18] + b"N" + genome[a + 48:a + 48 + k + 20]


def high_copy_path(k=21):
    """320 copies of one random 60-base string: every k-mer and edge counter is 320, above the 8-bit tier; the seeds are its
    first and its last k-mer"""
    s = H.ACGT[np.random.default_rng(60).integers(0, 4, 60)].tobytes()
    return b"\n".join([s] * 320), s[:k] + b"N" + s[-k:]
