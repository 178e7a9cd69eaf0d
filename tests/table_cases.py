"""Inputs of the per-base table tests, shared by the host program (tests/test_table_core_host.py) and the kernels
(tests/test_gpu_table_format.py): triples whose digit counts vary from lane to lane, coordinates across digit boundaries, and
pieces at the window's and the tile's edges.  Every case is (triples uint32 [n, 3], [table_ref.Piece])."""
import numpy as np

from tests import table_ref as T

EDGE_VALUES = np.array(sorted({0, 4294967295} | {10 ** d for d in range(1, 10)} | {10 ** d - 1 for d in range(1, 10)}), dtype=np.uint32)
ABS_EDGES = (0, 5, 99990, 2 ** 32 - 40)                # ranges of 100+ positions from here cross 9 -> 10, 99 999 -> 100 000, 2^32 - 1 -> 2^32
NAMES = {1: b"s", 7: b"chr_7_x", 300: (b"scaffold_0123456789" * 16)[:300]}
TILE = 256                                               # TAB_TILE of kreeq_amd/csrc/kq_table.h (a power of two below 8192)
SEGMENT_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193)


def values(n, seed):
    """[n, 3]: small random counts with the digit-boundary values and 2^32 - 1 mixed in, in every column"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 400, (n, 3), dtype=np.uint32)
    edge = rng.random((n, 3)) < 0.25
    v[edge] = EDGE_VALUES[rng.integers(0, len(EDGE_VALUES), int(edge.sum()))]
    if n >= len(EDGE_VALUES):                            # every edge value in every column at least once
        for c in range(3):
            v[rng.permutation(n)[:len(EDGE_VALUES)], c] = EDGE_VALUES
    return v


def one_segment(n, seed, name=NAMES[7], abs_pos=0, header=True):
    return values(n, seed), [T.Piece(0, n, abs_pos, name, 0, header)]


def many_pieces(seed, count=300):
    """`count` pieces of 1..3 positions over one triple array, names and coordinates changing, some without header"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 4, count)
    t = values(int(lens.sum()) + 5, seed + 1)
    pieces, at = [], 0
    for i, n in enumerate(lens.tolist()):
        pieces.append(T.Piece(at, n, ABS_EDGES[i % len(ABS_EDGES)] + i, NAMES[(1, 7, 300)[i % 3]], 0, i % 5 != 4))
        at += n
    return t, pieces


def big_then_one(k):
    """a segment of 10-digit values directly followed by a one-position segment: nothing of the first may show in the second"""
    t = np.full((k + 6, 3), 4294967295, dtype=np.uint32)
    t[-1] = (1, 2, 3)
    return t, [T.Piece(0, k + 5, 0, b"big", 0, True), T.Piece(k + 5, 1, 7, b"one", 0, True)]


def cut_in_two(k, cut, n=100, seed=5):
    """-> (triples, the whole segment, its two pieces with n_ctx = min(cut, k - 1))"""
    t = values(n, seed)
    whole = [T.Piece(0, n, 99990, NAMES[7], 0, True)]
    return t, whole, [T.Piece(0, cut, 99990, NAMES[7], 0, True), T.Piece(cut, n - cut, 99990 + cut, NAMES[7], min(cut, k - 1), False)]
