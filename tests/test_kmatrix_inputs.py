"""CPU checks of the inputs tests/test_gpu_kmatrix.py builds (tests/helpers.py): the de Bruijn sequences, the planted
palindromes, the high-copy reads and the canonical-key enumeration, so that they are known to be what that file claims
before any GPU runs them."""
import numpy as np
import pytest

from tests import helpers as H


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def window_keys(codes, k):
    """packed key of every k-base window of a code array (first base in the low bits)"""
    n = len(codes) - k + 1
    keys = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        keys |= codes[j:j + n].astype(np.uint64) << np.uint64(2 * j)
    return keys


@pytest.mark.parametrize("k", range(2, 12))
def test_de_bruijn_has_every_kmer_once(k):
    seq = H.de_bruijn_linear(k)
    assert len(seq) == 4 ** k + k - 1
    codes = np.frombuffer(seq.translate(bytes.maketrans(b"ACGT", b"\0\1\2\3")), dtype=np.uint8)
    keys = window_keys(codes, k)
    assert np.array_equal(np.sort(keys), np.arange(4 ** k, dtype=np.uint64))


@pytest.mark.parametrize("k", range(2, 9))
def test_canonical_keys_equal_oracle_export(O, k):
    keys = H.all_canonical_keys(k)
    assert len(keys) == H.n_canonical(k)
    assert int(keys[-1]) == H.max_canonical_key(k)
    seq = H.de_bruijn_linear(k)
    db = O.OracleDB(k, 128)
    db.count_batch(seq)
    e = db.export()
    assert np.array_equal(np.sort(e["key"]), keys)
    st = db.summary()
    assert st["distinct"] == H.n_canonical(k) and st["missing"] == 4 ** k - H.n_canonical(k)


@pytest.mark.parametrize("k", [2, 5, 12, 21, 24, 25, 29, 31, 32])
def test_revcomp_keys_match_oracle_hash(O, k):
    """the numpy reverse complement / canonical form (used for the hand-built import keys at large k) == kqo_hash"""
    rng = np.random.default_rng(k)
    codes = rng.integers(0, 4, (200, k), dtype=np.uint8)
    fw = np.array([H.key_of_codes(c) for c in codes], dtype=np.uint64)
    want = np.array([O.hash_kmer(c, k)[0] for c in codes], dtype=np.uint64)
    assert np.array_equal(H.canonical_keys_of(fw, k), want)
    assert np.array_equal(H.revcomp_keys(H.revcomp_keys(fw, k), k), fw)


@pytest.mark.parametrize("k", [2, 4, 6, 8, 10, 16, 20, 24, 26, 30, 32])
def test_planted_palindromes(O, k):
    pals = H.palindromes(k, 60, seed=k)
    assert len(pals) == min(60, 4 ** (k // 2)) and len(set(pals)) == len(pals)
    reads = H.plant_palindromes(k, pals, seed=k)
    keys, edges = O.emit_records(k, b"\n".join(reads))
    codes = {b: i for i, b in enumerate(b"ACGT")}
    for p in pals:
        assert len(p) == k and p == H.revcomp_bases(p)
        key, is_fw = O.hash_kmer([codes[b] for b in p], k)
        assert not is_fw                                          # a palindrome is never forward
        assert key == H.key_of_codes([codes[b] for b in p])
        assert key in keys
        mine = edges[keys == key]
        assert (mine & 0xF0).any() and (mine & 0x0F).any()      # both edge directions occur
        assert (mine == 0).any()                                 # the palindrome alone in a read: no neighbour at all
    db = O.OracleDB(k, 128)
    db.count_batch(b"\n".join(reads))
    e = db.export()
    hot = H.key_of_codes([codes[b] for b in pals[0]])
    row = e[e["key"] == hot]
    assert len(row) == 1 and row["hc"][0] == 1 and row["cov"][0] > 255


@pytest.mark.parametrize("k", [3, 21, 32])
def test_hot_kmer_reads(O, k):
    kmer, reads = H.hot_kmer_reads(k, seed=k)
    assert kmer != H.revcomp_bases(kmer)
    db = O.OracleDB(k, 128)
    db.count_batch(b"\n".join(reads))
    e = db.export()
    assert e["cov"].max() > 255 and e["hc"].max() == 1
