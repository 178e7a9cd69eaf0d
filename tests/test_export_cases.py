"""The case list of tests/test_gpu_export.py is what it claims to be (tests/export_cases.py), checked without a GPU: keys are
distinct, canonical and never the empty marker; both tiers occur from n = 300; key 0, the largest canonical key and the pairs
that differ in bit 0 or in bit 2k - 1 alone are there from n = 4; every n exists at its k; every sort algorithm, both parities of
the onesweep pass count and both copy paths are reached; and the direct / bounced label of every case is the plan of
kreeq_amd/csrc/kq_export_host.h itself (tests/native/export_plan_main.cpp prints it)."""
import subprocess

import numpy as np
import pytest

from tests import export_cases as EC
from tests import helpers as H
from tests.test_export_plan_host import build_export_plan

CASES = EC.cases()
LIGHT = [c for c in CASES if c[1] <= 70_000]             # the key sets of the large cases are drawn the same way; two of them below


def check_keys(k, n, keys, seed=0):
    assert keys.dtype == np.uint64 and len(keys) == n == len(np.unique(keys))
    assert np.array_equal(H.canonical_keys_of(keys, k), keys)
    assert not (keys == np.uint64(EC.EMPTY_KEY)).any()
    if k < 32:
        assert not (keys >> np.uint64(2 * k)).any()
    if n >= 4:
        have = set(keys.tolist())
        top = 1 << (2 * k - 1)
        assert 0 in have and H.max_canonical_key(k) in have
        assert any((x ^ 1) in have for x in have if not x & 1)
        assert any((x | top) in have for x in have if not x & top)
        if k == 32:
            assert min(x for x in have if x & top) == 1 << 63 and sum(1 for x in have if x & top) >= 2
    if n >= 64 and k >= 5:
        low, top_keys = EC.pair_keys(k, seed)
        assert len(low) >= 1 and len(top_keys) >= 1
        assert set(low.tolist()) <= have and set((low ^ np.uint64(1)).tolist()) <= have
        assert set(top_keys.tolist()) <= have and set((top_keys | np.uint64(top)).tolist()) <= have


def check_payload(e):
    cov = e["cov"].astype(np.uint64)
    assert np.array_equal(cov, 1 + e["key"] % np.uint64(300))
    assert (e["fw"] <= e["cov"][:, None]).all() and (e["bw"] <= e["cov"][:, None]).all()
    assert np.array_equal(e["hc"] != 0, e["cov"] > 254)
    if len(e) >= 300:
        assert (e["cov"] > 254).any() and (e["cov"] <= 254).any()
        counters = np.concatenate([e["fw"], e["bw"]], axis=1)
        for a in range(8):                                  # no two counters are the same function of the key
            for b in range(a + 1, 8):
                assert (counters[:, a] != counters[:, b]).mean() > 0.5


@pytest.mark.parametrize("case", LIGHT, ids=EC.case_id)
def test_case_tables(case):
    k, n, modes = case
    assert n <= H.n_canonical(k)
    assert set(modes) <= set(EC.MODES) and "default" in modes
    e = EC.entries(k, n)
    check_keys(k, n, e["key"])
    check_payload(e)
    assert np.array_equal(EC.entries(k, n)["key"], e["key"])              # the same table every time
    want = EC.expected(e)
    assert len(want) == n and (want["key"][1:] > want["key"][:-1]).all()


@pytest.mark.parametrize("k,n", [(11, 2_097_152), (32, 1_500_000)])
def test_large_tables(k, n):
    assert (k, n, ("default",)) in CASES
    e = EC.entries(k, n)
    check_keys(k, n, e["key"])
    check_payload(e)
    if k == 11:
        assert n == H.n_canonical(11) and np.array_equal(np.sort(e["key"]), H.all_canonical_keys(11))       # the whole key space


def test_every_case_exists_at_its_k():
    assert len(CASES) == len(set((k, n) for k, n, _ in CASES))
    for k, n, _ in CASES:
        assert 2 <= k <= 32 and n <= H.n_canonical(k), (k, n)


def test_saturated_table():
    e = EC.saturated_entries()
    check_keys(21, len(e), e["key"], seed=5)
    assert set(e["cov"].tolist()) == {254, 255, 256, EC.LARGEST}
    assert (e["fw"] <= e["cov"][:, None]).all() and (e["bw"] <= e["cov"][:, None]).all() and np.array_equal(e["hc"] != 0, e["cov"] > 254)
    counters = set(np.concatenate([e["fw"], e["bw"]], axis=1).ravel().tolist())
    assert {0, 1, 254, 255, 256, EC.LARGEST - 1, EC.LARGEST} <= counters
    d = EC.doubled(e)
    assert set(d["cov"].tolist()) == {508, 510, 512, EC.LARGEST} and d["fw"].max() == EC.LARGEST and (d["hc"] == 1).all()


def test_regimes_are_reached():
    default = [(k, n) for k, n, _ in CASES]
    assert {EC.sort_algorithm(n) for _, n in default} == {"block", "merge", "onesweep"}
    assert EC.sort_algorithm(1024) == "block" and EC.sort_algorithm(1025) == "merge" and EC.sort_algorithm(1 << 20) == "merge" and EC.sort_algorithm((1 << 20) + 1) == "onesweep"
    passes = {EC.sort_passes(k) for k, n in default if EC.sort_algorithm(n) == "onesweep"}
    assert passes == {3, 4, 5, 6, 7, 8}
    assert {2 * k % 8 for k in EC.SWEEP_KS} >= {0, 2, 4, 6} and {EC.sort_passes(k) for k in EC.SWEEP_KS} == set(range(1, 9))
    # the merge sort and the one-workgroup sort at every pass count as well (the comparison takes the bit range)
    assert {EC.sort_passes(k) for k, n in default if EC.sort_algorithm(n) == "merge"} == set(range(2, 9))
    assert {EC.copy_plan(n, "default")[0] for _, n in default} == {"direct", "bounced"}
    assert EC.copy_plan(1_398_101, "default") == ("direct", 0, 1_398_101 * 48) and EC.copy_plan(1_398_102, "default") == ("bounced", 5, 32)
    assert EC.copy_plan(2_097_152, "default") == ("bounced", 6, 16 << 20) and EC.copy_plan(1_048_576, "default") == ("direct", 0, 48 << 20)
    assert EC.copy_plan(0, "bounced")[0] == "direct" and EC.copy_plan(1, "bounced") == ("bounced", 1, 48) and EC.copy_plan(256, "host_sort_bounced") == ("bounced", 3, 4096)
    assert EC.copy_plan(65537, "bounced") == ("bounced", 769, 48) and EC.copy_plan(65537, "host_sort") == ("direct", 0, 65537 * 48)


def test_copy_labels_are_the_librarys_plan(tmp_path):
    exe = build_export_plan(str(tmp_path / "export_plan"), sanitize=False)
    sizes = sorted({n for _, n, _ in CASES})
    for sub, mode in (("plan", "default"), ("testplan", "bounced")):
        out = subprocess.run([exe, sub] + [str(n * EC.ENTRY_BYTES) for n in sizes], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
        for n, line in zip(sizes, out):
            nbytes, bounced, chunks, last = (int(x) for x in line.split())
            assert nbytes == n * EC.ENTRY_BYTES
            assert EC.copy_plan(n, mode) == ("bounced" if bounced else "direct", chunks, last), (n, mode, line)
