"""`kreeq validate -o vcf` with KQ_VCF_DEVICE=1: the candidate-error searches on the GPU (kq_search_variants) give the VCF
of the host search byte for byte -- on the reference's golden, on the random 30 kb case of tests/test_gpu_cli.py against the
oracle -- and the host search still runs outside the device limits and under map-range passes."""
import os
import subprocess

import numpy as np
import pytest

from kreeq_amd import build
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEVICE_LINE, HOST_LINE = "candidate-error search ran as the device search", "candidate-error search ran as the host search"


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(build.LIB), "libkreeq_amd.so must be built in-tree"
    return build.build_cli()


def run(cli, args, device=True, cwd=None):
    """-> (stdout lines without the empty tail, stderr)"""
    env = dict(os.environ)
    env.pop("KQ_VCF_DEVICE", None)
    if device:
        env["KQ_VCF_DEVICE"] = "1"
    p = subprocess.run([cli] + args + ["--verbose"], capture_output=True, text=True, timeout=300, env=env, cwd=cwd)
    assert p.returncode == 0, p.stderr
    out = p.stdout.split("\n")
    while out and out[-1] == "":
        out.pop()
    return out, p.stderr


def golden_args():
    argv, expected = H.parse_tst(os.path.join(H.GOLDEN, "validateFiles", "test.50.tst"))
    args = [H.golden_input(a) if a.startswith("testFiles/") else a for a in argv[1:]]
    return args, expected


def test_golden_replay(cli):
    args, expected = golden_args()
    got, err = run(cli, args)
    assert got == H.vcf_expected(expected)
    assert DEVICE_LINE in err and HOST_LINE not in err
    got, err = run(cli, args, device=False)                            # off by default
    assert got == H.vcf_expected(expected)
    assert HOST_LINE in err and DEVICE_LINE not in err


@pytest.fixture(scope="module")
def random_case(tmp_path_factory):
    """the 30 kb case of tests/test_gpu_cli.py::test_vcf_random_vs_oracle: planted substitutions, insertions and deletions
    (some close together), error-free reads at 12x -> (fasta, fastq, the oracle's VCF at depth 60 / span 20)"""
    from oracle import oracle as O
    from oracle import variants as V

    d = tmp_path_factory.mktemp("vcf_device")
    rng = np.random.default_rng(7)
    acgt = "ACGT"
    genome = "".join(acgt[i] for i in rng.integers(0, 4, 30000))
    reads = []
    for s in rng.integers(0, len(genome) - 150, 2400):
        r = genome[s:s + 150]
        if rng.random() < 0.5:
            r = r[::-1].translate(str.maketrans("ACGT", "TGCA"))
        reads.append(r)
    asm = list(genome)
    for p in sorted(rng.choice(np.arange(200, len(genome) - 200), 60, replace=False), reverse=True):
        kind = rng.integers(0, 3)
        if kind == 0:
            asm[p] = acgt[(acgt.index(asm[p]) + 1 + rng.integers(0, 3)) % 4].lower()
        elif kind == 1:
            del asm[p]
        else:
            asm.insert(p, acgt[rng.integers(0, 4)].lower())
    asm = "".join(asm)
    recs = [("chrA", asm[:14000]), ("chrB", asm[14000:20000] + "NNNN" + asm[20000:])]
    fa, fq = str(d / "asm.fasta"), str(d / "reads.fastq")
    with open(fa, "w") as f:
        for h, s in recs:
            f.write(f">{h}\n{s}\n")
    with open(fq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n")
    db = O.OracleDB(21, 128)
    db.count_batch("\n".join(reads).encode(), threads=4)
    want = V.correct_sequences(V.Graph(db.export(), 21), recs, 60, 20)
    assert len(want) > 4 + 30
    return fa, fq, want


def test_random_vs_oracle(cli, random_case):
    fa, fq, want = random_case
    got, err = run(cli, ["validate", "-f", fa, "-r", fq, "-o", "vcf", "--search-depth", "60", "--max-span", "20"])
    assert got == want
    assert DEVICE_LINE in err


def test_outside_the_limits_runs_the_host_search(cli, random_case):
    fa, fq, _ = random_case
    args = ["validate", "-f", fa, "-r", fq, "-o", "vcf", "--search-depth", "300", "--max-span", "20"]
    got, err = run(cli, args)
    assert HOST_LINE in err and DEVICE_LINE not in err
    default, _ = run(cli, args, device=False)
    assert got == default and len(got) > 4


def test_map_range_passes_run_the_host_search(cli, tmp_path):
    args, expected = golden_args()
    got, err = run(cli, args + ["--passes", "2"], cwd=str(tmp_path))
    assert got == H.vcf_expected(expected)
    assert HOST_LINE in err and DEVICE_LINE not in err
