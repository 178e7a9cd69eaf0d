"""k_bgzf_deflate alone: one resident text of about 64 MiB, six kq_deflate_bgzf_dev calls per text.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_extra/bgzf_deflate.py` for the kernels' own time (no counters in the same
run): the durations of the k_bgzf_deflate / k_bgzf_sizes_scan / k_bgzf_gather dispatches in the kernel trace.  The wall time per
call printed here includes the launches and the status read-back.  Texts: FASTQ records, and a .kwig table of values in runs.
Also prints the compressed size against Python zlib level 1 (raw deflate of the same 0xff00-byte pieces, 26 bytes of container
added per piece) on the first 16 MiB of each text."""
import gzip
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import kreeq_amd
from kreeq_amd import capi
from tests import bgzf_inputs as B

TEXT_MIB, CALLS, MEMBER = 64, 6, 0xff00


def kwig_text(n_bytes):
    """fixedStep lines cov,fw,bw of values in runs of 1..39 positions"""
    rng = np.random.default_rng(3)
    n = n_bytes // 6
    v = np.repeat(rng.integers(0, 60, (n // 20 + 1, 3)), rng.integers(1, 40, n // 20 + 1), axis=0)[:n]
    return b"21\nfixedStep chrom=chr1 start=0 step=1\n" + b"".join(b"%d,%d,%d\n" % (a, b, c) for a, b, c in v.tolist())


def zlib1(text):
    total = 0
    for i in range(0, len(text), MEMBER):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(c.compress(text[i:i + MEMBER]) + c.flush()) + 26
    return total


db = kreeq_amd.KreeqDB(21, 128)
for name, piece in (("fastq", B.fastq_text(4 << 20, seed=1)), ("kwig", kwig_text(4 << 20))):
    text = piece * ((TEXT_MIB << 20) // len(piece))
    src = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    cap = capi.bgzf_bound(len(text), capi.BGZF_EOF)
    out = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        n = db.deflate_bgzf_dev(src.data_ptr(), len(text), out.data_ptr(), cap, capi.BGZF_EOF)
        times.append(time.perf_counter() - t0)
    data = out[:n].cpu().numpy().tobytes()
    assert gzip.decompress(data[:len(data)]) == text
    times.sort()
    med = (times[2] + times[3]) / 2
    head = text[:16 << 20]
    ours = len(db.deflate_bgzf(head))
    ref = zlib1(head)
    print(f"{name}: {len(text) / 2**20:.1f} MiB text -> {n / 2**20:.1f} MiB BGZF ({n / len(text):.3f}); per call median {med * 1e3:.2f} ms "
          f"(min {times[0] * 1e3:.2f}, max {times[-1] * 1e3:.2f}) = {len(text) / med / 1e9:.2f} GB/s of text; first 16 MiB: {ours} bytes, "
          f"zlib level 1 {ref} bytes, ratio {ours / ref:.3f}", flush=True)
db.close()
