"""k_bgzf_inflate alone: one resident batch of about 64 MiB of FASTQ text as level-6 BGZF in 0xff00-byte blocks, six
kq_inflate_bgzf_dev calls.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_extra/bgzf_inflate.py` for the
kernel's own time (no counters in the same run): the durations of the k_bgzf_inflate dispatches in the kernel trace.  The wall
time per call printed here includes the descriptor upload, the launch and the status read-back."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import kreeq_amd
from kreeq_amd import capi
from tests import bgzf_inputs as B

TEXT_MIB, CALLS = 64, 6
piece = B.fastq_text(4 << 20, seed=1)                               # 4 MiB of records, repeated (every block is inflated on its own)
piece = piece[:piece.rindex(b"\n@read") + 1]
text = piece * ((TEXT_MIB << 20) // len(piece))
data = B.bgzf_file(text, level=6, eof=False)
blocks, used = capi.bgzf_scan(data)
assert used == len(data)
comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
out = torch.empty(len(text) + 64, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
db = kreeq_amd.KreeqDB(21, 128)
times = []
for _ in range(CALLS):
    t0 = time.perf_counter()
    n = db.inflate_bgzf_dev(comp.data_ptr(), len(data), blocks, out.data_ptr(), len(text))
    times.append(time.perf_counter() - t0)
assert n == len(text)
got = out[:n].cpu().numpy().tobytes()
assert got == text
times.sort()
med = (times[2] + times[3]) / 2
print(f"{len(blocks)} blocks, {len(data) / 2**20:.1f} MiB compressed -> {n / 2**20:.1f} MiB text; per call median {med * 1e3:.2f} ms "
      f"(min {times[0] * 1e3:.2f}, max {times[-1] * 1e3:.2f}) = {n / med / 1e9:.2f} GB/s of text")
db.close()
