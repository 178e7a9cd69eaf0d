"""k = 31 multi-GPU path rehearsed on one GPU: world size 1 over RCCL, a HiFi-shaped batch (reads of 15 kbp), the table sized
for it.  Three per-step times from ONE process on the same input and the same table:
  fused     kq_count_batch_dev, the single-GPU count
  sharded8  emit (8-byte hash-remainder records, bucket-sorted) -> all_to_all -> insert (levels start from the received runs)
  wide9     the key + edge byte path of small tables (ShardedCounter(force_wide=True)): owner split of its own, two arrays,
            two all-to-alls, the receiver hashes again
A step = clear, count one batch, flush (the table pass over what is pending belongs to the step), device synchronise; host
clock around it.  The blocks run fused, sharded8, wide9 and then wide9 AGAIN: the distance between the two wide9 medians is the
repeat spread inside a process.  Every block must leave the same table summary.  One JSON line on stdout (and --out).

  python tools/bench_extra/sharded8_rehearsal.py [--mbp 20] [--cov 60] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--mbp", type=float, default=20.0, help="genome size")
    ap.add_argument("--cov", type=float, default=60.0)
    ap.add_argument("--read-len", type=int, default=15000)
    ap.add_argument("--err", type=float, default=0.002)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="one block only (for a kernel trace): fused | sharded8 | wide9")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this measurement has no CPU form")

    from kreeq_amd import synth
    from kreeq_amd.dist import GpuEngine, ShardedCounter

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        g_len = int(a.mbp * 1e6)
        n_reads = int(g_len * a.cov / a.read_len)
        gen = torch.Generator(device=dev)
        gen.manual_seed(2)
        t = synth.reads_dev(synth.genome_dev(g_len, dev, seed=1), n_reads, a.read_len, gen, err=a.err, chunk=10_000)
        n_bases = t.numel()
        hint = int(1.15 * (g_len + n_bases * a.err * a.k)) + (1 << 22)      # distinct k-mers: the genome's + up to k per substitution
        st = torch.cuda.Stream()
        torch.cuda.set_stream(st)
        eng = GpuEngine(a.k, 128, 0, capacity_hint=hint)
        eng.db.set_option("trust_capacity", 1)
        assert eng.sharded8, "the table must have the bucket geometry (>= 2048 regions)"
        drivers = {"sharded8": ShardedCounter(eng, a.k, 128, sharded_path=True)}
        drivers["sharded8"].force_exchange = True
        eng.sharded8 = True
        drivers["wide9"] = ShardedCounter(eng, a.k, 128, sharded_path=True, force_wide=True)
        drivers["wide9"].force_exchange = True

        def step(name):
            eng.clear()
            if name == "fused":
                eng.count(t)
            else:
                eng.sharded8 = not drivers[name].force_wide
                with torch.cuda.stream(st):
                    drivers[name].count_batch(t)
            eng.flush()
            torch.cuda.synchronize(dev)

        def block(name):
            for _ in range(a.warmup):
                step(name)
            ms = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                step(name)
                ms.append((time.perf_counter() - t0) * 1e3)
            s = eng.db.summary()
            q = statistics.quantiles(ms, n=4)
            return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "q1_ms": q[0], "q3_ms": q[2],
                    "steps": len(ms), "total": s["total"], "distinct": s["distinct"]}

        order = [a.only] if a.only else ["fused", "sharded8", "wide9", "wide9"]
        res = {"k": a.k, "bases": n_bases, "reads": n_reads, "read_len": a.read_len, "capacity_hint": hint,
               "regions": eng.db.info()["slots_total"] // 2048, "chunks_per_step": None, "blocks": []}
        for name in order:
            r = block(name)
            r["path"] = name
            res["blocks"].append(r)
        sums = {(b["total"], b["distinct"]) for b in res["blocks"]}
        res["tables_agree"] = len(sums) == 1
        sc = drivers["sharded8"]
        res["chunks_per_step"] = max(sc.n_chunks, -(-n_bases // min(sc.MAX_CHUNK_BASES, sc.MAX_MESSAGE_BYTES // 8)))
        by = {}
        for b in res["blocks"]:
            by.setdefault(b["path"], []).append(b["median_ms"])
        if not a.only:
            res["sharded8_over_fused"] = by["sharded8"][0] / by["fused"][0]
            res["sharded8_over_wide9"] = by["sharded8"][0] / min(by["wide9"])
            res["wide9_repeat_spread"] = abs(by["wide9"][0] - by["wide9"][1]) / min(by["wide9"])
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        if not res["tables_agree"]:
            sys.exit("the paths left different tables")
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
