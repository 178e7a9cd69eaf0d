#!/usr/bin/env python3
"""Which kernels the count and lookup paths launch, case by case: a walk over k, table geometry, map range, bucket window,
KQ_OPT_COUNT_MAP_PASSES, KQ_OPT_PENDING_BYTES, every KQ_OPT_KERNEL_SET bit and the record entry points, on inputs of a few tens of
thousands of bases (count_path / lookup_path = partitioned force the partitioned paths at any size).  Two commits launch the same
kernels when their lists are equal.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/bench_extra/selection_trace.py run LABELS.txt
  python3 tools/bench_extra/selection_trace.py lists DIR/.../*_kernel_trace.csv LABELS.txt > kernels.txt

`run` writes one label per case and launches a marker kernel (torch's erfinv, which nothing else here uses) ahead of each, then
syncs; `lists` cuts the trace at the markers and prints, in a compact form, every case's label with the library's kernels in
launch order."""
import csv
import re
import sys

import numpy as np

MAPS = 128
# capacity hint, KQ_OPT_NARROW_MID: slots = hint / 0.7, regions = slots / 2048 (a multiple of 256 from 2048 regions, and for k >= 29)
TABLES = {"coarse<512": (400_000, 0),           # below 2048 regions, fewer than 512 first-level bins
          "coarse>=512": (1_430_000, 0),        # below 2048 regions, 512 .. 2047 first-level bins
          "bucket": (2_935_000, 0),             # 2048 regions: hash-prefix buckets, one level
          "bucket+mid": (2_935_000, 2),         # ... with a middle level
          "tight": (93_585_409, 0),             # 2^16 regions with region starts: tight records for k <= 21
          "tight+mid": (93_585_409, 16)}        # ... with a middle level: the last level has both forms


def reads(n_reads=250, length=150, seed=7):
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, 20_000, dtype=np.uint8)
    starts = rng.integers(0, len(genome) - length + 1, n_reads)
    chars = np.frombuffer(b"ACGT", dtype=np.uint8)[genome[starts[:, None] + np.arange(length)[None, :]]]
    return b"\n".join(r.tobytes() for r in chars), np.frombuffer(b"ACGT", dtype=np.uint8)[genome[:3000]].tobytes()


def run(label_path):
    import torch

    import kreeq_amd as kq

    batch, genome = reads()
    labels = open(label_path, "w")
    marker = torch.full((64,), 0.5, device="cuda")
    resident = torch.frombuffer(bytearray(batch), dtype=torch.uint8).cuda()
    open_dbs = []

    def table(k, name, maps=MAPS, **opts):
        hint, mid = TABLES[name]
        db = kq.KreeqDB(k, maps, capacity_hint=hint)
        open_dbs.append(db)
        db.set_option("count_path", "partitioned")
        db.set_option("lookup_path", "partitioned")
        db.set_option("trust_capacity", 1)
        if mid:
            db.set_option("narrow_mid", mid)
        for o, v in opts.items():
            db.set_option(o, v)
        return db

    def case(label, fn):
        """label, marker, the case, sync; a case the library refuses is named in the label file (the same way at any commit)"""
        torch.cuda.synchronize()
        marker.erfinv_()
        torch.cuda.synchronize()
        try:
            fn()
            outcome = ""
        except kq.KqError as e:
            outcome = "   REFUSED: %s" % e
        for db in open_dbs:
            try:
                db.sync()
            except kq.KqError as e:
                outcome += "   SYNC REFUSED: %s" % e
            db.close()
        del open_dbs[:]
        torch.cuda.synchronize()
        print(label + outcome, flush=True)
        labels.write(label + outcome + "\n")
        labels.flush()

    # 1. count at every k class on every geometry
    for k in (15, 21, 25, 30, 31):
        for name in TABLES:
            case("count k=%d %s" % (k, name), lambda: table(k, name).count_batch(batch))
    # 2. filters, windows, shared histograms and the pending arena on the bucketed tables
    for k in (21, 31):
        window = "bucket_window" if k == 21 else "shard_window"
        for name in ("bucket", "bucket+mid", "tight", "tight+mid"):
            tag = "k=%d %s" % (k, name)
            case("count %s maps [0,64) of 128" % tag, lambda: table(k, name, count_map_range=(0, 64)).count_batch(batch))
            case("count %s maps [0,50) of 100" % tag, lambda: table(k, name, maps=100, count_map_range=(0, 50)).count_batch(batch))
            case("count %s window [64,128)" % tag, lambda: table(k, name, **{window: 64 | (128 << 16)}).count_batch(batch))

            def two_passes():
                db = table(k, name, count_map_passes=2)
                for rng in ((0, 64), (64, 128)):
                    db.set_option("count_map_range", rng)
                    db.count_batch_dev(resident.data_ptr(), resident.numel())
            case("count %s count_map_passes=2, two map ranges of a resident batch" % tag, two_passes)

            def two_windows():
                db = table(k, name, count_map_passes=2, **{window: 0 | (128 << 16)})
                db.count_batch_dev(resident.data_ptr(), resident.numel())
                db.sync()
                db.clear()
                db.set_option(window, 128 | (256 << 16))
                db.count_batch_dev(resident.data_ptr(), resident.numel())
            case("count %s count_map_passes=2, two windows of a resident batch" % tag, two_windows)
            for pending in (0, -1):
                def twice():
                    db = table(k, name, pending_bytes=pending)
                    db.count_batch(batch)
                    db.count_batch(batch)
                case("count %s pending_bytes=%d, two batches" % (tag, pending), twice)
    # 3. every alternative kernel, full and half map range
    for mask in (1, 2, 4, 16, 32, 64, 128):
        for name in ("bucket+mid", "tight", "tight+mid"):
            for rng in ((0, 128), (0, 64)):
                case("count k=21 %s kernel_set=%d maps [%d,%d)" % (name, mask, rng[0], rng[1]),
                     lambda: table(21, name, kernel_set=mask, count_map_range=rng).count_batch(batch))
    # 4. the record entry points
    for k in (21, 31):
        for name in ("coarse<512", "coarse>=512", "tight"):
            def insert_host():
                keys, edges = table(k, "coarse<512").emit_records(batch)
                table(k, name).insert_records(keys, edges)
            case("insert_records k=%d %s" % (k, name), insert_host)
    n = resident.numel()
    for k in (21, 25):
        for name in ("coarse>=512", "bucket", "bucket+mid", "tight"):
            for pending in (0, -1):
                def packed():
                    recs = torch.empty(n, dtype=torch.int64, device="cuda")
                    counts = table(k, "coarse<512").emit_packed_dev(resident.data_ptr(), n, 3, recs.data_ptr(), n)
                    db = table(k, name, pending_bytes=pending)
                    for _ in range(2):
                        db.insert_packed_dev(recs.data_ptr(), int(counts.sum()))
                case("emit_packed_dev (3 parts) + insert_packed_dev k=%d %s pending_bytes=%d" % (k, name, pending), packed)
    for k in (21, 31):
        def partitioned():
            keys = torch.empty(n, dtype=torch.int64, device="cuda")
            edges = torch.empty(n, dtype=torch.uint8, device="cuda")
            counts = table(k, "coarse<512").emit_partitioned_dev(resident.data_ptr(), n, 3, keys.data_ptr(), edges.data_ptr(), n)
            table(k, "bucket").insert_records_dev(keys.data_ptr(), edges.data_ptr(), int(counts.sum()))
        case("emit_partitioned_dev (3 parts) + insert_records_dev k=%d" % k, partitioned)
    cut = batch.rfind(b"\n", 0, len(batch) // 2)
    halves = [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() for b in (batch[:cut], batch[cut + 1:])]
    for k, name in ((21, "bucket"), (21, "bucket+mid"), (21, "tight"), (31, "bucket"), (31, "bucket+mid")):
        def sharded():
            five = k == 21
            sender = table(k, "coarse<512")
            runs, metas = [], []
            for t in halves:
                recs = torch.empty(t.numel(), dtype=torch.int32 if five else torch.int64, device="cuda")
                aux = torch.empty(t.numel(), dtype=torch.uint8, device="cuda")
                meta = torch.empty((2, 256), dtype=torch.int64, device="cuda")
                if five:
                    counts = sender.emit_sharded_dev(t.data_ptr(), t.numel(), 2, recs.data_ptr(), aux.data_ptr(), recs.numel(), meta.data_ptr())
                else:
                    counts = sender.emit_sharded8_dev(t.data_ptr(), t.numel(), 2, recs.data_ptr(), recs.numel(), meta.data_ptr())
                off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
                runs.append([(recs[off[p]:off[p + 1]], aux[off[p]:off[p + 1]]) for p in range(2)])
                metas.append(meta)
            for p in range(2):
                db = table(k, name, **{"bucket_window" if five else "shard_window": (128 * p) | ((128 * p + 128) << 16)})
                r = torch.cat([run[p][0] for run in runs])
                a = torch.cat([run[p][1] for run in runs])
                m = torch.stack([meta[p] for meta in metas]).contiguous()
                torch.cuda.synchronize()              # (the library works on its own stream)
                for _ in range(2):
                    if five:
                        db.insert_sharded_dev(r.data_ptr(), a.data_ptr(), r.numel(), 2, m.data_ptr())
                    else:
                        db.insert_sharded8_dev(r.data_ptr(), r.numel(), 2, m.data_ptr())
        case("emit_sharded%s_dev + insert_sharded%s_dev, 2 peers, 2 parts, k=%d %s" % ("" if k == 21 else "8", "" if k == 21 else "8", k, name), sharded)
    # 5. region-wise lookup, counters only
    for k in (15, 21, 25, 30, 31):
        for name in ("coarse<512", "bucket", "tight+mid"):
            def lookup():
                db = table(k, name)
                db.count_batch(batch)
                db.lookup_sequence(genome)
                db.lookup_sequence(genome, map_lo=0, map_hi=64)
            case("count + lookup_sequence at maps [0,128) and [0,64) k=%d %s" % (k, name), lookup)
    case("end", lambda: None)
    labels.close()


def lists(trace_csv, label_path):
    labels = [l.rstrip("\n") for l in open(label_path)]
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    cases, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "erfinv" in name:
            cur = []
            cases.append(cur)
        elif cur is not None and re.match(r"(void )?k_\w+", name):
            cur.append(re.sub(r"^void ", "", name).split("(")[0])
    assert len(cases) == len(labels), "%d markers in the trace, %d labels" % (len(cases), len(labels))
    # compact and still exact: the kernels' names once, numbered in sorted order; every distinct launch sequence once (S1, S2 ...
    # in the order of first use; `7x3` = kernel 7 three times in a row); then the sequence of every case.  Equal files = equal
    # ordered kernel lists, case by case
    number = {name: i + 1 for i, name in enumerate(sorted({k for kernels in cases for k in kernels}))}
    for name, i in number.items():
        print("%d = %s" % (i, name))
    seqs = {}
    for kernels in cases:
        text = run_lengths([number[k] for k in kernels])
        if text not in seqs:
            seqs[text] = "S%d" % (len(seqs) + 1)
            print("%s (%d launches): %s" % (seqs[text], len(kernels), text))
    for label, kernels in zip(labels, cases):
        print("== %s: %s" % (label, seqs[run_lengths([number[k] for k in kernels])]))


def run_lengths(items):
    runs = []
    for it in items:
        if runs and runs[-1][0] == it:
            runs[-1][1] += 1
        else:
            runs.append([it, 1])
    return " ".join(str(it) if n == 1 else "%sx%d" % (it, n) for it, n in runs)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "lists":
        lists(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
