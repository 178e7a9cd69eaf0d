"""Times `kreeq validate -d db -f asm -o null.<ext> --passes N` (per-base tables under map-range passes) on
the synthetic assembly of cli_tables.py, with three arms alternating in one process so that they see the same machine: the
table accumulated on the device (KQ_TABLE_DEVICE=1 KQ_TABLE_DEVICE_PASSES=1), this build's host writer, and, when --parent
names one, another build's `kreeq` binary (it must find libkreeq_amd.so through its own rpath).  .bkwig and .kwig at --mbp,
.csvtable on the first 20 Mbp, each at --passes 2 and 4; one warm-up round, then --rounds alternating rounds; output to
/dev/null (through a symlink with the extension).  Every run is one JSON line on stdout (wall clock and the KQ_TABLE_TRACE
line) and an entry of <out>/cli_tables_passes.json; a SUMMARY line per format and pass count gives median and range per arm.
Last, .bkwig and .kwig once each to a file under --work from the device arm and the host arm, compared byte for byte.

  python tools/bench_extra/cli_tables_passes.py --out DIR [--mbp 100] [--rounds 3] [--parent PATH] [--work /tmp/kq_table_passes_bench] [--rocprof DIR]"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from kreeq_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--mbp", type=int, default=100)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--formats", default="bkwig,kwig,csvtable")
ap.add_argument("--passes", default="2,4")
ap.add_argument("--parent", default="")
ap.add_argument("--rocprof", default="", help="directory for one extra .bkwig run of the device arm under rocprofv3 --kernel-trace --stats")
ap.add_argument("--work", default="/tmp/kq_table_passes_bench")
ARGS = ap.parse_args()
NEW, PARENT = os.path.join(ROOT, "kreeq_amd", "bin", "kreeq"), ARGS.parent
WORK, OUT = ARGS.work, ARGS.out
MBP, SEQ = ARGS.mbp, 1_000_000
DEVICE_ENV = {"KQ_TABLE_DEVICE": "1", "KQ_TABLE_DEVICE_PASSES": "1"}
results = []


def fasta(path, codes_list, prefix):
    with open(path, "wb") as f:
        for i, c in enumerate(codes_list):
            f.write(b">%s%d\n" % (prefix, i))
            f.write(synth.codes_to_ascii(c).tobytes())
            f.write(b"\n")


def run(tag, exe, args, env_extra, limit):
    env = dict(os.environ, KQ_DB_DEVICE="1", KQ_TABLE_TRACE="1", **env_extra)
    t0 = time.time()
    p = subprocess.run([exe] + args + ["--verbose"], capture_output=True, text=True, timeout=limit, env=env)
    dt = time.time() - t0
    trace = [l for l in p.stderr.split("\n") if l.startswith("[table]")]
    side = [l.split("] ", 1)[-1] for l in p.stderr.split("\n") if "per-base table" in l]
    rec = {"tag": tag, "wall_s": round(dt, 3), "rc": p.returncode, "trace": trace, "side": side}
    results.append(rec)
    print(json.dumps(rec), flush=True)
    json.dump(results, open(os.path.join(OUT, "cli_tables_passes.json"), "w"), indent=1)
    if p.returncode != 0:
        print(p.stderr[-2000:], flush=True)
        sys.exit(1)                                                       # nothing more on the GPU after a failure
    return dt


def main():
    os.makedirs(OUT, exist_ok=True)
    shutil.rmtree(WORK, ignore_errors=True)
    os.makedirs(WORK)
    t0 = time.time()
    g = synth.genome_codes(MBP * SEQ, seed=1)
    asm = synth.mutate(g, 0.001, seed=5)
    fasta(WORK + "/asm.fasta", [asm[i:i + SEQ] for i in range(0, len(asm), SEQ)], b"chr")
    fasta(WORK + "/asm20.fasta", [asm[i:i + SEQ] for i in range(0, min(20, MBP) * SEQ, SEQ)], b"chr")
    with open(WORK + "/reads.fasta", "wb") as f:
        for c in range(8):
            r = synth.mutate(g, 0.001, seed=10 + c)
            for i in range(0, len(r), SEQ):
                f.write(b">r%d_%d\n" % (c, i))
                f.write(synth.codes_to_ascii(r[i:i + SEQ]).tobytes())
                f.write(b"\n")
    print("inputs written in %.1f s" % (time.time() - t0), flush=True)
    run("build_db", NEW, ["validate", "-r", WORK + "/reads.fasta", "-o", WORK + "/db.kreeq"], {}, 600)
    formats = [f for f in ARGS.formats.split(",") if f]
    for ext in formats:
        os.symlink("/dev/null", WORK + "/null." + ext)
    arms = [("device", NEW, DEVICE_ENV), ("host", NEW, {})] + ([("parent", PARENT, {})] if PARENT else [])
    summary = {}
    for passes in [int(p) for p in ARGS.passes.split(",")]:
        run("qv_only passes %d" % passes, NEW, ["validate", "-d", WORK + "/db.kreeq", "-f", WORK + "/asm.fasta", "--passes", str(passes)], {}, 600)      # what the ranges cost without any table
        for ext in formats:
            asm_file = "asm20.fasta" if ext == "csvtable" else "asm.fasta"
            args = ["validate", "-d", WORK + "/db.kreeq", "-f", WORK + "/" + asm_file, "-o", WORK + "/null." + ext, "--passes", str(passes)]
            times = {a[0]: [] for a in arms}
            for r in range(-1, ARGS.rounds):                              # round -1 warms up; the arms alternate inside a round
                for arm, exe, env in arms:
                    dt = run("%s passes %d %s null %d" % (ext, passes, arm, r), exe, args, env, 900)
                    if r >= 0:
                        times[arm].append(dt)
            key = "%s passes %d" % (ext, passes)
            summary[key] = {k: {"median_s": round(statistics.median(v), 3), "min_s": round(min(v), 3), "max_s": round(max(v), 3)} for k, v in times.items() if v}
            print("SUMMARY", key, json.dumps(summary[key]), flush=True)
    # to a file on local disk: one run each, compared
    for ext in [f for f in ("bkwig", "kwig") if f in formats]:
        for arm, env in (("device", DEVICE_ENV), ("host", {})):
            path = WORK + "/out." + arm + "." + ext
            run("%s passes 2 %s file" % (ext, arm), NEW, ["validate", "-d", WORK + "/db.kreeq", "-f", WORK + "/asm.fasta", "-o", path, "--passes", "2"], env, 900)
        same = subprocess.run(["cmp", WORK + "/out.device." + ext, WORK + "/out.host." + ext]).returncode == 0
        summary["%s file identical" % ext] = same
        print("IDENTICAL", ext, same, flush=True)
        os.remove(WORK + "/out.device." + ext)
        os.remove(WORK + "/out.host." + ext)
    json.dump({"runs": results, "summary": summary}, open(os.path.join(OUT, "cli_tables_passes.json"), "w"), indent=1)
    if ARGS.rocprof:                                                      # kernel times (k_tab_merge, k_lookup): a run of its own, nothing else traced
        args = ["validate", "-d", WORK + "/db.kreeq", "-f", WORK + "/asm.fasta", "-o", WORK + "/null.bkwig", "--passes", "2"]
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", ARGS.rocprof, "-o", "passes2_bkwig", "--", NEW] + args,
                           capture_output=True, text=True, timeout=900, env=dict(os.environ, KQ_DB_DEVICE="1", **DEVICE_ENV))
        print("ROCPROF rc", p.returncode, p.stderr[-500:] if p.returncode else "", flush=True)


if __name__ == "__main__":
    try:
        main()
    finally:
        shutil.rmtree(WORK, ignore_errors=True)
