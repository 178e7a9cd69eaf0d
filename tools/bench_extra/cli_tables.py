"""Times `kreeq validate -d db -f asm -o x.<ext>` (per-base tables) on a synthetic assembly with the host
writers, with the device formatter (KQ_TABLE_DEVICE=1) and, when --parent names one, with another build's `kreeq` binary
(it must find libkreeq_amd.so through its own rpath), alternating in one process so that the three see the same machine.
.bkwig and .kwig at --mbp, .csvtable on the first 20 Mbp; output to /dev/null (through a symlink with the extension), then
.bkwig and .kwig once each to a file under --work, compared byte for byte.  Every run is one JSON line on stdout (wall clock
and the KQ_TABLE_TRACE line) and an entry of <out>/cli_tables.json.

  python tools/bench_extra/cli_tables.py --out DIR [--mbp 100] [--parent PATH] [--work /tmp/kq_table_bench]"""
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
ap.add_argument("--parent", default="")
ap.add_argument("--work", default="/tmp/kq_table_bench")
ARGS = ap.parse_args()
NEW, PARENT = os.path.join(ROOT, "kreeq_amd", "bin", "kreeq"), ARGS.parent
WORK, OUT = ARGS.work, ARGS.out
MBP, SEQ = ARGS.mbp, 1_000_000
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
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=limit, env=env)
    dt = time.time() - t0
    trace = [l for l in p.stderr.split("\n") if l.startswith("[table]")]
    rec = {"tag": tag, "wall_s": round(dt, 3), "rc": p.returncode, "trace": trace}
    results.append(rec)
    print(json.dumps(rec), flush=True)
    json.dump(results, open(os.path.join(OUT, "cli_tables.json"), "w"), indent=1)
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
    run("qv_only", NEW, ["validate", "-d", WORK + "/db.kreeq", "-f", WORK + "/asm.fasta"], {}, 300)       # what a run costs without any table
    for ext in ("kwig", "bkwig", "csvtable"):
        os.symlink("/dev/null", WORK + "/null." + ext)
    summary = {}
    for ext, asm_file, reps in (("bkwig", "asm.fasta", 3), ("kwig", "asm.fasta", 3), ("csvtable", "asm20.fasta", 2)):
        args = ["validate", "-d", WORK + "/db.kreeq", "-f", WORK + "/" + asm_file, "-o", WORK + "/null." + ext]
        times = {"device": [], "host": [], "parent": []}
        for r in range(reps):                                             # alternating, in one call
            times["device"].append(run("%s device null %d" % (ext, r), NEW, args, {"KQ_TABLE_DEVICE": "1"}, 600))
            times["host"].append(run("%s host null %d" % (ext, r), NEW, args, {}, 900))
            if PARENT:
                times["parent"].append(run("%s parent null %d" % (ext, r), PARENT, args, {}, 900))
        summary[ext] = {k: {"median_s": round(statistics.median(v), 3), "runs": [round(x, 3) for x in v]} for k, v in times.items() if v}
        print("SUMMARY", ext, json.dumps(summary[ext]), flush=True)
    # to a file on local disk: one run each
    for ext in ("bkwig", "kwig"):
        for mode, env in (("device", {"KQ_TABLE_DEVICE": "1"}), ("host", {})):
            path = WORK + "/out." + mode + "." + ext
            summary["%s file %s" % (ext, mode)] = run("%s %s file" % (ext, mode), NEW, ["validate", "-d", WORK + "/db.kreeq", "-f", WORK + "/asm.fasta", "-o", path], env, 900)
            summary["%s file %s bytes" % (ext, mode)] = os.path.getsize(path)
        same = subprocess.run(["cmp", WORK + "/out.device." + ext, WORK + "/out.host." + ext]).returncode == 0
        summary["%s file identical" % ext] = same
        print("IDENTICAL", ext, same, flush=True)
        os.remove(WORK + "/out.device." + ext)
        os.remove(WORK + "/out.host." + ext)
    json.dump({"runs": results, "summary": summary}, open(os.path.join(OUT, "cli_tables.json"), "w"), indent=1)
    shutil.rmtree(WORK, ignore_errors=True)


if __name__ == "__main__":
    try:
        main()
    finally:
        shutil.rmtree(WORK, ignore_errors=True)
