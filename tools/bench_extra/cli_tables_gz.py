"""Times `kreeq validate -d db -f asm -o x.<ext>.gz` (BGZF per-base tables) on the synthetic assembly of
tools/bench_extra/cli_tables.py: the device formatter + device deflater (KQ_TABLE_DEVICE=1), this build's host writer through zlib,
this build's plain `-o x.<ext>` under KQ_TABLE_DEVICE=1 and, when --parent names one, the parent build's plain `-o x.<ext>` under
KQ_TABLE_DEVICE=1 (what compression adds or saves in copy and write time), alternating in one process.  .kwig at --mbp, .csvtable
on the first 20 Mbp, .kwig once more with --passes 2 on the accumulator path; output to /dev/null through a symlink with the
extension.  Then .kwig.gz and .csvtable.gz once each to a file under --work: gzip-checked member by member against the plain
device file's bytes, and their size against Python zlib level 1 (raw deflate of the same 0xff00-byte pieces + 26 bytes each) over
the first --ratio-mib of text.  Every run is one JSON line on stdout and an entry of <out>/cli_tables_gz.json.

  python tools/bench_extra/cli_tables_gz.py --out DIR [--mbp 100] [--parent PATH] [--work /tmp/kq_table_gz_bench]"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from kreeq_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--mbp", type=int, default=100)
ap.add_argument("--parent", default="")
ap.add_argument("--work", default="/tmp/kq_table_gz_bench")
ap.add_argument("--ratio-mib", type=int, default=256)
ARGS = ap.parse_args()
NEW, PARENT = os.path.join(ROOT, "kreeq_amd", "bin", "kreeq"), ARGS.parent
WORK, OUT = ARGS.work, ARGS.out
MBP, SEQ = ARGS.mbp, 1_000_000
DEV, BOTH = {"KQ_TABLE_DEVICE": "1"}, {"KQ_TABLE_DEVICE": "1", "KQ_TABLE_DEVICE_PASSES": "1"}
results = []


def fasta(path, codes_list, prefix):
    with open(path, "wb") as f:
        for i, c in enumerate(codes_list):
            f.write(b">%s%d\n" % (prefix, i))
            f.write(synth.codes_to_ascii(c).tobytes())
            f.write(b"\n")


def save(summary=None):
    json.dump({"runs": results, "summary": summary or {}}, open(os.path.join(OUT, "cli_tables_gz.json"), "w"), indent=1)


def run(tag, exe, args, env_extra, limit):
    env = dict(os.environ, KQ_DB_DEVICE="1", KQ_TABLE_TRACE="1", **env_extra)
    t0 = time.time()
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=limit, env=env)
    dt = time.time() - t0
    rec = {"tag": tag, "wall_s": round(dt, 3), "rc": p.returncode, "trace": [l for l in p.stderr.split("\n") if l.startswith("[table]")]}
    results.append(rec)
    print(json.dumps(rec), flush=True)
    save()
    if p.returncode != 0:
        print(p.stderr[-2000:], flush=True)
        sys.exit(1)                                                       # nothing more on the GPU after a failure
    return dt


def ratio(gz_path, plain_path, limit):
    """members of gz_path over the first `limit` bytes of text: their size, zlib level 1's, and that they hold plain_path's bytes"""
    ours = ref = text_bytes = members = 0
    with open(gz_path, "rb") as f, open(plain_path, "rb") as g:
        while text_bytes < limit:
            head = f.read(18)
            if len(head) < 18:
                break
            size = int.from_bytes(head[16:18], "little") + 1
            body = f.read(size - 18)
            text = zlib.decompress(body[:-8], -15)
            assert g.read(len(text)) == text and int.from_bytes(body[-4:], "little") == len(text), "member %d differs from the plain file" % members
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            ref += len(c.compress(text) + c.flush()) + 26
            ours += size
            text_bytes += len(text)
            members += 1
    return {"text_bytes": text_bytes, "members": members, "gpu_bytes": ours, "zlib1_bytes": ref, "gpu_over_zlib1": round(ours / ref, 4), "gpu_over_text": round(ours / text_bytes, 4)}


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
    for ext in ("kwig", "csvtable", "kwig.gz", "csvtable.gz"):
        os.symlink("/dev/null", WORK + "/null." + ext)
    summary = {}
    for ext, asm_file, reps, extra, env in (("kwig", "asm.fasta", 3, [], DEV), ("csvtable", "asm20.fasta", 2, [], DEV), ("kwig", "asm.fasta", 2, ["--passes", "2"], BOTH)):
        base = ["validate", "-d", WORK + "/db.kreeq", "-f", WORK + "/" + asm_file] + extra
        gz, plain = base + ["-o", WORK + "/null." + ext + ".gz"], base + ["-o", WORK + "/null." + ext]
        key = ext + (" passes 2" if extra else "")
        times = {"gz device": [], "plain device": [], "plain device, parent": [], "gz host zlib": []}
        for r in range(reps):                                             # alternating, in one call
            times["gz device"].append(run("%s gz device %d" % (key, r), NEW, gz, env, 600))
            times["plain device"].append(run("%s plain device %d" % (key, r), NEW, plain, env, 600))
            if PARENT:
                times["plain device, parent"].append(run("%s plain device parent %d" % (key, r), PARENT, plain, env, 600))
            if r == 0 and not extra:
                times["gz host zlib"].append(run("%s gz host zlib" % key, NEW, gz, {}, 900))
        summary[key] = {k: {"median_s": round(statistics.median(v), 3), "runs": [round(x, 3) for x in v]} for k, v in times.items() if v}
        print("SUMMARY", key, json.dumps(summary[key]), flush=True)
        save(summary)
    for ext, asm_file in (("kwig", "asm.fasta"), ("csvtable", "asm20.fasta")):      # to a file: sizes and the ratio against zlib level 1
        base = ["validate", "-d", WORK + "/db.kreeq", "-f", WORK + "/" + asm_file]
        summary[ext + " file gz s"] = run("%s gz device file" % ext, NEW, base + ["-o", WORK + "/out." + ext + ".gz"], DEV, 900)
        summary[ext + " file plain s"] = run("%s plain device file" % ext, NEW, base + ["-o", WORK + "/out." + ext], DEV, 900)
        summary[ext + " file bytes"] = {"gz": os.path.getsize(WORK + "/out." + ext + ".gz"), "plain": os.path.getsize(WORK + "/out." + ext)}
        summary[ext + " ratio"] = ratio(WORK + "/out." + ext + ".gz", WORK + "/out." + ext, ARGS.ratio_mib << 20)
        print("RATIO", ext, json.dumps(summary[ext + " file bytes"]), json.dumps(summary[ext + " ratio"]), flush=True)
        os.remove(WORK + "/out." + ext + ".gz")
        os.remove(WORK + "/out." + ext)
        save(summary)


if __name__ == "__main__":
    try:
        main()
    finally:
        shutil.rmtree(WORK, ignore_errors=True)
