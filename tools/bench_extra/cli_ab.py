"""Another build's `kreeq` against this tree's on the CLI scripts of this directory (cli_ingest.py, cli_db.py, cli_vcf_scale.py),
alternating in one process so that both see the same machine: each script is run REPS times per build as a child process in
which `build.CLI` names that build's binary (the other binary must find libkreeq_amd.so through its own rpath), and the figures
it prints are collected.  Per script one <out>/cli_<name>_ab.json: every value, and median / min / max per build and label.
cli_tables.py has its own --parent mode.  Stops at the first child that fails.

  python tools/bench_extra/cli_ab.py --parent PATH --out DIR [--reps 3] ingest db vcf"""
import argparse
import json
import os
import re
import runpy
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from kreeq_amd import build  # noqa: E402

# name -> (script, its arguments, (label, figure) of an output line)
TOOLS = {
    "ingest": ("cli_ingest.py", [], r"^(-j \w+): ingest \+ count \+ summary (\d+) ms"),                # best of the script's three runs, ms
    "db": ("cli_db.py", [], r"^(wall) ([\d.]+) s"),                                                   # each of the script's three runs, s
    "vcf": ("cli_vcf_scale.py", ["1", "10"], r"^(scale \d+) host search: wall ([\d.]+) s"),           # both host runs per scale, s
}

if len(sys.argv) > 1 and sys.argv[1] == "--child":                     # --child EXE SCRIPT ARGS: the script with build.CLI = EXE
    build.CLI = sys.argv[2]
    sys.argv = sys.argv[3:]
    runpy.run_path(sys.argv[0], run_name="__main__")
    sys.exit(0)

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True)
ap.add_argument("--out", required=True)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("tools", nargs="+", choices=sorted(TOOLS))
ARGS = ap.parse_args()
os.makedirs(ARGS.out, exist_ok=True)
for name in ARGS.tools:
    script, args, pat = TOOLS[name]
    values = {"parent": {}, "new": {}}
    for rep in range(ARGS.reps):
        for which, exe in (("parent", os.path.abspath(ARGS.parent)), ("new", build.CLI)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", exe, os.path.join(HERE, script)] + args, capture_output=True, text=True, timeout=600)
            print("%s %s run %d: rc %d" % (name, which, rep, p.returncode), flush=True)
            if p.returncode != 0:
                print(p.stderr[-2000:], flush=True)
                sys.exit(1)                                             # nothing more on the GPU after a failure
            for label, v in re.findall(pat, p.stdout, re.M):
                values[which].setdefault(label, []).append(float(v))
    summary = {w: {label: {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} for label, v in d.items()} for w, d in values.items()}
    json.dump({"tool": "tools/bench_extra/" + script, "args": args, "invocations_per_build": ARGS.reps, "values": values, "summary": summary},
              open(os.path.join(ARGS.out, "cli_%s_ab.json" % name), "w"), indent=1)
    for label, a in summary["parent"].items():
        b = summary["new"][label]
        print("%s %s: parent median %g (%g-%g), new median %g (%g-%g): %s the parent's spread" % (
            name, label, a["median"], a["min"], a["max"], b["median"], b["min"], b["max"],
            "inside" if a["min"] <= b["median"] <= a["max"] else "below" if b["median"] < a["min"] else "ABOVE"), flush=True)
