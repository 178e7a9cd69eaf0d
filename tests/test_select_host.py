"""The kernel selector (kreeq_amd/csrc/kq_select_host.h: which instantiation of k_p1_hist, k_p1_scatter*, k_lv_*, k_count_regions*
and k_lookup_regions a handle gets) as a stand-alone host program under -fsanitize=address,undefined.  tests/native/select_main.cpp
holds the table, written out by hand from the launch ladders the selector replaced: k in {15, 21, 25, 30, 31}, full / partial /
non-power-of-two map range, window, owner mode with and without lockstep bytes, fan-outs on both sides of 512, region starts, even
buckets, offset matrix, every KQ_OPT_KERNEL_SET bit and 1 | 128.

The launcher lists of kreeq_amd.hip and the table name the same instantiations, and this test is how the two are compared: the
program prints every descriptor its table expects as "ROW <row maker> <template arguments>", the test reads the row makers
(p1h<6, 21>() ...) out of kreeq_amd.hip, replaces the constants' names by their values, and asks for equal sets per family and
for the number of instantiations per family that the device code has (14 k_p1_hist, 22 k_p1_scatter, 12 k_p1_scatter_s, ...)."""
import os
import re
import shutil
import subprocess

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "kreeq_amd", "csrc")
# kq_formats.h, and the default of KQ_P1S_TPR in kq_kernels.h
VALUES = {"FMT_PACK8": 0, "FMT_WIDE": 1, "FMT_NARROW": 2, "FMT_PACK8_TO_NARROW": 3, "FMT_TOP8": 4, "FMT_NARROW_TO_TIGHT": 6, "NB_MAX": 2048,
          "KQ_P1S_TPR": 2, "true": 1, "false": 0}
# row maker -> (kernel, instantiations of it in the device code)
FAMILIES = {"p1h": ("k_p1_hist", 14), "p1w": ("k_p1_scatter", 22), "p1s": ("k_p1_scatter_s", 12), "p1c": ("k_p1_scatter_c", 2), "lvh": ("k_lv_hist", 4),
            "lvw": ("k_lv_scatter", 11), "lvs": ("k_lv_scatter_s", 2), "p3g": ("k_count_regions", 7), "p3q": ("k_count_regions_q4", 4),
            "p3r": ("k_count_regions_q4r", 4), "lkr": ("k_lookup_regions", 4)}


def launcher_rows():
    src = open(os.path.join(CSRC, "kreeq_amd.hip")).read()
    rows = []
    for maker, args in re.findall(r"\b(%s)<([^<>]*)>\(\)" % "|".join(FAMILIES), src):
        vals = [VALUES[a] if a in VALUES else int(a) for a in (t.strip() for t in args.split(","))]
        if maker == "p1s" and len(vals) == 3:
            vals.append(0)                      # TOP8 = false
        rows.append((maker, tuple(vals)))
    return rows


def test_selector_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "select")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "select_main.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures" in p.stdout
    table = {(m.group(1), tuple(int(v) for v in m.group(2).split(","))) for m in re.finditer(r"^ROW (\w+) ([\d,]+)$", p.stdout, re.M)}
    listed = launcher_rows()
    assert len(listed) == len(set(listed)), "an instantiation is listed twice"
    for maker, (kernel, n) in FAMILIES.items():
        in_table = sorted(r for r in table if r[0] == maker)
        in_lists = sorted(r for r in listed if r[0] == maker)
        assert in_lists == in_table, "%s: launcher list and selector table differ" % kernel
        assert len(in_lists) == n, "%s: %d instantiations listed" % (kernel, len(in_lists))
    assert len(table) == sum(n for _, n in FAMILIES.values())
