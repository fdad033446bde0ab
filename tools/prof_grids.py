#!/usr/bin/env python
"""Kernel time of bench.py's timed region per (kernel name, grid, workgroup).

tools/prof_window.py sums per kernel name, which merges every shape a conv
kernel runs at.  This keeps the launch geometry apart, so that the launches of
one shape (e.g. the RPN head's 3x3 backward at each FPN level) can be summed
before and after a change that gives them another kernel or another grid.

usage: prof_grids.py <rocprof out dir> <out csv> [--steps K] [--match REGEX]
"""
import argparse
import collections
import csv
import glob
import os
import re


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("out_csv")
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--range", default="timed_region")
    ap.add_argument("--match", default="conv|wgrad|row_|rows_")
    a = ap.parse_args()
    kt = glob.glob(os.path.join(a.outdir, "**", "*kernel_trace.csv"), recursive=True)
    mt = glob.glob(os.path.join(a.outdir, "**", "*marker_api_trace.csv"), recursive=True)
    assert kt, "no kernel trace"
    lo = hi = None
    for f in mt:
        for r in csv.DictReader(open(f)):
            if r.get("Function", "") == a.range or r.get("Message", "") == a.range:
                lo, hi = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    assert lo is not None, "marker range %r not found" % a.range
    pat = re.compile(a.match)
    agg = collections.defaultdict(lambda: [0, 0])
    for f in kt:
        for r in csv.DictReader(open(f)):
            s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            if not (lo <= s <= hi) or not pat.search(r["Kernel_Name"]):
                continue
            name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("d2mi::(anonymous namespace)::", ""))
            grid = "x".join(r.get(k, "1") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
            wg = "x".join(r.get(k, "1") for k in ("Workgroup_Size_X", "Workgroup_Size_Y",
                                                  "Workgroup_Size_Z"))
            g = agg[(name.replace("void ", ""), grid, wg)]
            g[0] += 1
            g[1] += e - s
    rows = sorted(agg.items(), key=lambda kv: -kv[1][1])
    with open(a.out_csv, "w", newline="") as fo:
        w = csv.writer(fo)
        w.writerow(["Name", "Grid", "Workgroup", "CallsPerStep", "AverageUs", "UsPerStep"])
        for (name, grid, wg), (n, t) in rows:
            w.writerow([name, grid, wg, round(n / a.steps, 3), round(t / n / 1e3, 2),
                        round(t / a.steps / 1e3, 2)])


if __name__ == "__main__":
    main()
