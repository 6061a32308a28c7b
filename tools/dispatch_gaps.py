#!/usr/bin/env python3
"""Kernel time and the gaps between consecutive dispatches of the plan kernel, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bench -- python bench.py --steps 100 ...
    python tools/dispatch_gaps.py DIR [TAG] [--first 59 --last 158]

Reads every *kernel_trace.csv under DIR, keeps the dispatches whose kernel name contains "lsc_plan" in start order and prints one JSON
line for dispatches --first..--last (the timed window of bench.py --steps 100: ticks 60-159): mean kernel time, and mean / median /
extremes of start[i+1] - end[i].  Under rocprofv3 the gaps carry the profiler's own interception; they compare two libraries, they are
not what an unprofiled run pays.  Needs no GPU.
"""
import argparse
import csv
import glob
import json


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("tag", nargs="?", default="")
    ap.add_argument("--first", type=int, default=59)
    ap.add_argument("--last", type=int, default=158)
    ap.add_argument("--kernel", default="lsc_plan", help="substring of the kernel name")
    a = ap.parse_args()
    files = glob.glob(a.dir + "/**/*kernel_trace.csv", recursive=True)
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    plan = [r for r in rows if a.kernel in r[2]]
    win = plan[a.first:a.last + 1]
    others = [r for r in rows if win and win[0][0] <= r[0] <= win[-1][0] and a.kernel not in r[2]]
    dur = [e - s for s, e, _ in win]
    gap = sorted(win[i + 1][0] - win[i][1] for i in range(len(win) - 1))
    us = lambda ns: round(ns / 1e3, 3)
    print(json.dumps({"tag": a.tag, "files": len(files), "dispatches": len(rows), "plan_dispatches": len(plan), "window": len(win),
                      "other_kernels_in_window": len(others), "kernel": win[0][2][:60] if win else None,
                      "kernel_mean_us": us(sum(dur) / max(len(dur), 1)), "gap_mean_us": us(sum(gap) / max(len(gap), 1)),
                      "gap_p50_us": us(gap[len(gap) // 2]) if gap else None, "gap_min_us": us(gap[0]) if gap else None,
                      "gap_max_us": us(gap[-1]) if gap else None}))


if __name__ == "__main__":
    main()
