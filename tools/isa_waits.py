#!/usr/bin/env python3
"""The LDS trips of a stretch of source in one kernel's ISA, in program order: a listing for latency work on a lone wave.

    hipcc <the Makefile's FLAGS> --cuda-device-only -gline-tables-only -S lsc_kernels.hip -o lsc_kernels.s
    python tools/isa_waits.py lsc_kernels.s _ZN3lsc19lsc_plan_alt_kernelILb0ELi1EEEvNS_8PlanArgsE 2450 2740 [--also 1856 1915]

Walks the kernel's body and follows the .loc directives (line tables do not change the code).  From the first to the last instruction
whose line lies in [first, last] it prints every ds_* instruction, every s_waitcnt that names lgkmcnt and every s_barrier with the line
it is booked under; --also names further ranges (helpers inlined into the stretch) whose lines count as inside.  Instructions booked under
other lines -- code the scheduler moved in -- are printed with a '~'.  Needs no GPU.
"""
import argparse
import re


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm"); ap.add_argument("kernel"); ap.add_argument("first", type=int); ap.add_argument("last", type=int)
    ap.add_argument("--also", type=int, nargs=2, action="append", default=[])
    ap.add_argument("--file", default="lsc_kernels.hip")
    a = ap.parse_args()
    files, body, inside = {}, [], False
    for ln in open(a.asm):
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', ln)
        if m:
            files[int(m.group(1))] = m.group(3) or m.group(2)
        if ln.startswith(a.kernel + ":"):
            inside = True
            continue
        if inside:
            if ln.startswith(".Lfunc_end"):
                break
            body.append(ln.rstrip())
    ranges = [(a.first, a.last)] + [tuple(r) for r in a.also]
    cur, rows = (None, 0), []
    for ln in body:
        m = re.match(r'\s*\.loc\s+(\d+)\s+(\d+)', ln)
        if m:
            cur = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        t = ln.strip()
        if not t or t.startswith((".", ";")) or t.endswith(":"):
            continue
        rows.append((cur, t.split(";")[0].strip()))
    main_in = [i for i, (c, _) in enumerate(rows) if c[0].endswith(a.file) and a.first <= c[1] <= a.last]
    if not main_in:
        raise SystemExit("no instruction of the range in this kernel")
    n_wait = n_ds = n_bar = 0
    for (f, line), t in rows[main_in[0]:main_in[-1] + 1]:
        op = t.split()[0]
        wait = op == "s_waitcnt" and "lgkmcnt" in t
        if not (op.startswith("ds_") or wait or op == "s_barrier"):
            continue
        own = f.endswith(a.file) and any(lo <= line <= hi for lo, hi in ranges)
        n_wait += wait and own; n_ds += op.startswith("ds_") and own; n_bar += (op == "s_barrier") and own
        print(f"{' ' if own else '~'} {f.split('/')[-1]}:{line:<5d} {t}")
    print(f"# inside the ranges: {n_ds} ds_*, {n_wait} s_waitcnt lgkmcnt, {n_bar} s_barrier")


if __name__ == "__main__":
    main()
