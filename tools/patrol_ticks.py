#!/usr/bin/env python3
"""What the goal stage costs a tick.

    python tools/patrol_ticks.py [--out profiles/patrol_ticks.jsonl] [--repeats 5] [--start-tick 20] [--ticks 100] [--parent-lib liblsc_hip.so]

One JSON line.  Workloads: the 64-agent circle swap of radius 8 m (circle64) and random1024 (bench.py's flagship swarm: 1024 agents, seeded),
both with prior_based goals, device-resident.  Legs per workload, alternating in ONE process, --repeats times each:
    parent   no mission state, through a build of the parent commit's library (--parent-lib; left out without it)
    plain    no mission state, through this build
    patrol   a mission state open in PATROL on this build: the stage launches in front of every tick
Every leg flies the SAME calls on a fresh context: flown to --start-tick by lsc_fly_device, synchronised, --ticks ticks enqueued by one
lsc_fly_device call, synchronised; the figure is that time over the ticks.  The line carries every run, median and spread (max - min) of
each leg, and the swaps the patrol leg made.  The stage's cost is patrol over plain WHERE NOBODY SWAPPED (swaps 0: the three legs then
plan the same plans; after a swap the patrol leg flies another mission than the other two, and the difference is that mission's too).
circle64's agents need more than 120 ticks for their 16 m; random1024's legs are of every length, so a window in front of its first
arrival is short (--start-tick 3 --ticks 12).  parent and plain must lie inside each other's spread.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lsc_planner_amd as L  # noqa: E402
from lsc_planner_amd import _lib  # noqa: E402


def other_library(path):
    """A second build of the library in this process, bound like the first as far as it has the symbols (a parent build lacks the
    mission calls, which its leg never makes)."""
    cur, other = _lib.load_library(5), ctypes.CDLL(path)
    for name in _lib.EXPORTS:
        if hasattr(other, name):
            getattr(other, name).argtypes, getattr(other, name).restype = getattr(cur, name).argtypes, getattr(cur, name).restype
    return other


def missions():
    return {"circle64": L.circle_swap(64, 8.0), "random1024": L.random_swarm(1024)}


class Run:
    def __init__(self, torch, ms, patrol, lib=None):
        dev = torch.device("cuda", 0)
        mine = _lib._LIBS[5]
        try:
            if lib is not None:
                _lib._LIBS[5] = lib              # (SwarmPlanner takes the library of its segment count from this table)
            pl = L.SwarmPlanner(ms, L.PlannerConfig(device=0, goal_mode="prior_based"))
        finally:
            _lib._LIBS[5] = mine
        n = ms.qn
        self.torch, self.pl = torch, pl
        s0 = torch.zeros((n, 9), dtype=torch.float32, device=dev)
        s0[:, :3] = torch.from_numpy(ms.start).to(dev)
        self.states = [s0, torch.zeros_like(s0)]
        self.goal = torch.from_numpy(ms.goal).to(dev).contiguous()
        self.trajs = [torch.zeros((n, 90), dtype=torch.float32, device=dev) for _ in range(2)]
        self.cost = torch.zeros(n, dtype=torch.float64, device=dev)
        self.status = torch.zeros(n, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(n, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.seq = 0
        if patrol:
            pl.mission_open(state="patrol")

    def fly(self, k):
        j = self.seq & 1
        self.pl.fly([self.states[j], self.states[j ^ 1]], self.goal, [self.trajs[j], self.trajs[j ^ 1]], self.seq + 1, k, self.cost, self.status,
                    self.iters, self.stream)
        self.seq += k


def one(torch, ms, patrol, start_tick, ticks, lib=None):
    """-> (ms per tick, agent-ticks that failed in the timed window's last tick, swaps made)"""
    r = Run(torch, ms, patrol, lib)
    try:
        r.fly(start_tick - 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.fly(ticks)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        legs = int(r.pl.mission_read()["legs"].sum()) if patrol else 0
        return dt / ticks * 1e3, int((r.status != 0).sum().item()), legs
    finally:
        r.pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patrol_ticks.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--start-tick", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    _lib.load_library(5)
    parent = other_library(a.parent_lib) if a.parent_lib else None
    ms = missions()
    legs = [(w, leg) for w in ms for leg in (["parent"] if parent is not None else []) + ["plain", "patrol"]]
    one(torch, ms["circle64"], True, 5, 5)                                  # (first-launch costs of the process stay out of every leg)
    runs, failed, swaps = {k: [] for k in legs}, {k: 0 for k in legs}, {k: 0 for k in legs}
    for _ in range(a.repeats):                                              # alternate: one run of every leg per round
        for w, leg in legs:
            ms_tick, bad, sw = one(torch, ms[w], leg == "patrol", a.start_tick, a.ticks, parent if leg == "parent" else None)
            runs[w, leg].append(ms_tick)
            failed[w, leg], swaps[w, leg] = max(failed[w, leg], bad), max(swaps[w, leg], sw)
    line = {"tool": "patrol_ticks", "start_tick": a.start_tick, "ticks": a.ticks, "repeats": a.repeats, "ms_per_tick": {}}
    for (w, leg), v in runs.items():
        line["ms_per_tick"][f"{w}_{leg}"] = {"median": round(float(np.median(v)), 5), "spread": round(float(max(v) - min(v)), 5),
                                             "runs": [round(float(x), 5) for x in v], "failed_agents_last_tick": failed[w, leg],
                                             "swaps": swaps[w, leg]}
    for w in ms:
        line[f"{w}_patrol_minus_plain_ms"] = round(float(np.median(runs[w, "patrol"]) - np.median(runs[w, "plain"])), 5)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
