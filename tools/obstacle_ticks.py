#!/usr/bin/env python3
"""What the mission's dynamic obstacles cost a tick.

    python tools/obstacle_ticks.py [--out profiles/obstacle_ticks.jsonl] [--repeats 5] [--start-tick 60] [--ticks 100] [--parent-lib liblsc_hip.so]
                                   [--legs circle64_K0,circle64_K8_models_moving,circle64_K8_chasers_moving]

One JSON line.  Legs: device-resident fused ticks of a circle swap of radius 8 m with static goals, K spheres of 0.2 m on a ring of
2.5 m drifting at 0.05 m/s, their states in a device buffer: circle64_K0 / _K8 / _K32 (63, 71, 95 obstacles per agent) and
circle56_K8 (63, as circle64_K0); circle64_K8_models: the same eight spheres as straight motion models that the context moves itself
(lsc_obstacle_motion: the obstacle stage is one more launch in front of every tick), next to circle64_K8, whose states the caller feeds --
held during the timed ticks like the fed ones (the clock's step is set to 0 there), so that the two legs' plan kernels see the same
obstacles and stage_ms is the stage's launch alone; circle64_K8_models_moving lets the clock run on; circle64_K8_chasers_moving: eight
chasing obstacles from the same ring, each after an agent of its own at the spheres' 0.05 m/s, installed through lsc_obstacle_motion_ex
(the stage is lsc_obstacle_step_kernel then), the clock running.  --legs keeps only the named legs (parent_circle64_K0 comes with
--parent-lib).  The disturbance reset (lsc_set_obstacles_ex, reset_threshold 0.15): circle64_K8_reset -- nobody is pushed, so against
circle64_K8 it is the price of the alternate-mode hooks in the obstacle kernel --; circle64_K8_reset_pushed: agent 0 is moved 0.3 m in
x five ticks in front of the timed ones, so every timed tick plans the whole swarm through the alternate-mode solver with the spheres
in its obstacle list, next to circle64_K0_reset_pushed, the same swarm and push without spheres.  Every leg flies the SAME ticks on a fresh context: flown to --start-tick, synchronised, --ticks ticks
enqueued, synchronised; the figure is that time over the ticks (the obstacles are held during the timed ticks: no launch of the tool's
own sits between two ticks).  Legs alternate in ONE process, --repeats times each; the line carries every run, median and spread
(max - min) of each leg and the ratio circle56_K8 / circle64_K0.  --parent-lib: a build of the parent commit's library; its leg
parent_circle64_K0 (the same ticks through that library, same process, same alternation) stands beside circle64_K0.  Needs a GPU."""
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
    obstacle calls, which its K = 0 leg never makes)."""
    cur, other = _lib.load_library(5), ctypes.CDLL(path)
    for name in _lib.EXPORTS:
        if hasattr(other, name):
            getattr(other, name).argtypes, getattr(other, name).restype = getattr(cur, name).argtypes, getattr(cur, name).restype
    return other


def ring(k):
    """k obstacles: (pos, vel, radius, downwash)"""
    th = 2.0 * np.pi * (np.arange(k) + 0.5) / max(k, 1)
    pos = np.stack([2.5 * np.cos(th), 2.5 * np.sin(th), 0.6 + 1.3 * (np.arange(k) % 4) / 3.0], axis=1)
    vel = 0.05 * np.stack([-np.sin(th), np.cos(th), np.zeros(k)], axis=1)
    return pos, vel, np.full(k, 0.2), np.full(k, 1.5)


class Run:
    def __init__(self, torch, n, k, lib=None, models=False, reset=0.0):
        dev = torch.device("cuda", 0)
        ms = L.circle_swap(n, 8.0)
        mine = _lib._LIBS[5]
        try:
            if lib is not None:
                _lib._LIBS[5] = lib              # (SwarmPlanner takes the library of its segment count from this table)
            pl = L.SwarmPlanner(ms, L.PlannerConfig(device=0, reset_threshold=reset))
        finally:
            _lib._LIBS[5] = mine
        self.torch, self.pl, self.k = torch, pl, k
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
        self.models = models
        if k and models == "chasers":
            pos, vel, rad, dw = ring(k)
            self.pl.set_obstacle_motion([{"type": "chasing", "start": list(map(float, p)), "size": float(r), "downwash": float(d), "max_vel": 0.05, "max_acc": 1.0,
                                          "gamma_target": 1.0, "gamma_obs": 0.05, "target": (i * n) // k} for i, (p, r, d) in enumerate(zip(pos, rad, dw))])
            self.pl.obstacle_clock(0.2, 0.2, 0.2)
        elif k and models:
            pos, vel, rad, dw = ring(k)
            self.pl.set_obstacle_motion([{"type": "straight", "start": list(map(float, p)), "goal": list(map(float, p + 1000.0 * v)), "speed": 0.05,
                                          "size": float(r), "downwash": float(d)} for p, v, r, d in zip(pos, vel, rad, dw)])
            self.pl.obstacle_clock(0.2, 0.2, 0.2)
        elif k:
            self.pos, self.vel, rad, dw = ring(k)
            if reset > 0.0:
                self.pl.set_obstacles(rad, dw, max_acc=1.0)              # (lsc_set_obstacles_ex: size prediction on, horizon 1.0)
            else:
                self.pl.set_obstacles(rad, dw)
            self.pos_vel = torch.zeros((k, 6), dtype=torch.float32, device=dev)
            self.pl.obstacle_states(self.pos_vel)

    def tick(self, move):
        if self.k and move and not self.models:
            pv = np.concatenate([self.pos + self.vel * (0.2 * self.seq), self.vel], axis=1).astype(np.float32)
            self.pos_vel.copy_(self.torch.from_numpy(pv))
        j = self.seq & 1
        self.pl.tick_device_fused(self.states[j], self.goal, self.trajs[j], self.trajs[j ^ 1], self.states[j ^ 1], self.cost, self.status,
                                  self.iters, self.seq + 1, self.stream)
        self.seq += 1


def one(torch, n, k, start_tick, ticks, lib=None, models=False, hold=True, reset=0.0, push=False):
    """-> (ms per tick, agent-ticks that failed in the timed window's last tick)"""
    r = Run(torch, n, k, lib, models, reset)
    try:
        for t in range(start_tick - 1):
            if push and t == start_tick - 6:
                r.states[r.seq & 1][0, 0] += 0.3                         # agent 0 off its plan: the swarm is flagged from here on
            r.tick(True)
        torch.cuda.synchronize()
        if models and hold:
            r.pl.obstacle_clock(0.2, r.pl.obstacle_clock_read(), 0.0)
        t0 = time.perf_counter()
        for _ in range(ticks):
            r.tick(False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt / ticks * 1e3, int((r.status != 0).sum().item())
    finally:
        r.pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacle_ticks.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--start-tick", type=int, default=60)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--legs", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    legs = {"circle64_K0": (64, 0), "circle64_K8": (64, 8), "circle64_K8_models": (64, 8), "circle64_K8_models_moving": (64, 8), "circle64_K8_chasers_moving": (64, 8), "circle64_K32": (64, 32), "circle56_K8": (56, 8),
            "circle64_K8_reset": (64, 8), "circle64_K8_reset_pushed": (64, 8), "circle64_K0_reset_pushed": (64, 0)}
    _lib.load_library(5)
    parent = other_library(a.parent_lib) if a.parent_lib else None
    if parent is not None:
        legs = {"parent_circle64_K0": (64, 0), **legs}
    if a.legs:
        legs = {leg: v for leg, v in legs.items() if leg in a.legs.split(",") or leg.startswith("parent_")}
    one(torch, 64, 8, 5, 5)                                                 # (first-launch costs of the process stay out of every leg)
    runs, failed = {leg: [] for leg in legs}, {leg: 0 for leg in legs}
    for _ in range(a.repeats):                                              # alternate: one run of every leg per round
        for leg, (n, k) in legs.items():
            ms_tick, bad = one(torch, n, k, a.start_tick, a.ticks, parent if leg.startswith("parent_") else None,
                               "chasers" if "_chasers" in leg else "_models" in leg, not leg.endswith("_moving"),
                               0.15 if "_reset" in leg else 0.0, leg.endswith("_pushed"))
            runs[leg].append(ms_tick)
            failed[leg] = max(failed[leg], bad)
    line = {"tool": "obstacle_ticks", "start_tick": a.start_tick, "ticks": a.ticks, "repeats": a.repeats,
            "ms_per_tick": {leg: {"median": round(float(np.median(v)), 5), "spread": round(float(max(v) - min(v)), 5),
                                  "runs": [round(float(x), 5) for x in v], "failed_agents_last_tick": failed[leg]} for leg, v in runs.items()}}
    if "circle64_K8_models" in runs and "circle64_K8" in runs:
        line["stage_ms"] = round(float(np.median(runs["circle64_K8_models"]) - np.median(runs["circle64_K8"])), 5)       # models on the device - fed by the caller
    if "circle64_K8_reset" in runs and "circle64_K8" in runs:
        line["hooks_ms"] = round(float(np.median(runs["circle64_K8_reset"]) - np.median(runs["circle64_K8"])), 5)          # the ALT + OBS build - the OBS build
    if "circle64_K8_reset_pushed" in runs and "circle64_K0_reset_pushed" in runs:
        line["spheres_in_the_alternate_solver_ms"] = round(float(np.median(runs["circle64_K8_reset_pushed"]) - np.median(runs["circle64_K0_reset_pushed"])), 5)
    if "circle56_K8" in runs and "circle64_K0" in runs:
        line["ratio_56_plus_8_over_64"] = round(float(np.median(runs["circle56_K8"]) / np.median(runs["circle64_K0"])), 4)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
