#!/usr/bin/env python3
"""What K ticks per call cost, with and without the flight log, next to the loop that calls the library once per tick.

    python tools/flight_loop.py [--out profiles/flight_loop.jsonl] [--repeats 5] [--start-tick 60] [--only circle64,random1024,random8192]

Per configuration one JSON line.  Every leg flies the SAME ticks: a fresh context is fast-forwarded to --start-tick (lsc_fly_device, log
closed), the stream is synchronised, then K ticks are enqueued and the stream is synchronised again; the clock runs over enqueue and
synchronise, and a leg's figure is that time over K.  Legs:

    python_loop      Python calls tick_device_fused once per tick (what bench.py's device-resident leg does)
    fly_closed       one lsc_fly_device call, no log open
    fly_what_<w>     one lsc_fly_device call with a log recording `what` = w (1 samples, 2 safety, 4 agents; 0: the summary alone)

for K = 1, 5, 20, 100.  circle64_obstacles (reset_threshold 0, which dynamic obstacles need): the same circle without obstacles (k0_*) and
with K = 8 straight motion models that the context moves itself (k8_*: the obstacle stage in front of every tick and, with a log, the
obstacle track behind the record launch), K = 20 and 100; record_ms / record_and_track_ms: the loop's difference fly_what_7 - fly_closed
of each (which = 6 times the flight kernel alone).  All legs of a configuration run in ONE process, alternating, --repeats times each, so that a drift of the node shows
in all of them; the line carries every run, the median and the spread (max - min) of each leg.  record_kernel_ms_<w>: mean of
kernel_times_ms(6), the record launch's own dispatch time, over 100 ticks.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lsc_planner_amd as L  # noqa: E402

TIMES = [0.0, 0.1]           # the record times of a 0.2 s tick sampled every 0.1 s (multisim_record_time_step)


class Run:
    def __init__(self, torch, ms, cfg, obstacles=None):
        dev = torch.device("cuda", 0)
        self.torch, self.pl = torch, L.SwarmPlanner(ms, cfg)
        if obstacles:
            self.pl.set_obstacle_motion(obstacles)
            self.pl.obstacle_clock(0.2, 0.2, 0.2)
        n = ms.qn
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

    def fly(self, k):
        j = self.seq & 1
        self.pl.fly([self.states[j], self.states[j ^ 1]], self.goal, [self.trajs[j], self.trajs[j ^ 1]], self.seq + 1, k, self.cost, self.status,
                    self.iters, self.stream)
        self.seq += k

    def python_loop(self, k):
        for _ in range(k):
            j = self.seq & 1
            self.pl.tick_device_fused(self.states[j], self.goal, self.trajs[j], self.trajs[j ^ 1], self.states[j ^ 1], self.cost, self.status,
                                      self.iters, self.seq + 1, self.stream)
            self.seq += 1


def one(torch, ms, cfg, leg, K, start_tick, timing=False, obstacles=None):
    """-> (ms per tick, record kernel times or None)"""
    r = Run(torch, ms, cfg, obstacles)
    try:
        r.fly(start_tick - 1)
        leg = leg.split("_", 1)[1] if leg[:3] in ("k0_", "k8_") else leg
        if leg.startswith("fly_what_"):
            w = int(leg.rsplit("_", 1)[1])
            r.pl.flight_begin(TIMES, K, samples=bool(w & 1), safety=bool(w & 2), agents=bool(w & 4))
        torch.cuda.synchronize()
        r.pl.set_timing(timing)
        t0 = time.perf_counter()
        if leg == "python_loop":
            r.python_loop(K)
        else:
            r.fly(K)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        k6 = r.pl.kernel_times_ms(6) if timing else None
        r.pl.set_timing(False)
        return dt / K * 1e3, k6
    finally:
        r.pl.close()


def configuration(torch, name, ms, cfg, whats, Ks, repeats, start_tick):
    legs = ["python_loop", "fly_closed"] + [f"fly_what_{w}" for w in whats]
    one(torch, ms, cfg, "fly_closed", 5, start_tick)                       # (first-launch costs of the process stay out of every leg)
    out = {"tool": "flight_loop", "config": name, "agents": int(ms.qn), "start_tick": start_tick, "record_times": TIMES, "repeats": repeats,
           "ms_per_tick": {}}
    for K in Ks:
        runs = {leg: [] for leg in legs}
        for _ in range(repeats):                                           # alternate: one run of every leg per round
            for leg in legs:
                runs[leg].append(one(torch, ms, cfg, leg, K, start_tick)[0])
        out["ms_per_tick"][f"K{K}"] = {leg: {"median": round(float(np.median(v)), 5), "spread": round(float(max(v) - min(v)), 5),
                                              "runs": [round(float(x), 5) for x in v]} for leg, v in runs.items()}
    for w in whats:
        k6 = one(torch, ms, cfg, f"fly_what_{w}", 100, start_tick, timing=True)[1]
        out[f"record_kernel_ms_{w}"] = {"mean": round(float(k6.mean()), 5), "min": round(float(k6.min()), 5), "max": round(float(k6.max()), 5),
                                        "launches": int(len(k6))}
    return out


def ring8():
    """Eight spheres of 0.2 m on a ring of 2.5 m drifting at 0.05 m/s (tools/obstacle_ticks.py), as straight motion models."""
    th = 2.0 * np.pi * (np.arange(8) + 0.5) / 8
    pos = np.stack([2.5 * np.cos(th), 2.5 * np.sin(th), 0.6 + 1.3 * (np.arange(8) % 4) / 3.0], axis=1)
    vel = 0.05 * np.stack([-np.sin(th), np.cos(th), np.zeros(8)], axis=1)
    return [{"type": "straight", "start": list(map(float, p)), "goal": list(map(float, p + 1000.0 * v)), "speed": 0.05, "size": 0.2, "downwash": 1.5}
            for p, v in zip(pos, vel)]


def configuration_obstacles(torch, ms, cfg, Ks, repeats, start_tick):
    legs = ["k0_fly_closed", "k0_fly_what_7", "k8_python_loop", "k8_fly_closed", "k8_fly_what_7"]
    obstacles = ring8()
    one(torch, ms, cfg, "k8_fly_what_7", 5, start_tick, obstacles=obstacles)
    out = {"tool": "flight_loop", "config": "circle64_obstacles", "agents": int(ms.qn), "start_tick": start_tick, "record_times": TIMES, "repeats": repeats,
           "ms_per_tick": {}}
    for K in Ks:
        runs = {leg: [] for leg in legs}
        for _ in range(repeats):
            for leg in legs:
                runs[leg].append(one(torch, ms, cfg, leg, K, start_tick, obstacles=obstacles if leg.startswith("k8_") else None)[0])
        med = {leg: float(np.median(v)) for leg, v in runs.items()}
        out["ms_per_tick"][f"K{K}"] = {leg: {"median": round(med[leg], 5), "spread": round(float(max(v) - min(v)), 5),
                                              "runs": [round(float(x), 5) for x in v]} for leg, v in runs.items()}
        out["ms_per_tick"][f"K{K}"]["record_ms"] = round(med["k0_fly_what_7"] - med["k0_fly_closed"], 5)
        out["ms_per_tick"][f"K{K}"]["record_and_track_ms"] = round(med["k8_fly_what_7"] - med["k8_fly_closed"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flight_loop.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--start-tick", type=int, default=60)
    ap.add_argument("--only", default="circle64,random1024,random8192")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    cfg = L.PlannerConfig(device=0, goal_mode="prior_based", reset_threshold=0.15)
    want = a.only.split(",")
    Ks = (1, 5, 20, 100)
    lines = []
    if "circle64" in want:
        lines.append(configuration(torch, "circle64", L.circle_swap(64, 8.0), cfg, range(8), Ks, a.repeats, a.start_tick))
    if "circle64_obstacles" in want:
        lines.append(configuration_obstacles(torch, L.circle_swap(64, 8.0), L.PlannerConfig(device=0, goal_mode="prior_based"), (20, 100), a.repeats, a.start_tick))
    if "random1024" in want:
        lines.append(configuration(torch, "random1024", L.random_swarm(1024), cfg, range(8), Ks, a.repeats, a.start_tick))
    if "random8192" in want:
        half = 20.0 * (8192 / 1024.0) ** 0.5
        ms = L.random_swarm(8192, world=(-half, -half, 0, half, half, 5), seed=20260929)
        lines.append(configuration(torch, "random8192", ms, cfg, (5, 7), Ks, max(2, a.repeats // 2), min(a.start_tick, 10)))
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
