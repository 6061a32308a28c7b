#!/usr/bin/env python3
"""What a tick costs beyond its kernel: the headline mission with launch timing off and on, and the host's share.

    [LSC_HIP_LIB=<another build>] python tools/tick_boundary.py [--steps 100] [--start-tick 60] [--missions 4]

Flies the 64-agent circle swap as bench.py does -- fast-forward to --start-tick, then --steps ticks of tick_device_fused on the current
stream with a synchronise on both sides -- four times over the same ticks (a fresh context each time, so every leg plans the same
window): timing off, timing on, and both once more with the clock stopped BEFORE the final synchronise (what the host needs to enqueue
the ticks).  Then the same for --missions missions through tick_device_fused_batch.  Prints one JSON line:

    ms_per_tick_timing_off / _on     wall clock over synchronised ticks
    kernel_ms_mean                   mean of kernel_times_ms(0) over the timed ticks (timing on)
    host_us_per_call_timing_off/_on  the enqueue time alone, per lsc_tick_device_fused call

The library comes from LSC_HIP_LIB as in the other A/B tools (lsc_planner_amd/_lib.py).  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lsc_planner_amd as L  # noqa: E402
import bench  # noqa: E402  (the headline's mission, MissionRun and the batched tick: the same loop bench.py times)


def fly(torch, runs, batch, start_tick, steps, timing, sync_inside):
    """-> (seconds for `steps` ticks, kernel_times_ms(0) of the first context).  sync_inside: the final synchronise is inside the clock."""
    for _ in range(start_tick - 1):
        bench.tick_runs(L, runs, batch)
    torch.cuda.synchronize()
    runs[0].pl.set_timing(timing)
    t0 = time.perf_counter()
    for _ in range(steps):
        bench.tick_runs(L, runs, batch)
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    k = runs[0].pl.kernel_times_ms(0) if timing else np.zeros(0)
    runs[0].pl.set_timing(False)
    return (t_all if sync_inside else t_enq), k


def leg(torch, missions, cfg_of, dev, batch, start_tick, steps, repeats):
    def once(timing, sync_inside):
        runs = [bench.MissionRun(L, torch, m, cfg_of(), dev, torch.cuda.current_stream()) for m in missions]
        dt, k = fly(torch, runs, batch, start_tick, steps, timing, sync_inside)
        for r in runs:
            r.close()
        return dt, k

    off, on, kmean = [], [], []
    for _ in range(repeats):                         # alternate, so that a drift of the node shows in both
        off.append(once(False, True)[0] / steps * 1e3)
        dt, k = once(True, True)
        on.append(dt / steps * 1e3)
        kmean.append(float(k.mean()))
    host_off = once(False, False)[0] / steps * 1e6
    host_on = once(True, False)[0] / steps * 1e6
    r5 = lambda x: round(float(x), 5)
    return {
        "ms_per_tick_timing_off": r5(np.median(off)), "ms_per_tick_timing_off_runs": [r5(x) for x in off],
        "ms_per_tick_timing_on": r5(np.median(on)), "ms_per_tick_timing_on_runs": [r5(x) for x in on],
        "kernel_ms_mean": r5(np.median(kmean)), "kernel_ms_mean_runs": [r5(x) for x in kmean],
        "host_us_per_call_timing_off": round(host_off, 2), "host_us_per_call_timing_on": round(host_on, 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--start-tick", type=int, default=60)
    ap.add_argument("--missions", type=int, default=4, help="missions of the batched leg (0: skip it)")
    ap.add_argument("--repeats", type=int, default=6, help="runs per timing setting; the line carries every run and the median")
    ap.add_argument("--reset-threshold", type=float, default=0.15)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ms, layout = bench.weak_scaling_mission(L, 1)
    cfg_of = lambda: L.PlannerConfig(device=0, goal_mode="prior_based", reset_threshold=a.reset_threshold)
    out = {"tool": "tick_boundary", "library": L.lib_path(), "workload": layout, "start_tick": a.start_tick, "steps": a.steps,
           "single": leg(torch, [ms], cfg_of, dev, False, a.start_tick, a.steps, a.repeats)}
    K = a.missions
    if K > 0:
        missions = [ms] + [bench.rotated_mission(L, ms, 2.0 * np.pi * (m / (7.0 * K) + 0.013 * m), f"rot{m}") for m in range(1, K)]
        out[f"batch{K}"] = leg(torch, missions, cfg_of, dev, True, a.start_tick, a.steps, a.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
