#!/usr/bin/env python3
"""ms per tick of large random swarms (BASELINE configs[4]'s density and bench.py's random1024 tick: prior_based goals, reset_threshold
0.15, one fused device-resident launch per tick; bench.py itself stops short of 65 536 agents: its dense-sweep leg allocates N^2 rows),
for two builds of the library in turn: the one next to the package and --before LIB (an older liblsc_hip.so, loaded through LSC_HIP_LIB).  Legs
alternate (after, before, after, before, ... per size), each a fresh bench.py process, so that drift of the GPU shows up in both.

    python tools/large_swarm.py [--before path/to/liblsc_hip.so] [--agents 8192,16384,32768,65536] [--rounds 2] [--out FILE]
    python tools/large_swarm.py --footprint [--agents 16384,65536]

--footprint: device memory a context of bench.py's configuration (prior_based goals, reset_threshold 0.15) takes at each size, read with
hipMemGetInfo (torch.cuda.mem_get_info) in front of and behind the planner's creation (lsc_create + lsc_set_agents), one process per size.

Every leg prints one JSON line (size, build, mean and median ms per tick); --out appends them to FILE.  Steps and warm-up shrink with N
(a 65 536-agent tick without the culls takes most of a second).  Needs a GPU; reads nothing outside the repository.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(n, lib, steps, warmup, timeout):
    env = dict(os.environ)
    if lib:
        env["LSC_HIP_LIB"] = lib
    else:
        env.pop("LSC_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg-child", str(n), str(steps), str(warmup)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"leg failed with exit status {r.returncode} ({n} agents, {'before' if lib else 'after'})")
    return json.loads(r.stdout.strip().splitlines()[-1])


def swarm(L, n):
    half = 20.0 * (n / 1024.0) ** 0.5
    return L.random_swarm(n, world=(-half, -half, 0, half, half, 5), seed=20260929)


def run_leg(n, steps, warmup):
    """bench.py's random1024 tick at n agents (prior_based goals, reset_threshold 0.15, one fused device-resident launch per tick), from
    the mission's start: `warmup` ticks, then `steps` timed ones (wall clock between two synchronisations; the tick is one launch)."""
    import time
    import torch
    import lsc_planner_amd as L
    dev = torch.device("cuda", 0)
    ms = swarm(L, n)
    pl = L.SwarmPlanner(ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15))
    f32 = dict(dtype=torch.float32, device=dev)
    states = [torch.zeros((n, 9), **f32), torch.zeros((n, 9), **f32)]
    states[0][:, :3] = torch.from_numpy(ms.start).to(dev)
    goal = torch.from_numpy(ms.goal).to(dev).contiguous()
    trajs = [torch.zeros((n, 90), **f32), torch.zeros((n, 90), **f32)]
    cost = torch.zeros(n, dtype=torch.float64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    iters = torch.zeros(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pl.tick_device_fused(states[k % 2], goal, trajs[k % 2], trajs[(k + 1) % 2], states[(k + 1) % 2], cost, status, iters, k + 1, stream)
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    u = pl.neighbour_counts()
    pl.close()
    return {"ms_per_tick": round(float(sum(times) / len(times)), 4), "tick_p50_ms": round(float(sorted(times)[len(times) // 2]), 4),
            "lists": u is not None, "agents_with_a_list": None if u is None else round(float((u >= 0).mean()), 4),
            "statuses_ok": round(float((status.cpu().numpy() == 0).mean()), 4)}


def footprint(n):
    import torch
    import lsc_planner_amd as L
    ms = swarm(L, n)
    torch.cuda.synchronize()
    free0, total = torch.cuda.mem_get_info(0)
    p = L.SwarmPlanner(ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15))
    free1, _ = torch.cuda.mem_get_info(0)
    print(json.dumps({"agents": n, "context_bytes": free0 - free1, "context_gib": round((free0 - free1) / 2 ** 30, 2),
                      "device_gib": round(total / 2 ** 30, 1), "lists": p.neighbour_counts() is not None}), flush=True)
    p.close()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--footprint-child":
        sys.path.insert(0, ROOT)
        footprint(int(sys.argv[2]))
        return
    if len(sys.argv) > 4 and sys.argv[1] == "--leg-child":
        sys.path.insert(0, ROOT)
        print(json.dumps(run_leg(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))), flush=True)
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", default=None, help="liblsc_hip.so of the build to compare against (omit: this build only)")
    ap.add_argument("--agents", default="8192,16384,32768,65536")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--footprint", action="store_true")
    a = ap.parse_args()
    if a.footprint:
        for n in [int(x) for x in a.agents.split(",")]:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--footprint-child", str(n)], cwd=ROOT, capture_output=True, text=True,
                               timeout=a.timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"footprint of {n} agents failed with exit status {r.returncode}")
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        return
    builds = [("after", None)] + ([("before", os.path.abspath(a.before))] if a.before else [])
    for n in [int(x) for x in a.agents.split(",")]:
        steps, warmup = (20, 10) if n <= 16384 else (4, 3)
        for rnd in range(a.rounds):
            for name, lib in (builds if rnd % 2 == 0 else builds[::-1]):
                res = leg(n, lib, steps, warmup, a.timeout)
                line = dict({"agents": n, "build": name, "round": rnd, "steps": steps, "warmup": warmup}, **res)
                print(json.dumps(line), flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
