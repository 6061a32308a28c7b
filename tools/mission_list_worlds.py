"""Octomap mission lists batched: the first K missions of the reference's 20-agent forest list (each on its own world/forest/forest{i}.bt)
and of its office list (all on office.bt), flown T ticks from their starts, device-resident, two ways:

  batched      : one lsc_tick_device_fused_batch per tick (goal batch -> corridor batch -> plan batch)
  back_to_back : every mission's own lsc_tick_device_fused in turn (three launches each)

One JSON line per (list, K): agent-replans/s by device time (HIP events around the tick) and by wall time (the tick synchronised), p99
tick (device), and the goal / corridor / plan kernel ms per tick (lsc_set_timing: which 3 / 4 / 0, summed over the contexts that record).
Missions and maps come from tests/golden (testall_missions_20agents.json, reference_maps.npz).

    python tools/mission_list_worlds.py [--ticks 40] [--warmup 5] [--ks 1,2,4,8] [--lists forest,office] [--modes batched,back_to_back]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def lay_out(tmp):
    maps = np.load(os.path.join(GOLDEN, "reference_maps.npz"))
    for key in maps.files:
        p = os.path.join(tmp, key)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(maps[key].tobytes())
    return json.load(open(os.path.join(GOLDEN, "testall_missions_20agents.json")))


def mission_list(L, missions, kind, k, tmp):
    """The first k missions of the list in the reference's order (names sorted: 1, 10, 11, ...) and their worlds."""
    names = sorted(missions[kind])[:k]
    out = []
    for name in names:
        p = os.path.join(tmp, f"{kind}_{name}")
        with open(p, "w") as f:
            f.write(missions[kind][name])
        i = name[len("multi_random_20agents_"):-len(".json")]
        out.append((L.load_mission(p), os.path.join(tmp, "forest", f"forest{i}.bt") if kind == "forest" else os.path.join(tmp, "office.bt")))
    return out


def fly(L, torch, specs, ticks, warmup, batched):
    from test_gpu_octomap_batch import Run
    cfg = lambda: L.PlannerConfig(use_octomap=True, goal_mode="prior_based", reset_threshold=0.15)
    runs = [Run(L, torch, ms, cfg(), bt) for ms, bt in specs]

    def tick():
        if batched:
            for r in runs:
                r.seq += 1
            L.tick_device_fused_batch([r.pl for r in runs], [r.states[0] for r in runs], [r.goal for r in runs], [r.prev for r in runs],
                                      [r.nxt for r in runs], [r.states[1] for r in runs], [r.cost for r in runs], [r.status for r in runs],
                                      [r.iters for r in runs], [r.seq for r in runs], runs[0].stream)
            for r in runs:
                r.flip()
        else:
            for r in runs:
                r.tick()
    try:
        for _ in range(warmup):
            tick()
        torch.cuda.synchronize()
        for r in runs:
            r.pl.set_timing(True)
        dev, wall = [], []
        for _ in range(ticks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            tick()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
        per_tick = {}
        for name, which in (("goal_ms", 3), ("sfc_ms", 4), ("plan_ms", 0)):
            tot = 0.0
            for r in runs:
                avg, n = r.pl.kernel_time_ms(which)
                tot += avg * n
            per_tick[name] = round(tot / ticks, 4)
        statuses = np.concatenate([r.status.cpu().numpy() for r in runs])
    finally:
        for r in runs:
            r.pl.close()
    agents = sum(ms.qn for ms, _ in specs)
    dev, wall = np.asarray(dev), np.asarray(wall)
    return dict(agent_replans_per_s_device=round(agents * ticks / (dev.sum() * 1e-3), 1),
                agent_replans_per_s_wall=round(agents * ticks / (wall.sum() * 1e-3), 1),
                tick_ms_mean=round(float(dev.mean()), 4), tick_ms_p99=round(float(np.percentile(dev, 99)), 4), **per_tick,
                last_tick_status_counts={int(s): int((statuses == s).sum()) for s in np.unique(statuses)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--lists", default="forest,office")
    ap.add_argument("--modes", default="batched,back_to_back")
    a = ap.parse_args()
    import torch
    import lsc_planner_amd as L
    with tempfile.TemporaryDirectory() as tmp:
        missions = lay_out(tmp)
        for kind in a.lists.split(","):
            for k in (int(x) for x in a.ks.split(",")):
                specs = mission_list(L, missions, kind, k, tmp)
                line = dict(list=kind, K=k, agents=sum(ms.qn for ms, _ in specs), ticks=a.ticks, warmup=a.warmup)
                for mode in a.modes.split(","):
                    line[mode] = fly(L, torch, specs, a.ticks, a.warmup, mode == "batched")
                if "batched" in line and "back_to_back" in line:
                    line["speedup_device"] = round(line["batched"]["agent_replans_per_s_device"] / line["back_to_back"]["agent_replans_per_s_device"], 3)
                    line["speedup_wall"] = round(line["batched"]["agent_replans_per_s_wall"] / line["back_to_back"]["agent_replans_per_s_wall"], 3)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
