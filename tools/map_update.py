"""What it costs to give a context another map: the host path against the device path, on the forest world and its 6 x 6 tiling
(tools/config_runs.forest_tiles).  One process, the legs alternating, --runs runs each; median and max - min in ms, wall clock:

  a  lsc_edt_from_bt + lsc_set_distmap      the host's distance field, integral images and goal grids, uploaded (every buffer reallocated)
  b  lsc_set_occupancy                      the occupancy uploaded, everything built on the device (allocates; synchronises)
     (the .bt file's occupancy is read once, outside the leg: lsc_occupancy_from_bt is reported on its own)
  c  lsc_map_update of one box              from the enqueue to a synchronise of the stream: the whole rebuild, nothing allocated

    python tools/map_update.py [--tiles 1,6] [--agents 64] [--runs 5] [--out profiles/map_update.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "spread_ms": round(float(max(ms) - min(ms)), 4), "runs": [round(float(v), 4) for v in ms]}


def case(L, torch, tiles, n, runs, seed):
    from config_runs import forest_tiles
    bt, world = forest_tiles(tiles)
    wmin, wmax = np.asarray(world[:3], np.float32), np.asarray(world[3:], np.float32)
    dist, kmin, res = L.edt_from_bt(bt, wmin, wmax)
    ms = L.random_swarm(n, world=world, seed=seed, edt=dist, edt_key_min=kmin, edt_res=res)
    t0 = time.perf_counter()
    occ, kmin_o, _ = L.occupancy_from_bt(bt, wmin, wmax)
    t_occ = (time.perf_counter() - t0) * 1e3
    cfg = L.PlannerConfig(use_octomap=True, goal_mode="prior_based")
    host, dev = L.SwarmPlanner(ms, cfg), L.SwarmPlanner(ms, cfg)
    stream = torch.cuda.current_stream().cuda_stream
    # a free 3 x 3 column of full height near the middle of the field
    cx, cy = dist.shape[0] // 2, dist.shape[1] // 2
    while occ[cx - 1:cx + 2, cy - 1:cy + 2].any():
        cx += 1
    box = [cx - 1, cy - 1, 0, cx + 2, cy + 2, dist.shape[2]]
    legs = {"a": [], "b": [], "c": []}
    host.load_octomap(bt); dev.set_occupancy(occ, kmin, res)              # (warm-up: first allocations, first launches)
    dev.map_update([box], [1], stream=stream); dev.map_update([box], [0], stream=stream)
    torch.cuda.synchronize()
    for r in range(runs):
        t0 = time.perf_counter()
        host.load_octomap(bt)
        torch.cuda.synchronize()
        legs["a"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        dev.set_occupancy(occ, kmin, res)
        torch.cuda.synchronize()
        legs["b"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        dev.map_update([box], [1 - r % 2], stream=stream)
        torch.cuda.synchronize()
        legs["c"].append((time.perf_counter() - t0) * 1e3)
    # the column goes (if the last leg left it standing): both contexts hold the file's map again, and the two paths must agree
    dev.map_update([box], [0], stream=stream)
    a, b = host.map_read(), dev.map_read()
    assert np.array_equal(b["occupancy"] != 0, occ != 0), "the updates did not restore the occupancy"
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("edt", "integral", "goal_occupancy")), "the two paths disagree"
    host.close(); dev.close()
    return {"case": "map_update", "tiles": tiles, "agents": n, "field": list(dist.shape), "cells": int(dist.size), "grid": [int(v) for v in a["dims"][4:7]],
            "occupancy_from_bt_ms": round(t_occ, 3), "a_edt_from_bt_set_distmap": stats(legs["a"]), "b_set_occupancy": stats(legs["b"]),
            "c_map_update_one_box": stats(legs["c"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tiles", default="1,6")
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import lsc_planner_amd as L
    for k in (int(x) for x in a.tiles.split(",")):
        line = json.dumps(case(L, torch, k, a.agents, a.runs, a.seed))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
