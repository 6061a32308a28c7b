"""Goal planning on large octomap worlds: the 10 m forest fixture tiled k x k (tools/config_runs.forest_tiles), flown device-resident
(lsc_tick_device_fused) from random starts.  Per tick the goal, corridor and plan kernel times (lsc_set_timing: HIP events around each
launch, which 3 / 4 / 0), the nodes the goal searches expanded (summed over the agents) and where they kept their OPEN rows
(lsc_goal_storage: LDS, LDS restarted in HBM, HBM).  One JSON line per case.

  grid      : forest_tiles(k) for k in --tiles with --agents agents each, the default search ("auto": the LDS searches where the grid fits
              them, the HBM search where it does not: k = 4 and 6)
  ab        : forest_tiles(--ab-tiles) with goal_search "general" and "hbm" on the same ticks, alternating per tick after the same warm-up:
              the per-tick ratio and the price per expanded node of keeping the OPEN rows in HBM (the searches expand the same nodes;
              a tick waits for its longest search, so the price is the extra time over that search's expansions)

    python tools/large_world_goals.py [--tiles 2,3,4,6] [--agents 64,256] [--ticks 10] [--warmup 2] [--ab-tiles 2] [--skip-ab] [--skip-grid]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


class Flight:
    """One swarm flown with tick_device_fused; tick() returns (goal, sfc, plan) kernel ms of that tick and the expansions it made."""

    def __init__(self, L, torch, ms, cfg, bt):
        self.torch, self.ms = torch, ms
        self.pl = L.SwarmPlanner(ms, cfg)
        self.pl.load_octomap(bt)
        self.note = self.pl.L.lsc_last_note(self.pl.ctx).decode()
        dev = torch.device("cuda", 0)
        n, nv = ms.qn, self.pl.NV
        f32 = dict(dtype=torch.float32, device=dev)
        self.states = [torch.zeros((n, 9), **f32), torch.zeros((n, 9), **f32)]
        self.states[0][:, :3] = torch.from_numpy(ms.start).to(dev)
        self.goal = torch.from_numpy(ms.goal).to(dev).contiguous()
        self.trajs = [torch.zeros((n, nv), **f32), torch.zeros((n, nv), **f32)]
        self.cost = torch.zeros(n, dtype=torch.float64, device=dev)
        self.status = torch.zeros(n, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(n, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.seq = 0
        self.exp = np.zeros(self.pl.count, np.int32)

    def tick(self, timed):
        pl = self.pl
        if timed:
            pl.set_timing(True)
        self.seq += 1
        pl.tick_device_fused(self.states[0], self.goal, self.trajs[0], self.trajs[1], self.states[1], self.cost, self.status, self.iters,
                             self.seq, self.stream)
        self.states.reverse()
        self.trajs.reverse()
        self.torch.cuda.synchronize()
        ip = ctypes.POINTER(ctypes.c_int)
        pl._check(pl.L.lsc_get_goal_trace(pl.ctx, None, None, None, self.exp.ctypes.data_as(ip), None, None))
        if not timed:
            return None
        ms = [float(pl.kernel_times_ms(w).sum()) for w in (3, 4, 0)]
        pl.set_timing(False)
        return ms, int(self.exp.sum()), int(self.exp.max())

    def close(self):
        self.pl.close()


def swarm(L, tiles, n, seed):
    from config_runs import forest_tiles
    bt, world = forest_tiles(tiles)
    dist, kmin, r = L.edt_from_bt(bt, np.asarray(world[:3], np.float32), np.asarray(world[3:], np.float32))
    return L.random_swarm(n, world=world, seed=seed, edt=dist, edt_key_min=kmin, edt_res=r), bt


def cfg(L, search="auto"):
    return L.PlannerConfig(use_octomap=True, goal_mode="prior_based", reset_threshold=0.15, goal_search=search)


def grid_case(L, torch, tiles, n, ticks, warmup, seed):
    ms, bt = swarm(L, tiles, n, seed)
    f = Flight(L, torch, ms, cfg(L), bt)
    try:
        for _ in range(warmup):
            f.tick(False)
        rows = [f.tick(True) for _ in range(ticks)]
        where = f.pl.goal_storage()
        status = f.status.cpu().numpy()
        dims = np.zeros(3, np.int32)
        f.pl._check(f.pl.L.lsc_get_goal_trace(f.pl.ctx, None, None, None, None, dims.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None))
    finally:
        f.close()
    ms_ = np.array([r[0] for r in rows])
    return {"case": "grid", "tiles": tiles, "agents": n, "grid": dims.tolist(), "cells": int(np.prod(dims)), "ticks": ticks, "warmup": warmup,
            "goal_ms_per_tick": round(float(ms_[:, 0].mean()), 4), "goal_ms_max": round(float(ms_[:, 0].max()), 4),
            "sfc_ms_per_tick": round(float(ms_[:, 1].mean()), 4), "plan_ms_per_tick": round(float(ms_[:, 2].mean()), 4),
            "expansions_per_tick": int(np.mean([r[1] for r in rows])), "expansions_max_agent": int(np.mean([r[2] for r in rows])),
            "storage_last_tick": {k: int((where == v).sum()) for k, v in (("lds", 0), ("lds_restarted", 1), ("hbm", 2))},
            "status_last_tick": {int(s): int((status == s).sum()) for s in np.unique(status)}, "note": f.note}


def ab_case(L, torch, tiles, n, ticks, warmup, seed):
    """general and hbm fly the same swarm; the ticks alternate between the two contexts (same inputs: the searches are identical)."""
    ms, bt = swarm(L, tiles, n, seed)
    fl = {s: Flight(L, torch, ms, cfg(L, s), bt) for s in ("general", "hbm")}
    try:
        for _ in range(warmup):
            for f in fl.values():
                f.tick(False)
        rows = {s: [] for s in fl}
        for t in range(ticks):
            for s in (("general", "hbm") if t % 2 == 0 else ("hbm", "general")):
                rows[s].append(fl[s].tick(True))
    finally:
        for f in fl.values():
            f.close()
    g = {s: np.array([r[0][0] for r in rows[s]]) for s in fl}
    e = {s: np.array([r[1] for r in rows[s]]) for s in fl}
    emax = np.array([r[2] for r in rows["hbm"]])
    assert np.array_equal(e["general"], e["hbm"]), "the two searches expanded different nodes"
    return {"case": "ab", "tiles": tiles, "agents": n, "ticks": ticks, "warmup": warmup,
            "goal_ms_per_tick": {s: round(float(g[s].mean()), 4) for s in g},
            "hbm_over_general": round(float(g["hbm"].mean() / g["general"].mean()), 3),
            "per_tick_ratio_min_max": [round(float((g["hbm"] / g["general"]).min()), 3), round(float((g["hbm"] / g["general"]).max()), 3)],
            "expansions_per_tick": int(e["hbm"].mean()), "expansions_max_agent": int(emax.mean()),
            # a tick waits for its longest search: the extra time per node of that search
            "extra_ns_per_expansion_of_the_longest_search": round(float(1e6 * (g["hbm"] - g["general"]).mean() / emax.mean()), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tiles", default="2,3,4,6")
    ap.add_argument("--agents", default="64,256")
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ab-tiles", type=int, default=2)
    ap.add_argument("--skip-ab", action="store_true")
    ap.add_argument("--skip-grid", action="store_true")
    a = ap.parse_args()
    import torch
    import lsc_planner_amd as L
    L.load_library()
    agents = [int(x) for x in a.agents.split(",")]
    if not a.skip_grid:
        for k in (int(x) for x in a.tiles.split(",")):
            for n in agents:
                print(json.dumps(grid_case(L, torch, k, n, a.ticks, a.warmup, a.seed)), flush=True)
    if not a.skip_ab:
        for n in agents:
            print(json.dumps(ab_case(L, torch, a.ab_tiles, n, a.ticks, a.warmup, a.seed)), flush=True)


if __name__ == "__main__":
    main()
