"""-m gpu: the mission list as a batch axis on octomap worlds.  lsc_tick_device_fused_batch / lsc_replan_tick_batch run the goal search
(lsc_goal_batch_kernel), the corridor update (lsc_sfc_batch_kernel) and the plan kernel of several independent swarms, one launch each,
and every swarm must plan the same bits as its own tick: trajectories, next states, costs, statuses, iteration counts and planned goals,
tick by tick.  Missions are the reference's 20-agent forest / office suites (tests/golden/testall_missions_20agents.json) on their
own worlds (reference_maps.npz)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from harness import assert_same_flights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    return L


@pytest.fixture(scope="module")
def suite(tmp_path_factory):
    """(missions {suite: {name: text}}, world directory with the reference's .bt files)"""
    root = tmp_path_factory.mktemp("world")
    z = np.load(os.path.join(GOLDEN, "reference_maps.npz"))
    for name in z.files:
        path = root / name
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(z[name].tobytes())
    return json.load(open(os.path.join(GOLDEN, "testall_missions_20agents.json"))), str(root)


def mission(L, suite, kind, i, n=None):
    """Mission i of the forest / office suite (first n agents) and its world file."""
    missions, world = suite
    path = os.path.join(world, f"{kind}_{i}.json")
    with open(path, "w") as f:
        f.write(missions[kind][f"multi_random_20agents_{i}.json"])
    ms = L.load_mission(path)
    if n is not None and n < ms.qn:
        ms = L.Mission(ms.start[:n].copy(), ms.goal[:n].copy(), ms.world_min, ms.world_max, ms.radius[:n].copy(), ms.downwash[:n].copy(),
                       ms.max_vel[:n].copy(), ms.max_acc[:n].copy(), ms.nominal_velocity[:n].copy(), name=f"{kind}{i}_{n}")
    bt = os.path.join(world, "forest", f"forest{i}.bt") if kind == "forest" else os.path.join(world, "office.bt")
    return ms, bt


class Run:
    """One mission flown device-resident (tick_device_fused), buffers sized by the library's segment count."""

    def __init__(self, L, torch, ms, cfg, bt):
        dev = torch.device("cuda", 0)
        self.torch, self.pl = torch, L.SwarmPlanner(ms, cfg)
        if bt is not None:
            self.pl.load_octomap(bt)
        n, nv = ms.qn, self.pl.NV
        f32 = dict(dtype=torch.float32, device=dev)
        s0 = torch.zeros((n, 9), **f32)
        s0[:, :3] = torch.from_numpy(ms.start).to(dev)
        self.states = [s0, torch.zeros_like(s0)]
        self.goal = torch.from_numpy(ms.goal).to(dev).contiguous()
        self.prev, self.nxt = torch.zeros((n, nv), **f32), torch.zeros((n, nv), **f32)
        self.cost = torch.zeros(n, dtype=torch.float64, device=dev)
        self.status = torch.zeros(n, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(n, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.seq = 0

    def flip(self):
        self.states.reverse()
        self.prev, self.nxt = self.nxt, self.prev

    def tick(self):
        self.seq += 1
        self.pl.tick_device_fused(self.states[0], self.goal, self.prev, self.nxt, self.states[1], self.cost, self.status, self.iters,
                                  self.seq, self.stream)
        self.flip()

    def snapshot(self):
        self.torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (self.prev, self.states[0], self.cost, self.status, self.iters)] + [self.pl.last_goals()]


def fly(L, specs, ticks, batch, gust_at=None):
    """specs: [(mission, config, world file or None)] -> per tick, per mission the snapshot list."""
    import torch
    runs = [Run(L, torch, ms, cfg, bt) for ms, cfg, bt in specs]
    out = []
    try:
        for t in range(ticks):
            if gust_at is not None and t == gust_at:
                for r in runs:                       # agent 0 of every swarm 0.3 m off its plan (> reset_threshold)
                    r.states[0][0, 0] += 0.3
            if batch:
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
            out.append([r.snapshot() for r in runs])
    finally:
        for r in runs:
            r.pl.close()
    return out


NAMES = ("traj", "next state", "cost", "status", "iters", "goals")


def prior(L, **kw):
    return L.PlannerConfig(use_octomap=True, goal_mode="prior_based", **kw)


def ragged_specs(L, suite):
    return [mission(L, suite, "forest", i, n) for i, n in ((1, 20), (2, 13), (3, 8), (4, 20))]


def test_ragged_forest_batch(L, suite):
    """Four forest missions cut to 20 / 13 / 8 / 20 agents on their own worlds, 40 ticks: one goal, corridor and plan launch per tick."""
    specs = [(ms, prior(L), bt) for ms, bt in ragged_specs(L, suite)]
    solo = fly(L, specs, 40, False)
    specs = [(ms, prior(L), bt) for ms, bt in ragged_specs(L, suite)]
    bat = fly(L, specs, 40, True)
    assert_same_flights(solo, bat, NAMES)
    assert sum(int((m[3] == 0).sum()) for m in solo[-1]) > 0
    assert not np.array_equal(solo[-1][0][5], solo[-1][3][5])         # (the missions are not copies of each other)


def test_mixed_batch_forest_office_and_empty_map(L, suite):
    """Another grid (office: a second search instantiation, so a second goal launch) and a swarm without a distance field in one batch."""
    def specs():
        f, fb = mission(L, suite, "forest", 5)
        o, ob = mission(L, suite, "office", 1)
        c = L.circle_swap(8, circle_radius=3.0, z=1.0, world=(-5, -5, 0, 5, 5, 2.5))
        return [(f, prior(L), fb), (o, prior(L), ob), (c, L.PlannerConfig(goal_mode="prior_based"), None)]
    assert_same_flights(fly(L, specs(), 20, False), fly(L, specs(), 20, True), NAMES)


def test_gust_forest_batch(L, suite):
    """Disturbance checks on (reset_threshold 0.15) and a gust at tick 6: corridors re-seeded, agents handed over, batched."""
    def specs():
        return [(ms, prior(L, reset_threshold=0.15), bt) for ms, bt in (mission(L, suite, "forest", i) for i in (6, 7, 8))]
    assert_same_flights(fly(L, specs(), 12, False, gust_at=6), fly(L, specs(), 12, True, gust_at=6), NAMES)


def test_host_buffer_batch_equals_replan_tick(L, suite):
    """replan_tick_batch against SwarmPlanner.plan (lsc_replan_tick) per context, closed loop on the host.  One context with a small
    OPEN-row capacity (status 5 inside the batch), one with an agent whose seed box touches a tree (status 4)."""
    from lsc_planner_amd.planner import next_state_host

    def setup():
        a, ab = mission(L, suite, "forest", 9)
        b, bb = mission(L, suite, "forest", 10, 16)
        c, cb = mission(L, suite, "office", 2)
        # an agent of b starts right next to a tree (closer than radius + res / 2): its first corridor seed box is blocked (status 4)
        dist, kmin, res = L.edt_from_bt(bb, b.world_min, b.world_max)
        layer = dist[:, :, int(1.0 / res)]
        occ = np.argwhere((layer > 0) & (layer <= 0.15))
        assert len(occ)
        cell = occ[len(occ) // 2]
        b.start[3] = np.array([(cell[0] + kmin[0] - 32768 + 0.5) * res, (cell[1] + kmin[1] - 32768 + 0.5) * res, 1.05], np.float32)
        out = []
        for ms, bt, cfg in ((a, ab, prior(L)), (b, bb, prior(L)), (c, cb, prior(L, goal_row_cap=30))):
            pl = L.SwarmPlanner(ms, cfg)
            pl.load_octomap(bt)
            out.append((pl, ms))
        return out

    def run(batch, ticks=8):
        pls = setup()
        st = []
        for pl, ms in pls:
            s = np.zeros((ms.qn, 9), np.float32)
            s[:, :3] = ms.start
            st.append([s, np.zeros((ms.qn, 3, pl.SEGV), np.float32)])
        res = []
        for t in range(ticks):
            if batch:
                for pl, _ in pls:
                    pl.planner_seq += 1
                outs = L.replan_tick_batch([p for p, _ in pls], [s[0] for s in st], [ms.goal for _, ms in pls], [s[1] for s in st],
                                           [p.planner_seq for p, _ in pls])
            else:
                outs = []
                for (pl, ms), s in zip(pls, st):
                    g = pl.plan(s[0], ms.goal, s[1])
                    outs.append((g["traj"], g["cost"], g["status"], g["iters"]))
            tick = []
            for (pl, ms), s, o in zip(pls, st, outs):
                tick.append([x.copy() for x in o] + [pl.last_goals()])
                s[1] = o[0].copy()
                s[0] = next_state_host(o[0])
            res.append(tick)
        for pl, _ in pls:
            pl.close()
        return res

    solo, bat = run(False), run(True)
    for t, (ta, tb) in enumerate(zip(solo, bat)):
        for m, (ma, mb) in enumerate(zip(ta, tb)):
            for k, (x, y) in enumerate(zip(ma, mb)):
                assert np.array_equal(x, y), f"tick {t} mission {m} output {k}"
    statuses = [np.concatenate([t[m][2] for t in solo]) for m in range(3)]
    assert (statuses[1] == 4).any(), "the blocked seed box is meant to give status 4"
    assert (statuses[2] == 5).any(), "goal_row_cap 30 on the office grid is meant to give status 5"


def test_refusals(L, suite):
    """Goal trace on, goal profiling on, use_octomap without a distance map: LscError with the reason."""
    import torch
    ms, bt = mission(L, suite, "forest", 11, 6)
    ms2, bt2 = mission(L, suite, "forest", 12, 6)

    def attempt(prep, load=True):
        runs = [Run(L, torch, ms, prior(L), bt), Run(L, torch, ms2, prior(L), bt2 if load else None)]
        try:
            prep(runs[1].pl)
            for r in runs:
                r.seq += 1
            L.tick_device_fused_batch([r.pl for r in runs], [r.states[0] for r in runs], [r.goal for r in runs], [r.prev for r in runs],
                                      [r.nxt for r in runs], [r.states[1] for r in runs], [r.cost for r in runs], [r.status for r in runs],
                                      [r.iters for r in runs], [r.seq for r in runs], runs[0].stream)
        finally:
            for r in runs:
                r.pl.close()
    with pytest.raises(L.LscError, match="goal trace"):
        attempt(lambda pl: pl.set_goal_trace(256))
    with pytest.raises(L.LscError, match="goal profiling"):
        attempt(lambda pl: pl.goal_profile(1))
    with pytest.raises(L.LscError, match="lsc_set_distmap was not called"):
        attempt(lambda pl: None, load=False)


def test_poison_build_ragged_batch():
    """The ragged case through the LDS-poison build: every block carves its LDS from its own arguments (row capacity, smem_bytes)."""
    lib = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_poison.so")
    assert os.path.exists(lib), "liblsc_hip_poison.so not built (make -C lsc_planner_amd/csrc poison)"
    env = dict(os.environ, LSC_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_octomap_batch.py") +
                        "::test_ragged_forest_batch"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "1 passed" in r.stdout


def test_four_segments_batch(L, suite):
    """One batch against the M = 4 library (dt 0.5, horizon 2.0, the reference's C++ defaults)."""
    def specs():
        return [(ms, prior(L, dt=0.5, horizon=2.0), bt) for ms, bt in (mission(L, suite, "forest", i, 12) for i in (13, 14, 15))]
    solo = fly(L, specs(), 10, False)
    assert solo[0][0][0].shape[1] == 72
    assert_same_flights(solo, fly(L, specs(), 10, True), NAMES)
