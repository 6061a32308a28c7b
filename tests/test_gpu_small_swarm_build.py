"""-m gpu: the LSC build of small swarms (at most 64 obstacles: one wave per segment, lane = obstacle, rows stored straight to their final
slots; csrc/lsc_kernels.hip, phase B of plan_agent) against the generic pass it replaces there (forced by LSC_GENERIC_LSC_BUILD at
context creation).

Two contexts are flown in lockstep on the same inputs.  Both builds must give the same bits at every tick: plans, costs, statuses,
iteration counts, the planned goals, the row count and the fullest bucket of every agent -- the compact row layout (rn, rrhs, cmap, offs,
offcnt, cnt, nact) is the same to the last bit, so everything behind it is.  The last test runs the whole file once more through the
LDS-poison libraries: the new path must not read a word of LDS it did not write.
"""
import os

import numpy as np
import pytest

from harness import assert_lockstep, circle, exact, fly, held_pair, held_planner, start_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "LSC_GENERIC_LSC_BUILD"
NEW, OLD = "lsc build: one wave per segment", "lsc build: generic pass (LSC_GENERIC_LSC_BUILD)"
BEYOND = "lsc build: generic pass (more than 64 obstacles)"
DIAGNOSTICS = ("last_goals", "row_counts", "bucket_max")
GUSTS = {5: (3, (0.25, -0.2, 0.0)), 9: (0, (-0.2, 0.15, 0.05)), 14: (6, (0.1, 0.3, 0.0))}


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


def _circle(L, n, radius=None):
    return circle(L, n, radius if radius is not None else max(1.0, 8.0 * n / 64.0))


def _fly(new, old, ms, ticks, want_constraints=False, **kw):
    """Both contexts in lockstep on host buffers, every output and diagnostic equal at every tick; returns the largest row count seen."""
    keys = ("traj", "cost", "status", "iters") + (("normal", "d") if want_constraints else ())
    most = [0]

    def same(tick, state, traj, outs):
        assert_lockstep(new, old, tick, outs, eq=exact, keys=keys, diagnostics=DIAGNOSTICS)
        most[0] = max(most[0], int(new.row_counts().max()))
    fly((new, old), ms, ticks, each_tick=same, want_constraints=want_constraints, **kw)
    return most[0]


class _DeviceRun:
    """One context's device-resident fused ticks: the host never sees the states."""

    def __init__(self, torch, pl, ms):
        self.torch, self.pl, self.N = torch, pl, ms.qn
        dev = torch.device("cuda", 0)
        s0 = start_inputs(ms, pl.SEGV)[0]
        self.goal = torch.from_numpy(np.ascontiguousarray(ms.goal, np.float32)).to(dev)
        self.states = [torch.from_numpy(s0).to(dev), torch.zeros((self.N, 9), device=dev)]
        self.prev = torch.zeros((self.N, 3 * pl.SEGV), device=dev)
        self.next = torch.zeros((self.N, 3 * pl.SEGV), device=dev)
        self.cost = torch.zeros(self.N, dtype=torch.float64, device=dev)
        self.status = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(self.N, dtype=torch.int32, device=dev)

    def outputs(self):
        return [t.cpu().numpy().copy() for t in (self.next, self.states[1], self.cost, self.status, self.iters)]

    def advance(self):
        self.states.reverse()
        self.prev, self.next = self.next, self.prev


def test_bench_mission_host_buffer_ticks(L, monkeypatch):
    """The benchmark's mission (64-agent circle, R = 8 m, prior_based goals, reset_threshold 0.15), ticks 1-120."""
    ms = _circle(L, 64, 8.0)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15), monkeypatch, ENV, NEW, OLD)
    assert _fly(new, old, ms, 120) > 0
    new.close(); old.close()


def test_bench_mission_device_resident_fused_ticks(L, monkeypatch):
    """The same mission the way the benchmark flies it: lsc_tick_device_fused, one launch per tick, ticks 1-120."""
    import torch
    ms = _circle(L, 64, 8.0)
    pls = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15), monkeypatch, ENV, NEW, OLD)
    runs = [_DeviceRun(torch, pl, ms) for pl in pls]
    st = torch.cuda.current_stream().cuda_stream
    for tick in range(1, 121):
        outs = []
        for r in runs:
            r.pl.tick_device_fused(r.states[0], r.goal, r.prev, r.next, r.states[1], r.cost, r.status, r.iters, tick, st)
            torch.cuda.synchronize()
            outs.append(r.outputs())
        for k, (a, b) in enumerate(zip(*outs)):
            assert np.array_equal(a, b), (tick, ("traj", "state_next", "cost", "status", "iters")[k])
        assert_lockstep(pls[0], pls[1], tick, ({}, {}), eq=exact, keys=(), diagnostics=DIAGNOSTICS)
        for r in runs:
            r.advance()
    for pl in pls:
        pl.close()


@pytest.mark.parametrize("n", [2, 3, 20, 65, 66])
def test_swarm_sizes(L, monkeypatch, n):
    """Near-empty waves (1 and 2 lanes), 19 lanes, the full 64-lane wave -- and 65 obstacles, where BOTH contexts take the generic pass."""
    ms = _circle(L, n)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15), monkeypatch, ENV, NEW if n <= 65 else BEYOND, OLD)
    most = _fly(new, old, ms, 40)
    assert most > 0 or n == 2, most
    new.close(); old.close()


def test_sixty_three_lane_waves_static_goals(L, monkeypatch):
    """64 agents without the alternate-mode hooks (lsc_plan_kernel: static goals, no disturbance checks)."""
    ms = _circle(L, 64, 6.0)
    new, old = held_pair(L, ms, L.PlannerConfig(), monkeypatch, ENV, NEW, OLD)
    assert _fly(new, old, ms, 40) > 0
    new.close(); old.close()


@pytest.mark.parametrize("prune", [0, 3])
def test_prune_modes(L, monkeypatch, prune):
    """prune 0: every one of the 27 (N - 1) rows is kept; 3: the exact test only."""
    ms = _circle(L, 20, 2.0)
    new, old = held_pair(L, ms, L.PlannerConfig(prune=prune, goal_mode="prior_based"), monkeypatch, ENV, NEW, OLD)
    most = _fly(new, old, ms, 15)
    if prune == 0:
        assert most == 27 * 19, most
    new.close(); old.close()


def test_overflow_into_the_second_pass(L, monkeypatch):
    """A row capacity of 27 x 1: agents with more rows are flagged by the LDS pass -- which must store NONE of their rows: the slots beyond the
    capacity are not theirs -- and planned by the pass with its rows in HBM."""
    ms = _circle(L, 20, 1.5)
    new, old = held_pair(L, ms, L.PlannerConfig(max_rows_per_cp=1, goal_mode="prior_based"), monkeypatch, ENV, NEW, OLD)
    cap = new.row_capacity()[0]
    assert cap == 27, cap
    assert _fly(new, old, ms, 25) > cap
    new.close(); old.close()


def test_planar_world(L, monkeypatch):
    ms = _circle(L, 12, 2.0)
    cfg = L.PlannerConfig(goal_mode="prior_based", world_dimension=2, world_z_2d=1.0)
    new, old = held_pair(L, ms, cfg, monkeypatch, ENV, NEW, OLD)
    assert _fly(new, old, ms, 20, planar_z=1.0) > 0
    new.close(); old.close()


@pytest.mark.parametrize("goal_mode", ["static", "prior_based"])
def test_gusts_flag_the_swarm(L, monkeypatch, goal_mode):
    """Gusts push agents off their plans: from then on phase A flags the swarm, phase B builds no unit (n_units = 0) and the folded general
    solver plans every agent."""
    ms = L.circle_swap(12, 2.0, world=(-5, -5, 0, 5, 5, 2.5))
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode=goal_mode, reset_threshold=0.15), monkeypatch, ENV, NEW, OLD)
    _fly(new, old, ms, 18, gusts=GUSTS)
    new.close(); old.close()


@pytest.mark.parametrize("n", [20, 64])
def test_interior_point_slot_tables(L, monkeypatch, n):
    """solver interior_point: the slot tables of the row reduction are built from the same counts and offsets."""
    ms = _circle(L, n, 2.0 if n == 20 else 6.0)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", solver="interior_point"), monkeypatch, ENV, NEW, OLD)
    assert _fly(new, old, ms, 15) > 0
    new.close(); old.close()


@pytest.mark.parametrize("n", [20, 65])
def test_four_segment_library(L, monkeypatch, n):
    """M = 4 (dt 0.5, horizon 2.0): four segment waves, 24 control points."""
    L.load_library(4)
    ms = _circle(L, n)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", dt=0.5, horizon=2.0), monkeypatch, ENV, NEW, OLD)
    assert new.M == 4
    assert _fly(new, old, ms, 15) > 0
    new.close(); old.close()


def test_batched_tick_of_mixed_sizes(L, monkeypatch):
    """One launch for several swarms (lsc_tick_device_fused_batch), each block of the launch by its own arguments: 20 + 64 + 40 agents
    in the batch, and a 70-agent swarm flown beside it on its own fused ticks.  (A batched launch has no second pass and the LDS holds
    27 x 63 rows -- lsc_row_capacity --, so lsc_tick_device_fused_batch refuses every swarm of more than 64 agents: the 70-agent swarm,
    which takes the generic pass in both contexts, cannot be a block of the batch itself.)"""
    import torch
    sizes, beside = (20, 64, 40), 70
    cfg = lambda: L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15)
    groups = []
    for generic in (False, True):
        runs = []
        for n in sizes + (beside,):
            ms = _circle(L, n)
            pl = held_planner(L, ms, cfg, monkeypatch, ENV, generic, OLD if generic else (NEW if n <= 65 else BEYOND))
            runs.append(_DeviceRun(torch, pl, ms))
        groups.append(runs)
    st = torch.cuda.current_stream().cuda_stream
    for tick in range(1, 13):
        outs = []
        for runs in groups:
            inb, r70 = runs[:-1], runs[-1]
            L.tick_device_fused_batch([r.pl for r in inb], [r.states[0] for r in inb], [r.goal for r in inb], [r.prev for r in inb],
                                      [r.next for r in inb], [r.states[1] for r in inb], [r.cost for r in inb],
                                      [r.status for r in inb], [r.iters for r in inb], [tick] * len(inb), st)
            r70.pl.tick_device_fused(r70.states[0], r70.goal, r70.prev, r70.next, r70.states[1], r70.cost, r70.status, r70.iters, tick, st)
            torch.cuda.synchronize()
            outs.append([r.outputs() for r in runs])
        for s, (oa, ob) in enumerate(zip(*outs)):
            for k, (a, b) in enumerate(zip(oa, ob)):
                assert np.array_equal(a, b), (tick, (sizes + (beside,))[s], ("traj", "state_next", "cost", "status", "iters")[k])
            assert_lockstep(groups[0][s].pl, groups[1][s].pl, tick, ({}, {}), eq=exact, keys=(), diagnostics=DIAGNOSTICS)
        for runs in groups:
            for r in runs:
                r.advance()
    for runs in groups:
        for r in runs:
            r.pl.close()


@pytest.mark.parametrize("n", [20, 64])
def test_constraint_dump_of_the_plan_kernel(L, monkeypatch, n):
    """plan(..., want_constraints=True): the plan kernel's own dump of every unit's normal and margins, index (agent, obstacle, segment)."""
    ms = _circle(L, n, 2.0 if n == 20 else 6.0)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based"), monkeypatch, ENV, NEW, OLD)
    assert _fly(new, old, ms, 10, want_constraints=True) > 0
    new.close(); old.close()


def test_poison_build_small_swarms():
    """The whole file once more through the LDS-poison libraries (every byte of the workgroup's LDS is 0xff at entry): the new path no longer
    writes wcnt beyond its first row, tmp_rows or ntmp's rows, and must not read them."""
    import subprocess
    import sys
    lib = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_poison.so")
    lib4 = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_m4_poison.so")
    assert os.path.exists(lib), "liblsc_hip_poison.so not built (make -C lsc_planner_amd/csrc poison)"
    assert os.path.exists(lib4), "liblsc_hip_m4_poison.so not built (make -C lsc_planner_amd/csrc poison_m4)"
    env = dict(os.environ, LSC_HIP_LIB=lib, LSC_HIP_LIB_M4=lib4)
    env.pop(ENV, None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", "not poison_build"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:]
