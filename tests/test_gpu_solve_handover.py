"""-m gpu: how the active-set solve hands a change from its search to its step and back (csrc/lsc_kernels.hip, gi_solve / search_reduce).

Step -> search: the step publishes ONE word, its code, which every wave reads in the same batch as the search's own loads; the size of the
working set and the count of changes stay in wave 0's scalar registers (lane 0 of wave 0 writes every output they go into).  Search ->
step: by default the step loads the chosen row's word, then its right-hand side and normal with its second batch.  LSC_SOLVE_ROW_RECORD
at context creation switches the other hand-over on: the lane that holds the most violated row publishes the row's record -- word,
right-hand side, normal -- beside its wave's key, and the step takes it from there without a load (built, bit-identical, measured no
faster: DESIGN 4.1; kept behind the switch as the second opinion these tests compare against).

Every test flies a default context and a row-record context in lockstep on the same host-buffer inputs and compares plans, costs, statuses,
iteration counts, planned goals, row counts, the counters of lsc_solver_stats and the working-set peaks bit for bit at every tick: the
step's first values come from two independent places -- the lane's registers through the record, the arrays through the loads -- and a code
read too early or too late, or a size or count gone astray on wave 0, shows in the statuses, the iteration counts, the counters and the
peaks.  The last test runs the file once more through the LDS-poison libraries.
"""
import os

import numpy as np
import pytest

from harness import assert_lockstep, circle, fly, held_pair, held_planner, same_bits, start_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "LSC_SOLVE_ROW_RECORD"
NEW, OLD = "solve hand-over: plain", "solve hand-over: row record (LSC_SOLVE_ROW_RECORD)"
OUTPUTS = ("traj", "cost", "status", "iters")
DIAGNOSTICS = ("last_goals", "row_counts", "solver_stats", "working_set_peaks")


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


def _counted(pl):
    assert (pl.working_set_peaks() == 0).all()          # (the first call switches the counter on)
    return pl


def _pair(L, ms, cfg, monkeypatch):
    """(default context, context with the row record switched on), each checked through its note."""
    return tuple(_counted(pl) for pl in held_pair(L, ms, cfg, monkeypatch, ENV, NEW, OLD))


class _Seen:
    """Agent-ticks per class of the working set's peak (1-4, 5-8, 9-12, 13 = a thirteenth row asked for), per class the finished solves with
    more changes than their peak (a row left on the way), statuses, and the largest row count."""

    def __init__(self):
        self.peak, self.dropped, self.status, self.rows = np.zeros(4, int), np.zeros(3, int), {}, 0

    def add(self, pl, g):
        peaks = pl.working_set_peaks()
        self.rows = max(self.rows, int(pl.row_counts().max()))
        for p, it, s in zip(peaks, g["iters"], g["status"]):
            self.status[int(s)] = self.status.get(int(s), 0) + 1
            if p >= 1:
                self.peak[(min(int(p), 13) - 1) // 4] += 1
            if 1 <= p <= 12 and s == 0 and it > p:
                self.dropped[(int(p) - 1) // 4] += 1


def _fly(new, old, ms, ticks, seen=None, **kw):
    seen = seen or _Seen()

    def same(tick, state, traj, outs):
        assert_lockstep(new, old, tick, outs, keys=OUTPUTS, diagnostics=DIAGNOSTICS)
        seen.add(new, outs[0])
    fly((new, old), ms, ticks, each_tick=same, **kw)
    return seen


def _prior(L, **kw):
    return lambda: L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15, **kw)


def test_every_class_drops_and_the_thirteenth_row(L, monkeypatch):
    """Twelve agents swap across a circle of 1.5 m (the mission of tests/test_gpu_step_classes.py): working sets of every class, rows that
    leave, a thirteenth row and the hand-overs behind it -- full steps, partial steps and every code a step can publish."""
    ms = circle(L, 12, 1.5)
    new, old = _pair(L, ms, _prior(L), monkeypatch)
    seen = _fly(new, old, ms, 60)
    assert (seen.peak > 0).all(), seen.peak
    assert (seen.dropped > 0).all(), seen.dropped
    st = new.solver_stats()
    assert st["handed_over"] >= seen.peak[3] > 0 and st["solved"] > st["handed_over"], st
    new.close(); old.close()


def test_circle_of_eight(L, monkeypatch):
    """Eight agents at 1.2 m: infeasible QPs around tick 50, the interior point's verdicts behind a hand-over."""
    ms = circle(L, 8, 1.2)
    new, old = _pair(L, ms, _prior(L), monkeypatch)
    seen = _fly(new, old, ms, 60)
    assert seen.status.get(1, 0) > 0, seen.status
    new.close(); old.close()


def test_infeasible_by_the_certificate(L, monkeypatch):
    """An agent inside another's collision model: code 3, the verdict is the solve's own and nothing is handed over."""
    ms = L.circle_swap(3, circle_radius=2.0, z=1.0, world=(-5, -5, 0, 5, 5, 2.5))
    ms.start[1] = ms.start[0] + np.array([0.05, 0.0, 0.0], np.float32)
    new, old = _pair(L, ms, lambda: L.PlannerConfig(), monkeypatch)
    seen = _fly(new, old, ms, 2)
    st = new.solver_stats()
    assert seen.status.get(1, 0) > 0 and st["handed_over"] == 0 and st["solved"] == 2 * ms.qn, (seen.status, st)
    new.close(); old.close()


def test_random_swarm_without_the_hooks(L, monkeypatch):
    """Twenty agents at random in a 3 m box, no disturbance checks: lsc_plan_kernel, without the alternate-mode hooks."""
    ms = L.random_swarm(20, world=(-1.5, -1.5, 0, 1.5, 1.5, 3.0), seed=2, min_sep=0.35, shrink=0.2)
    new, old = _pair(L, ms, lambda: L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.0), monkeypatch)
    seen = _fly(new, old, ms, 30)
    assert seen.peak[0] > 0 and seen.peak[1] > 0, seen.peak
    new.close(); old.close()


def test_second_rows_beyond_the_lanes(L, monkeypatch):
    """24 agents on a circle of 1.5 m with pruning off: 27 rows against each of 23 obstacles, 621 LSC rows for 512 lanes.  Every lane below
    109 holds a second row, which only the search's loop sees: a most violated row found there goes to the step as "not published", and
    the row-record context loads it like the default one."""
    ms = circle(L, 24, 1.5)
    new, old = _pair(L, ms, _prior(L, prune=False), monkeypatch)
    seen = _fly(new, old, ms, 30)
    assert seen.rows > 512, seen.rows
    assert seen.peak[0] > 0, seen.peak
    new.close(); old.close()


@pytest.mark.parametrize("n", [65, 66])
def test_largest_small_swarm_and_the_first_beyond(L, monkeypatch, n):
    """65 agents: the largest swarm of the small-swarm path.  66: the generic path, whose solve starts behind the row placement."""
    ms = circle(L, n, 8.0 * n / 64.0)
    new, old = _pair(L, ms, _prior(L), monkeypatch)
    seen = _fly(new, old, ms, 12)
    assert seen.peak[0] > 0, seen.peak
    new.close(); old.close()


def test_planar_world(L, monkeypatch):
    ms = circle(L, 6, 1.5)
    new, old = _pair(L, ms, lambda: L.PlannerConfig(goal_mode="prior_based", world_dimension=2, world_z_2d=1.0), monkeypatch)
    seen = _fly(new, old, ms, 30, planar_z=1.0)
    assert seen.peak[0] > 0 and seen.peak[1] > 0, seen.peak
    new.close(); old.close()


def test_four_segment_library(L, monkeypatch):
    """M = 4 (liblsc_hip_m4.so): the 8-agent circle."""
    L.load_library(4)
    ms = circle(L, 8, 1.0)
    new, old = _pair(L, ms, _prior(L, dt=0.5, horizon=2.0), monkeypatch)
    assert new.M == 4
    seen = _fly(new, old, ms, 20)
    assert seen.peak[0] > 0, seen.peak
    new.close(); old.close()


def test_every_agent_handed_over(L, monkeypatch):
    """solver = hand_over (lsc_config.solver 2): the solve runs, then the interior point plans every agent."""
    ms = circle(L, 8, 1.0)
    new, old = _pair(L, ms, _prior(L, solver="hand_over"), monkeypatch)
    _fly(new, old, ms, 20)
    st = new.solver_stats()
    assert st["handed_over"] == 20 * ms.qn and st["solved"] == 0, st
    new.close(); old.close()


class _DeviceRun:
    """One context's device-resident fused ticks: the host never sees the states."""

    def __init__(self, torch, pl, ms):
        self.pl, self.N = pl, ms.qn
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
        return [t.cpu().numpy().copy() for t in (self.next, self.states[1], self.cost, self.status, self.iters)] + [self.pl.working_set_peaks()]

    def advance(self):
        self.states.reverse()
        self.prev, self.next = self.next, self.prev


def test_batch_launch(L, monkeypatch):
    """Two missions as blocks of one launch (lsc_plan_batch_kernel runs the same gi_solve; each block carries its context's switch) against
    the same two flown alone, by a default and by a row-record context each."""
    import torch
    missions = [circle(L, 8, 1.2), circle(L, 8, 1.0)]
    groups = []          # the batch, alone, alone with the row record
    for record in (False, False, True):
        note = OLD if record else NEW
        groups.append([_DeviceRun(torch, _counted(held_planner(L, ms, _prior(L), monkeypatch, ENV, record, note)), ms) for ms in missions])
    st = torch.cuda.current_stream().cuda_stream
    names = ("traj", "state_next", "cost", "status", "iters", "peaks")
    top = 0
    for tick in range(1, 31):
        inb = groups[0]
        L.tick_device_fused_batch([r.pl for r in inb], [r.states[0] for r in inb], [r.goal for r in inb], [r.prev for r in inb],
                                  [r.next for r in inb], [r.states[1] for r in inb], [r.cost for r in inb],
                                  [r.status for r in inb], [r.iters for r in inb], [tick] * len(inb), st)
        for runs in groups[1:]:
            for r in runs:
                r.pl.tick_device_fused(r.states[0], r.goal, r.prev, r.next, r.states[1], r.cost, r.status, r.iters, tick, st)
        torch.cuda.synchronize()
        outs = [[r.outputs() for r in runs] for runs in groups]
        for s in range(len(missions)):
            top = max(top, int(outs[0][s][5].max()))
            for other in (1, 2):
                for k, (a, b) in enumerate(zip(outs[0][s], outs[other][s])):
                    assert same_bits(a, b), (tick, s, ("alone", "alone, row record")[other - 1], names[k])
        for runs in groups:
            for r in runs:
                r.advance()
    assert top >= 5, top
    for runs in groups:
        for r in runs:
            r.pl.close()


def test_poison_build_solve_handover():
    """The whole file once more through the LDS-poison libraries (every byte of the workgroup's LDS is 0xff at entry): a code read before the
    kernel's top cleared it ends the solve at its first search, and a record column that no lane wrote is a NaN in the row-record
    context's step -- either way the two contexts part, or a test's own condition on the mission fails."""
    import subprocess
    import sys
    lib = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_poison.so")
    lib4 = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_m4_poison.so")
    assert os.path.exists(lib), "liblsc_hip_poison.so not built (make -C lsc_planner_amd/csrc poison)"
    assert os.path.exists(lib4), "liblsc_hip_m4_poison.so not built (make -C lsc_planner_amd/csrc poison_m4)"
    env = dict(os.environ, LSC_HIP_LIB=lib, LSC_HIP_LIB_M4=lib4)
    env.pop(ENV, None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", "not poison_build"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
