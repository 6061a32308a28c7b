"""-m gpu: the start of the active-set solve of small swarms on the waves that wait beside the GJK pass (csrc/lsc_kernels.hip, plan_agent: the
goal wave fills the bound slots, gi_hz, the unconstrained optimum and its x, the copy waves the velocity and acceleration slots, gi_zt and
the zeros of the working set; behind barrier (4) only the scales of the LSC rows are left) against the generic path
(LSC_GENERIC_LSC_BUILD at context creation), which forms all of that behind the row placement, by all waves, through three barriers.

Every test flies a default context and a generic-pass context in lockstep on the same host-buffer inputs and compares plans, costs,
statuses, iteration counts, planned goals and row counts bit for bit at every tick, like tests/test_gpu_goal_wave.py.  What is forced
here: every row T = 1 .. M of the tables the goal wave picks by its own T, the first tick, the kernel without the alternate-mode hooks, a
solve without a single LSC row, the largest swarm of the path and the first beyond it, the hand-over to the interior point (which must
find S.as_, S.az, S.at2, S.K and S.y as it expects them), the folded general solver behind the helper waves' stores, the planar kernel,
the M = 4 library and the batch launch.  The last test runs the file once more through the LDS-poison libraries.
"""
import os

import numpy as np
import pytest

from harness import assert_lockstep, circle, fly, held_pair, held_planner, same_bits, start_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "LSC_GENERIC_LSC_BUILD"
NEW, OLD = "lsc build: one wave per segment", "lsc build: generic pass (LSC_GENERIC_LSC_BUILD)"
BEYOND = "lsc build: generic pass (more than 64 obstacles)"
# case 1's mission: 8 agents on a circle of 1 m, each 2 m (goal_radius) from its goal: T = 1 at the start, then T = 2, 3, 4 as the agent
# closes in.  T = M needs a flight time of at most 1e-9 s, a position within a nanometre of the goal: the four agents on the axes get
# there -- one coordinate of their goals is 1 or -1, which the float32 state hits exactly, the other is next to zero, where float32 resolves
# the geometric approach (a factor of 0.87 per tick) all the way down.  Flown on the CPU oracle with the arithmetic of _terminal_segments:
# T = 1, 2, 3, 4, 5 first seen at ticks 1, 6, 32, 35, 141; every agent within 1e-5 m of its goal from tick 100 on, every status 0.
# (The same on a circle of 0.8 m -- ticks 1, 6, 29, 32, 152 --; at 1.2 m the oracle meets an infeasible QP at tick 49, at 1.5 m the swap
#  locks up.)
CIRCLE_N, CIRCLE_R = 8, 1.0
ARRIVED, CAP = 1e-5, 220


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


def _circle(L, n=CIRCLE_N, radius=CIRCLE_R):
    return circle(L, n, radius)


def _terminal_segments(goals, state, vnom, M, dt):
    """getTerminalSegments per agent on the host, by the kernel's arithmetic: float32 norm of goal - position, the rest in doubles."""
    d = np.asarray(goals, np.float32) - np.asarray(state[:, :3], np.float32)
    n2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float32) + d[:, 2] * d[:, 2]
    assert n2.dtype == np.float32
    flight = np.sqrt(n2.astype(np.float64)) / np.asarray(vnom, np.float64)
    T = np.trunc((M * dt - flight + 1e-9) / dt).astype(np.int64)
    return np.maximum(T, 1)


def _fly(new, old, ms, ticks, each_tick=None, **kw):
    """Both contexts in lockstep on host buffers, every output compared bit for bit.  each_tick(tick, state, gn) sees every tick's input
    states and the default context's outputs; a true return value ends the flight."""
    def same(tick, state, traj, outs):
        assert_lockstep(new, old, tick, outs)
        return each_tick and each_tick(tick, state, outs[0])
    return fly((new, old), ms, ticks, each_tick=same, **kw)


def test_every_table_row(L, monkeypatch):
    """Case 1's mission from its first tick until every agent rests on its goal: the goal wave picks gi_hz and the unconstrained optimum by
    its own T, and every row T = 1 .. M of the two tables is picked on the way (T recomputed on the host from the planned goals, the
    states and vnom; that the mission shows all of them is a condition on the mission, checked on the CPU oracle: see CIRCLE_R)."""
    ms = _circle(L)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15), monkeypatch, ENV, NEW, OLD)
    seen = set()

    def rows_picked(tick, state, gn):
        assert (gn["status"] == 0).all(), (tick, gn["status"])
        seen.update(int(t) for t in _terminal_segments(new.last_goals(), state, ms.nominal_velocity, new.M, new.cfg.dt))
        arrived[0] = bool((np.abs(state[:, :3] - ms.goal).max(1) < ARRIVED).all())
        return arrived[0] and len(seen) == new.M          # (the flight ends early once there is nothing left to see)
    arrived = [False]
    _fly(new, old, ms, CAP, each_tick=rows_picked)
    assert arrived[0], "not every agent arrived"
    assert seen == set(range(1, new.M + 1)), seen
    st = new.solver_stats()
    assert st["solved"] > 10 * st["handed_over"], st      # (planned by the active-set solve; a hand-over is the rare exception)
    new.close(); old.close()


def test_first_tick_static_goals(L, monkeypatch):
    """Static goals, reset_threshold 0 (lsc_plan_kernel, without the alternate-mode hooks): tick 1 builds the initial trajectories from the
    states (planner_seq < 2), and the early start reads the goal the goal wave wrote through."""
    ms = _circle(L, 4, 1.0)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="static", reset_threshold=0.0), monkeypatch, ENV, NEW, OLD)

    def goals_are_the_input(tick, state, gn):
        assert same_bits(new.last_goals(), ms.goal), tick
    _fly(new, old, ms, 4, each_tick=goals_are_the_input)
    new.close(); old.close()


def test_two_agents_without_a_row(L, monkeypatch):
    """Two agents 20 m apart on parallel courses: no LSC row survives (nact = 0), the loop over the own rows' scales runs zero times and the
    first search meets the axis rows alone."""
    ms = _circle(L, 2, 10.0)
    ms.goal = (ms.start + np.asarray([0.0, 3.0, 0.0], np.float32)).astype(np.float32)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15), monkeypatch, ENV, NEW, OLD)

    def no_rows(tick, state, gn):
        assert (new.row_counts() == 0).all(), (tick, new.row_counts())
    _fly(new, old, ms, 12, each_tick=no_rows)
    new.close(); old.close()


@pytest.mark.parametrize("n", [65, 66])
def test_largest_swarm_of_the_path_and_the_first_beyond(L, monkeypatch, n):
    """65 agents: 64 obstacles, the largest swarm with wave roles.  66 agents: both contexts take the generic pass -- the `else` of the early
    start -- and their notes say so."""
    R = 8.0 * n / 64.0
    ms = _circle(L, n, R)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15), monkeypatch, ENV, NEW if n <= 65 else BEYOND, OLD)
    _fly(new, old, ms, 25)
    new.close(); old.close()


@pytest.mark.parametrize("solver", ["hand_over", "interior_point"])
def test_hand_over_after_an_early_start(L, monkeypatch, solver):
    """hand_over: the active-set solve runs and EVERY agent is handed to the interior point, which must find the arrays the helper waves used
    (S.as_, S.az, S.at2, S.K, S.y) as it expects them.  interior_point: the SOLVER == 0 instantiations, which start nothing early."""
    ms = _circle(L)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15, solver=solver), monkeypatch, ENV, NEW, OLD)

    _fly(new, old, ms, 20)
    if solver == "hand_over":
        st = new.solver_stats()
        assert st["handed_over"] == 20 * ms.qn and st["solved"] == 0, st
    new.close(); old.close()


def test_disturbed_swarm(L, monkeypatch):
    """One gust beyond reset_threshold on one agent at tick 5: S.gen is set, no solve runs in plan_agent, and the folded general solver plans
    every agent in the same launch -- behind the stores of the helper waves."""
    ms = _circle(L)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15), monkeypatch, ENV, NEW, OLD)
    ran_here = {}

    def count(tick, state, gn):
        st = new.solver_stats()
        ran_here[tick] = st["solved"] + st["handed_over"]
    _fly(new, old, ms, 10, gusts={5: (3, (0.25, -0.2, 0.0))}, each_tick=count)
    assert ran_here[4] > ran_here[3] > 0, ran_here
    assert all(ran_here[t] == ran_here[4] for t in range(5, 11)), ran_here      # from the gust on: nobody is planned by the plan kernel's own solve
    new.close(); old.close()


def test_planar_world(L, monkeypatch):
    """world/dimension 2 (lsc_plan_kernel<false, true, 1> takes the path): the z unknowns of the early optimum rest at z_2d."""
    ms = _circle(L, 6, 1.5)
    cfg = L.PlannerConfig(goal_mode="prior_based", world_dimension=2, world_z_2d=1.0)
    new, old = held_pair(L, ms, cfg, monkeypatch, ENV, NEW, OLD)

    def at_z2d(tick, state, gn):
        assert (gn["traj"][:, 2, :] == np.float32(1.0)).all(), tick
    _fly(new, old, ms, 30, planar_z=1.0, each_tick=at_z2d)
    new.close(); old.close()


def test_four_segment_library(L, monkeypatch):
    """M = 4 (dt 0.5, horizon 2.0: liblsc_hip_m4.so): four segment waves, three copy waves, tables of 24 x NYA doubles."""
    L.load_library(4)
    ms = _circle(L)
    new, old = held_pair(L, ms, L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15, dt=0.5, horizon=2.0), monkeypatch, ENV, NEW, OLD)
    assert new.M == 4

    _fly(new, old, ms, 20)
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
        return [t.cpu().numpy().copy() for t in (self.next, self.states[1], self.cost, self.status, self.iters)]

    def advance(self):
        self.states.reverse()
        self.prev, self.next = self.next, self.prev


def test_batch_launch(L, monkeypatch):
    """Two 8-agent missions as blocks of one launch (lsc_tick_device_fused_batch: lsc_plan_batch_kernel runs the same plan_agent) against the
    same two flown alone, by a default and by a generic-pass context each."""
    import torch
    cfg = lambda: L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15)
    missions = [_circle(L), _circle(L, CIRCLE_N, 0.8)]
    groups = []          # the batch, alone, alone on the generic pass
    for generic in (False, False, True):
        runs = []
        for ms in missions:
            pl = held_planner(L, ms, cfg, monkeypatch, ENV, generic, OLD if generic else NEW)
            runs.append(_DeviceRun(torch, pl, ms))
        groups.append(runs)
    st = torch.cuda.current_stream().cuda_stream
    names = ("traj", "state_next", "cost", "status", "iters")
    for tick in range(1, 21):
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
            for other in (1, 2):
                for k, (a, b) in enumerate(zip(outs[0][s], outs[other][s])):
                    assert same_bits(a, b), (tick, s, ("alone", "alone, generic pass")[other - 1], names[k])
        for runs in groups:
            for r in runs:
                r.advance()
    for runs in groups:
        for r in runs:
            r.pl.close()


def test_poison_build_solve_start():
    """The whole file once more through the LDS-poison libraries (every byte of the workgroup's LDS is 0xff at entry): a slot the early start
    stopped writing, or writes behind its first reader, is a NaN in the first search -- a failed plan."""
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
