"""-m gpu: the size classes of the active-set solve's step (csrc/lsc_kernels.hip, gi_solve: a change of the working set runs its loops over
4, 8 or 12 slots -- the smallest class that covers the largest working set the solve has held so far --, and takes the indices of the
row's variables without dividing) against the statements they replace, which LSC_STEP_ALL_SLOTS at context creation keeps a context on:
every change over all 12 slots.

Every test flies a default context and an all-slots context in lockstep on the same host-buffer inputs and compares plans, costs, statuses,
iteration counts, planned goals, row counts, the counters of lsc_solver_stats and the working-set peaks bit for bit at every tick.  Which
classes a mission enters is read from lsc_working_set_peaks (1-4, 5-8, 9-12; 13 = the solve asked for a thirteenth row and handed the agent
over); that a mission shows the classes named in its test is a condition on the mission, found on the GPU with that counter, and asserted.
"""
import os

import numpy as np
import pytest

from harness import assert_lockstep, circle, fly, held_pair, held_planner, same_bits, start_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "LSC_STEP_ALL_SLOTS"
NEW, OLD = "step: size classes", "step: all slots (LSC_STEP_ALL_SLOTS)"
OUTPUTS = ("traj", "cost", "status", "iters")


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


def _counted(pl):
    assert (pl.working_set_peaks() == 0).all()          # (the first call switches the counter on)
    return pl


def _counted_pair(L, ms, cfg, monkeypatch):
    """(default context, context held to all slots), each checked through its note."""
    return tuple(_counted(pl) for pl in held_pair(L, ms, cfg, monkeypatch, ENV, NEW, OLD))


class _Seen:
    """What the solves of a flight showed: agent-ticks per class of the working set's peak, and per class the agent-ticks that the solve
    finished (status 0) with more changes than its peak -- at least one row left the working set on the way."""

    def __init__(self):
        self.peak, self.dropped, self.status = np.zeros(4, int), np.zeros(3, int), {}

    def add(self, peaks, g):
        for p, it, s in zip(peaks, g["iters"], g["status"]):
            self.status[int(s)] = self.status.get(int(s), 0) + 1
            if p >= 1:
                self.peak[(min(int(p), 13) - 1) // 4] += 1
            if 1 <= p <= 12 and s == 0 and it > p:
                self.dropped[(int(p) - 1) // 4] += 1


def _fly(new, old, ms, ticks, seen=None, **kw):
    """Both contexts in lockstep on host buffers, every output, diagnostic and counter compared bit for bit."""
    seen = seen or _Seen()

    def same(tick, state, traj, outs):
        assert_lockstep(new, old, tick, outs, keys=OUTPUTS, diagnostics=("last_goals", "row_counts", "solver_stats", "working_set_peaks"))
        seen.add(new.working_set_peaks(), outs[0])
    fly((new, old), ms, ticks, each_tick=same, **kw)
    return seen


def _prior(L):
    return lambda: L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15)


def test_every_class_drops_and_the_thirteenth_row(L, monkeypatch):
    """Twelve agents swap across a circle of 1.5 m: the crossing (from tick 29 on) fills working sets of every size.  Seen on the GPU over 60
    ticks: peaks of 1-4, 5-8 and 9-12 rows in 411, 187 and 69 agent-ticks, 37 solves that asked for a thirteenth row (code 2: handed over),
    and in every class solves that took more changes than their peak -- rows left the working set while the high-water mark stayed above
    (67 / 101 / 14 agent-ticks): the slots in [q, qhw) then hold stale values, which is why the class goes by qhw."""
    ms = circle(L, 12, 1.5)
    new, old = _counted_pair(L, ms, _prior(L), monkeypatch)
    seen = _fly(new, old, ms, 60)
    assert (seen.peak > 0).all(), seen.peak            # classes 4, 8, 12 entered; peak[3]: a thirteenth row asked for
    assert (seen.dropped > 0).all(), seen.dropped      # iters > peak for a finished solve of every class
    st = new.solver_stats()
    assert st["handed_over"] >= seen.peak[3] > 0 and st["solved"] > st["handed_over"], st
    new.close(); old.close()


def test_circle_of_eight(L, monkeypatch):
    """The 8-agent circle of tests/test_gpu_solve_start.py at 1.2 m, where the swap meets infeasible QPs around tick 50: every class, a
    thirteenth row and the interior point's verdicts behind a hand-over, on the kernel with the alternate-mode hooks."""
    ms = circle(L, 8, 1.2)
    new, old = _counted_pair(L, ms, _prior(L), monkeypatch)
    seen = _fly(new, old, ms, 60)
    assert (seen.peak > 0).all() and (seen.dropped > 0).all(), (seen.peak, seen.dropped)
    assert seen.status.get(1, 0) > 0, seen.status
    new.close(); old.close()


def test_random_swarm_without_the_hooks(L, monkeypatch):
    """Twenty agents at random in a 3 m box, no disturbance checks (lsc_plan_kernel, without the alternate-mode hooks): classes 4 and 8."""
    ms = L.random_swarm(20, world=(-1.5, -1.5, 0, 1.5, 1.5, 3.0), seed=2, min_sep=0.35, shrink=0.2)
    new, old = _counted_pair(L, ms, lambda: L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.0), monkeypatch)
    seen = _fly(new, old, ms, 30)
    assert seen.peak[0] > 0 and seen.peak[1] > 0, seen.peak
    new.close(); old.close()


def test_infeasible_by_the_certificate(L, monkeypatch):
    """An agent inside another's collision model (the scene of test_active_set_solver_statistics_and_hand_over): no admissible step, and the
    verdict is the active-set solve's own -- status 1 with nothing handed over --, formed from rwv[lane < q] behind a step of class 4 or 8."""
    ms = L.circle_swap(3, circle_radius=2.0, z=1.0, world=(-5, -5, 0, 5, 5, 2.5))
    ms.start[1] = ms.start[0] + np.array([0.05, 0.0, 0.0], np.float32)
    new, old = _counted_pair(L, ms, lambda: L.PlannerConfig(), monkeypatch)
    seen = _fly(new, old, ms, 2)
    st = new.solver_stats()
    assert seen.status.get(1, 0) > 0 and st["handed_over"] == 0 and st["solved"] == 2 * ms.qn, (seen.status, st)
    assert seen.peak[2] == 0 and seen.peak[3] == 0, seen.peak          # (the certificates of this scene come from small working sets)
    new.close(); old.close()


def test_every_agent_handed_over(L, monkeypatch):
    """solver = hand_over (lsc_config.solver 2): the solve runs through its classes, then the interior point plans every agent."""
    ms = circle(L, 8, 1.0)
    new, old = _counted_pair(L, ms, lambda: L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15, solver="hand_over"), monkeypatch)
    seen = _fly(new, old, ms, 20)
    st = new.solver_stats()
    assert st["handed_over"] == 20 * ms.qn and st["solved"] == 0, st
    assert seen.peak[0] > 0, seen.peak
    new.close(); old.close()


def test_two_agents_without_a_row(L, monkeypatch):
    """Two agents 20 m apart on parallel courses: no LSC row survives, the working set grows on axis rows alone."""
    ms = circle(L, 2, 10.0)
    ms.goal = (ms.start + np.asarray([0.0, 3.0, 0.0], np.float32)).astype(np.float32)
    new, old = _counted_pair(L, ms, _prior(L), monkeypatch)
    seen = _fly(new, old, ms, 12)
    assert (new.row_counts() == 0).all(), new.row_counts()
    assert seen.peak[0] > 0, seen.peak
    new.close(); old.close()


def test_planar_world(L, monkeypatch):
    """world/dimension 2 (the planar instantiations): classes 4 and 8 with the z unknowns at rest."""
    ms = circle(L, 6, 1.5)
    new, old = _counted_pair(L, ms, lambda: L.PlannerConfig(goal_mode="prior_based", world_dimension=2, world_z_2d=1.0), monkeypatch)
    seen = _fly(new, old, ms, 30, planar_z=1.0)
    assert seen.peak[0] > 0 and seen.peak[1] > 0, seen.peak
    new.close(); old.close()


def test_four_segment_library(L, monkeypatch):
    """M = 4 (liblsc_hip_m4.so): the 8-agent circle, then the instance of tests/golden/fuzz_found_m4_handover_8500018.npz, whose agent 9
    needs more than 12 rows: its solve walks through all three classes before it is handed over."""
    from lsc_planner_amd.mission import Mission
    L.load_library(4)
    cfg = lambda: L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15, dt=0.5, horizon=2.0)
    ms = circle(L, 8, 1.0)
    new, old = _counted_pair(L, ms, cfg, monkeypatch)
    assert new.M == 4
    seen = _fly(new, old, ms, 20)
    assert seen.peak[0] > 0, seen.peak
    new.close(); old.close()
    d = np.load(os.path.join(ROOT, "tests", "golden", "fuzz_found_m4_handover_8500018.npz"))
    ms = Mission(d["state"][:, :3].copy(), d["goal"].copy(), d["wmin"], d["wmax"], d["radius"], d["dw"], d["vmax"], d["amax"], d["vnom"], name="replay")
    new, old = _counted_pair(L, ms, lambda: L.PlannerConfig(goal_mode="static", dt=0.5, horizon=2.0, warm_start_mu=0.0), monkeypatch)
    seen = _Seen()
    for _ in range(2):          # (sequence number 1 takes the current-velocity model: only to move it on)
        gn, go = new.plan(d["state"], d["goal"], d["traj"]), old.plan(d["state"], d["goal"], d["traj"])
        for k in OUTPUTS:
            assert same_bits(gn[k], go[k]), k
        assert new.solver_stats() == old.solver_stats()
        peaks = new.working_set_peaks()
        assert same_bits(peaks, old.working_set_peaks())
    seen.add(peaks, gn)
    assert peaks[9] == 13 and seen.peak[3] >= 1, peaks
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
    """Two missions as blocks of one launch (lsc_tick_device_fused_batch: lsc_plan_batch_kernel runs the same gi_solve; each block carries
    its context's switch and counter) against the same two flown alone, by a default and by an all-slots context each."""
    import torch
    missions = [circle(L, 8, 1.2), circle(L, 8, 1.0)]
    groups = []          # the batch, alone, alone over all slots
    for all_slots in (False, False, True):
        note = OLD if all_slots else NEW
        groups.append([_DeviceRun(torch, _counted(held_planner(L, ms, _prior(L), monkeypatch, ENV, all_slots, note)), ms) for ms in missions])
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
                    assert same_bits(a, b), (tick, s, ("alone", "alone, all slots")[other - 1], names[k])
        for runs in groups:
            for r in runs:
                r.advance()
    assert top >= 5, top          # (the batch reached class 8)
    for runs in groups:
        for r in runs:
            r.pl.close()


def test_throughput_build(L, monkeypatch):
    """300 agents on one chip: more agents than CUs, the 256-lane build (lsc_plan_alt_tp_kernel) runs the same gi_solve."""
    R = 8.0 * 300 / 64.0
    ms = circle(L, 300, R)
    new, old = _counted_pair(L, ms, _prior(L), monkeypatch)
    seen = _fly(new, old, ms, 3)
    assert seen.peak[0] > 0, seen.peak
    new.close(); old.close()


def test_fuzzed_missions(L, monkeypatch):
    """50 trials of the generator of tests/fuzz_lsc.py (the same draws: crowded and empty worlds, goals outside the world, nearly coincident
    agents, agents at their goals, moving first ticks), eight ticks each through both contexts: whatever one side hands to the interior
    point the other must hand over too -- statuses, iteration counts and the counters of lsc_solver_stats are equal at every tick."""
    from lsc_planner_amd.mission import Mission
    seed0, seen, handed = 20261019, _Seen(), 0
    for trial in range(50):
        rng = np.random.default_rng(seed0 + trial)
        n = int(rng.integers(1, 14))
        side = float(rng.uniform(0.8, 6.0)); zt = float(rng.uniform(0.6, 3.0))
        wmin = np.array([-side, -side, 0], np.float32); wmax = np.array([side, side, zt], np.float32)
        kind = rng.integers(0, 4)
        start = rng.uniform(wmin + 0.05, wmax - 0.05, (n, 3)).astype(np.float32)
        goal = rng.uniform(wmin - 0.3, wmax + 0.3, (n, 3)).astype(np.float32)
        if kind == 1 and n > 1:
            start[1] = start[0] + np.float32(1e-3)
        if kind == 2:
            goal[:] = start
        radius = rng.uniform(0.05, 0.4, n); dw = rng.uniform(1.0, 3.0, n)
        vmax = np.repeat(rng.uniform(0.2, 3.0, (n, 1)), 3, 1); amax = np.repeat(rng.uniform(0.5, 6.0, (n, 1)), 3, 1)
        if kind == 3:
            vmax[:, 2] *= 0.3; amax[:, 2] *= 0.5
        vnom = rng.uniform(0.3, 2.0, n)
        ms = Mission(start, goal, wmin, wmax, radius, dw, vmax, amax, vnom, name="fuzz")
        mode = "prior_based" if trial % 2 else "static"
        new, old = _counted_pair(L, ms, lambda: L.PlannerConfig(goal_mode=mode), monkeypatch)
        state = start_inputs(ms, new.SEGV)[0]
        if trial % 3 == 0:
            state[:, 3:6] = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
        _fly(new, old, ms, 8, state=state, seen=seen)
        handed += new.solver_stats()["handed_over"]
        new.close(); old.close()
    assert seen.peak[0] > 0 and seen.peak[1] > 0, seen.peak
    assert handed > 0          # (hand-overs occurred, and each of them on both sides)
