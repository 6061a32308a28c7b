"""-m gpu: LSC rows against the mission's dynamic obstacles (lsc_set_obstacles / lsc_obstacle_states; csrc/lsc_kernels.hip: the OBS
instantiations of plan_agent) against the composed reference tick of tests/obstacle_reference.py.

Rows (normals, margins), statuses and planned goals are compared bit for bit; cost by COST_RTOL / COST_ATOL; plans by ACTIVE_SET_TRAJ_ATOL
under the active-set solve and by INTERIOR_POINT_TRAJ_ATOL where a test sends agents to the interior point on purpose (solver 0, solver 2,
the second pass).  The obstacles' columns of the dense dumps follow the N - 1 agents' columns.
"""
import csv
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_octomap_batch import mission, suite  # noqa: F401  (the forest suite's fixture and reader)
from obstacle_reference import (HOVER_DOWNWASH, HOVER_RADIUS, HOVER_TICKS, ObstacleSwarm, hover_mission, hover_states, sim_mission_doc)
from harness import assert_tick_matches, start_inputs
from tolerances import ACTIVE_SET_TRAJ_ATOL, COST_ATOL, INTERIOR_POINT_TRAJ_ATOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -1, -5


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


def _cfg(L, **kw):
    kw.setdefault("solver", "active_set")
    return L.PlannerConfig(**kw)


def _compare(g, r, atol, what, rows="bits"):
    """GPU tick g against reference tick r on the same inputs: rows through their integer views, cost with the absolute floor."""
    assert_tick_matches(g, r, what, rows=rows, cost_atol=COST_ATOL, traj_atol=atol)


def _two_agents(L, n=2):
    if n == 1:
        ms = L.circle_swap(2, circle_radius=1.5, world=(-5, -5, 0, 5, 5, 2.5))
        return L.Mission(ms.start[:1].copy(), ms.goal[:1].copy(), ms.world_min, ms.world_max, ms.radius[:1].copy(), ms.downwash[:1].copy(),
                         ms.max_vel[:1].copy(), ms.max_acc[:1].copy(), ms.nominal_velocity[:1].copy())
    return L.circle_swap(n, circle_radius=1.5, world=(-5, -5, 0, 5, 5, 2.5))


@pytest.mark.parametrize("n", [2, 1])
def test_smallest_shapes(L, oracle, n):
    """N = 2 (and 1) agents, K = 1 obstacle drifting across their path, ticks 1 .. 5 fed by the kernel's own plans; checked at planner_seq
    1, 2 and 5: the obstacle's columns of the dump are lsc_pair's bits, the agents' columns those of the same tick without obstacles."""
    from lsc_planner_amd.planner import next_state_host
    ms = _two_agents(L, n)
    rad, dw = np.array([0.3]), np.array([1.5])
    pos0, vel = np.array([[0.2, -0.6, 1.1]]), np.array([[0.0, 0.12, 0.0]], np.float32)
    pl, alone = L.SwarmPlanner(ms, _cfg(L)), L.SwarmPlanner(ms, _cfg(L))
    pl.set_obstacles(rad, dw)
    ref = ObstacleSwarm(oracle, ms, rad, dw)
    state, traj = start_inputs(ms, pl.SEGV)
    for seq in range(1, 6):
        pos = (pos0 + vel * (0.2 * (seq - 1))).astype(np.float32)
        pl.obstacle_states(pos, vel)
        g = pl.plan(state, ms.goal, traj, want_constraints=True)
        a = alone.plan(state, ms.goal, traj, want_constraints=True)
        assert g["normal"].shape == (n, n - 1 + 1, 5, 3) and g["d"].shape == (n, n, 5, 6)
        if seq in (1, 2, 5):
            r = ref.tick(state, ms.goal, traj, seq, pos, vel)
            # the obstacle is predicted from its CURRENT state at every planner_seq: its last segment moves (a shifted plan would rest there)
            last = oracle.const_vel_traj(pos[0], vel[0])[:, 24:]
            assert np.ptp(last[1]) > 0.01
            _compare(g, r, ACTIVE_SET_TRAJ_ATOL, (n, seq))
            if n > 1:
                assert np.array_equal(g["normal"][:, :n - 1], a["normal"]) and np.array_equal(g["d"][:, :n - 1], a["d"]), (n, seq)
        else:
            ref.stale[:] = g["traj"]
        traj = g["traj"]
        state = next_state_host(traj)
    pl.close(); alone.close()


def test_downwash_rule_of_a_non_agent_obstacle(L, oracle):
    """Agent downwash 2.0, obstacle downwash 1.5, the obstacle 0.4 m above agent 0's path: rows bit for bit -- and not the agents' formula's."""
    ms = _two_agents(L)
    assert (ms.downwash == 2.0).all()
    rad, dw = np.array([0.25]), np.array([1.5])
    pos = (ms.start[:1] + np.array([[-0.3, 0.0, 0.4]])).astype(np.float32)
    vel = np.zeros((1, 3), np.float32)
    pl = L.SwarmPlanner(ms, _cfg(L))
    pl.set_obstacles(rad, dw)
    pl.obstacle_states(pos, vel)
    state, traj = start_inputs(ms, pl.SEGV)
    g = pl.plan(state, ms.goal, traj, want_constraints=True)
    r = ObstacleSwarm(oracle, ms, rad, dw).tick(state, ms.goal, traj, 1, pos, vel)
    _compare(g, r, ACTIVE_SET_TRAJ_ATOL, "downwash")
    init = oracle.const_vel_traj(state[0, :3], state[0, 3:6])
    wrong_n, wrong_d = oracle.lsc_pair(init, oracle.const_vel_traj(pos[0], vel[0]), 0.15, float(np.float32(0.25)), 2.0, float(np.float32(1.5)))
    assert not (np.array_equal(g["normal"][0, 1], wrong_n) and np.array_equal(g["d"][0, 1], wrong_d))
    pl.close()


class _Device:
    """Device-resident fused ticks of one context, the obstacles' states in a device buffer of the caller's."""

    def __init__(self, torch, pl, ms, K):
        dev = torch.device("cuda", 0)
        self.torch, self.pl, N = torch, pl, ms.qn
        s0 = np.zeros((N, 9), np.float32); s0[:, :3] = ms.start
        self.goal = torch.from_numpy(np.ascontiguousarray(ms.goal, np.float32)).to(dev)
        self.states = [torch.from_numpy(s0).to(dev), torch.zeros((N, 9), device=dev)]
        self.prev, self.next = torch.zeros((N, 3 * pl.SEGV), device=dev), torch.zeros((N, 3 * pl.SEGV), device=dev)
        self.cost = torch.zeros(N, dtype=torch.float64, device=dev)
        self.status = torch.zeros(N, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(N, dtype=torch.int32, device=dev)
        self.pos_vel = torch.zeros((K, 6), device=dev)
        pl.obstacle_states(self.pos_vel)

    def tick(self, seq, pos, vel):
        t = self.torch
        self.pos_vel.copy_(t.from_numpy(np.concatenate([pos, vel], axis=1)))      # (on the current stream: in front of the tick)
        self.pl.tick_device_fused(self.states[0], self.goal, self.prev, self.next, self.states[1], self.cost, self.status, self.iters, seq,
                                  t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        out = [x.cpu().numpy().copy() for x in (self.next, self.states[1], self.cost, self.status)]
        self.states.reverse()
        self.prev, self.next = self.next, self.prev
        return out


def test_hover_closed_loop_host_and_device(L, oracle):
    """The hover scenario, 50 ticks through lsc_replan_tick, the kernel's own plans feeding the next tick: every agent-tick against the
    reference on the same inputs.  The same 50 ticks through lsc_tick_device_fused with lsc_obstacle_states_device give the same bits."""
    import torch
    from lsc_planner_amd.planner import next_state_host
    ms = hover_mission()
    pl, alone, dv = L.SwarmPlanner(ms, _cfg(L)), L.SwarmPlanner(ms, _cfg(L)), L.SwarmPlanner(ms, _cfg(L))
    pl.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH)
    dv.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH)
    run = _Device(torch, dv, ms, 3)
    ref = ObstacleSwarm(oracle, ms, HOVER_RADIUS, HOVER_DOWNWASH)
    state, traj = start_inputs(ms, pl.SEGV)
    moved = 0
    for j in range(1, HOVER_TICKS + 1):
        pos, vel = hover_states(j)
        pl.obstacle_states(pos, vel)
        g = pl.plan(state, ms.goal, traj, want_constraints=True)
        r = ref.tick(state, ms.goal, traj, j, pos, vel)
        _compare(g, r, ACTIVE_SET_TRAJ_ATOL, j)
        a = alone.plan(state, ms.goal, traj)
        moved += int((np.abs(g["traj"] - a["traj"]).max(axis=(1, 2)) > 1e-3).sum())
        d_traj, d_state, d_cost, d_status = run.tick(j, pos, vel)
        assert np.array_equal(d_traj.reshape(8, 3, 30), g["traj"]) and np.array_equal(d_cost, g["cost"]) and np.array_equal(d_status, g["status"]), j
        traj = g["traj"]
        state = next_state_host(traj)              # (the device loop is fed by its own fused propagation: plans that stay equal prove the states)
        ref.stale[:] = traj
    print("agent-ticks whose plan the obstacles moved by more than 1e-3 m:", moved)
    assert moved >= 10, moved
    for p in (pl, alone, dv):
        p.close()


def test_generic_build_gives_the_same_bits(L, monkeypatch):
    """LSC_GENERIC_LSC_BUILD (the generic pass instead of one wave per segment) against the default, hover, 12 ticks, dumps included."""
    from lsc_planner_amd.planner import next_state_host
    ms = hover_mission()
    new = L.SwarmPlanner(ms, _cfg(L))
    monkeypatch.setenv("LSC_GENERIC_LSC_BUILD", "1")
    old = L.SwarmPlanner(ms, _cfg(L))
    monkeypatch.delenv("LSC_GENERIC_LSC_BUILD")
    assert "generic pass (LSC_GENERIC_LSC_BUILD)" in old.note() and "one wave per segment" in new.note()
    state, traj = start_inputs(ms, new.SEGV)
    for j in range(1, 13):
        pos, vel = hover_states(j)
        outs = []
        for p in (new, old):
            if j == 1:
                p.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH)
            p.obstacle_states(pos, vel)
            outs.append(p.plan(state, ms.goal, traj, want_constraints=True))
        for k in ("traj", "cost", "status", "iters", "normal", "d"):
            assert np.array_equal(outs[0][k], outs[1][k]), (j, k)
        assert np.array_equal(new.row_counts(), old.row_counts()) and np.array_equal(new.bucket_max(), old.bucket_max())
        traj = outs[0]["traj"]
        state = next_state_host(traj)
    new.close(); old.close()


def _crowd(L, n, k, seed):
    """n agents on a circle and k small spheres drifting about inside it."""
    R = 8.0 * n / 64.0
    ms = L.circle_swap(n, circle_radius=R, world=(-R - 2, -R - 2, 0, R + 2, R + 2, 2.5))
    rng = np.random.default_rng(seed)
    ang, rad = rng.uniform(0, 2 * np.pi, k), R * (0.2 + 0.7 * np.sqrt(rng.uniform(0, 1, k)))
    pos = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(0.6, 1.6, k)], axis=1).astype(np.float32)
    vel = (rng.normal(size=(k, 3)) * [0.05, 0.05, 0.01]).astype(np.float32)
    return ms, pos, vel, rng.uniform(0.1, 0.3, k), rng.uniform(1.0, 2.0, k)


@pytest.mark.parametrize("n,k", [(60, 5), (60, 6), (70, 40)])
def test_boundaries_of_the_lsc_builds(L, oracle, n, k):
    """64 and 65 obstacles per agent -- the boundary of the one-wave-per-segment build -- and 109 (more than 512 units: the in-kernel
    cull of the generic pass runs when no dump is asked for).  One tick each against the reference, with and without the dumps."""
    ms, pos, vel, rad, dw = _crowd(L, n, k, 100 * n + k)
    pl = L.SwarmPlanner(ms, _cfg(L))
    pl.set_obstacles(rad, dw)
    assert ("one wave per segment" in pl.note()) == (n - 1 <= 64)        # (the note speaks of the agents; the build is chosen per tick by N - 1 + K)
    # ... and lsc_set_obstacles adds a remark of its own that goes by N - 1 + K
    build = "generic pass (more than 64 obstacles)" if n - 1 + k > 64 else "one wave per segment"
    assert f"dynamic obstacles: K = {k}, {n - 1 + k} per agent, {build}" in pl.note(), pl.note()
    pl.obstacle_states(pos, vel)
    state, traj = start_inputs(ms, pl.SEGV)
    r = ObstacleSwarm(oracle, ms, rad, dw).tick(state, ms.goal, traj, 1, pos, vel)
    g = pl.plan(state, ms.goal, traj, want_constraints=True)
    _compare(g, r, ACTIVE_SET_TRAJ_ATOL, (n, k, "dumps"))
    pl.planner_seq = 0
    g2 = pl.plan(state, ms.goal, traj)
    _compare(g2, r, ACTIVE_SET_TRAJ_ATOL, (n, k), rows=False)
    pl.close()


def test_second_pass_with_rows_in_hbm(L, oracle):
    """max_rows_per_cp = 1 and no pruning: 27 rows fit the LDS pass, every agent carries 27 x 10 and is planned by the second pass."""
    from lsc_planner_amd.planner import next_state_host
    ms = hover_mission()
    pl = L.SwarmPlanner(ms, _cfg(L, max_rows_per_cp=1, prune=False))
    pl.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH)
    assert pl.row_capacity()[0] == 27
    ref = ObstacleSwarm(oracle, ms, HOVER_RADIUS, HOVER_DOWNWASH)
    state, traj = start_inputs(ms, pl.SEGV)
    for j in range(1, 4):
        pos, vel = hover_states(j)
        pl.obstacle_states(pos, vel)
        g = pl.plan(state, ms.goal, traj, want_constraints=True)
        assert (pl.row_counts() == 27 * 10).all(), pl.row_counts()
        _compare(g, ref.tick(state, ms.goal, traj, j, pos, vel), INTERIOR_POINT_TRAJ_ATOL, j)
        traj = g["traj"]; state = next_state_host(traj); ref.stale[:] = traj
    pl.close()


@pytest.mark.parametrize("solver", ["interior_point", "active_set", "hand_over"])
def test_every_solver(L, oracle, solver):
    from lsc_planner_amd.planner import next_state_host
    ms = hover_mission()
    pl = L.SwarmPlanner(ms, L.PlannerConfig(solver=solver))
    pl.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH)
    ref = ObstacleSwarm(oracle, ms, HOVER_RADIUS, HOVER_DOWNWASH)
    state, traj = start_inputs(ms, pl.SEGV)
    for j in range(1, 9):
        pos, vel = hover_states(j)
        pl.obstacle_states(pos, vel)
        g = pl.plan(state, ms.goal, traj, want_constraints=True)
        _compare(g, ref.tick(state, ms.goal, traj, j, pos, vel), ACTIVE_SET_TRAJ_ATOL if solver == "active_set" else INTERIOR_POINT_TRAJ_ATOL, (solver, j))
        traj = g["traj"]; state = next_state_host(traj); ref.stale[:] = traj
    pl.close()


def test_the_four_segment_library(L, oracle):
    """dt 0.5 / horizon 2.0 (liblsc_hip_m4.so), two ticks, the reference on the oracle built for M = 4."""
    from lsc_planner_amd.planner import next_state_host
    ms = hover_mission()
    pl = L.SwarmPlanner(ms, _cfg(L, dt=0.5, horizon=2.0))
    assert pl.M == 4
    pl.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH)
    with oracle.segments(4):
        ref = ObstacleSwarm(oracle, ms, HOVER_RADIUS, HOVER_DOWNWASH, dt=0.5)
        state, traj = start_inputs(ms, pl.SEGV)
        for j in (1, 2):
            pos, vel = hover_states(j, dt=0.5)
            pl.obstacle_states(pos, vel)
            g = pl.plan(state, ms.goal, traj, want_constraints=True)
            assert g["normal"].shape == (8, 10, 4, 3)
            _compare(g, ref.tick(state, ms.goal, traj, j, pos, vel), ACTIVE_SET_TRAJ_ATOL, ("m4", j))
            traj = g["traj"]; state = next_state_host(traj, dt=0.5); ref.stale[:] = traj
    pl.close()


def test_lds_poison_library():
    """The smallest shapes, the closed loop, both builds and the second pass once more through the LDS-poison libraries."""
    lib = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_poison.so")
    lib4 = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_m4_poison.so")
    assert os.path.exists(lib) and os.path.exists(lib4), "the poison libraries are not built (make -C lsc_planner_amd/csrc poison poison_m4)"
    env = dict(os.environ, LSC_HIP_LIB=lib, LSC_HIP_LIB_M4=lib4)
    env.pop("LSC_GENERIC_LSC_BUILD", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "smallest_shapes or generic_build or second_pass or four_segment or boundaries"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]


@pytest.fixture(scope="module")
def forest(L, suite):
    """Mission 1 of the reference's forest suite, its first four agents, and its world file."""
    return mission(L, suite, "forest", 1, 4)


@pytest.mark.parametrize("goal_mode", ["static", "prior_based"])
def test_octomap_world(L, oracle, forest, goal_mode):
    """The forest, N = 4, K = 2 spheres next to two agents' ways: planned goals and corridor boxes are those of the same tick without
    obstacles, bit for bit -- goal planning and the corridor never see them --, plans against the reference with those boxes and goals."""
    from lsc_planner_amd.planner import next_state_host
    ms, bt = forest
    rad, dw = np.array([0.2, 0.25]), np.array([1.0, 2.0])
    step = (ms.goal - ms.start) / np.linalg.norm(ms.goal - ms.start, axis=1, keepdims=True)
    pos0 = (ms.start[:2] + 0.9 * step[:2] + np.array([[0.0, 0.25, 0.1], [0.2, 0.0, -0.1]])).astype(np.float64)
    vel = np.array([[0.03, 0.0, 0.0], [0.0, -0.03, 0.0]], np.float32)
    pl, alone = L.SwarmPlanner(ms, _cfg(L, use_octomap=True, goal_mode=goal_mode)), L.SwarmPlanner(ms, _cfg(L, use_octomap=True, goal_mode=goal_mode))
    pl.load_octomap(bt); alone.load_octomap(bt)
    pl.set_obstacles(rad, dw)
    ref = ObstacleSwarm(oracle, ms, rad, dw, use_sfc=True)
    state, traj = start_inputs(ms, pl.SEGV)
    differs = False
    for j in range(1, 7):
        pos = (pos0 + vel * (0.2 * (j - 1))).astype(np.float32)
        pl.obstacle_states(pos, vel)
        g = pl.plan(state, ms.goal, traj, want_constraints=True)
        a = alone.plan(state, ms.goal, traj)
        goals = pl.last_goals()
        assert np.array_equal(goals, alone.last_goals()) and np.array_equal(g["sfc"], a["sfc"]), j
        assert (g["status"] == 0).all(), (j, g["status"])
        _compare(g, ref.tick(state, goals, traj, j, pos, vel, sfc=g["sfc"]), ACTIVE_SET_TRAJ_ATOL, (goal_mode, j))
        differs = differs or np.abs(g["traj"] - a["traj"]).max() > 1e-3
        # (both contexts keep their corridor boxes in step: `alone` is fed the plans of the context with obstacles)
        traj = g["traj"]; state = next_state_host(traj); ref.stale[:] = traj
    assert differs, "the obstacles never moved a plan: the comparison would be vacuous"
    pl.close(); alone.close()


def test_no_obstacles_is_todays_context(L):
    """After set_obstacles([]) and on a context that never had any: ten ticks, the same bits, the same row capacity.  lsc_set_agents drops
    the obstacles; a tick without states is LSC_ESTATE."""
    from lsc_planner_amd.planner import next_state_host
    ms = hover_mission()
    never, had = L.SwarmPlanner(ms, _cfg(L, goal_mode="prior_based")), L.SwarmPlanner(ms, _cfg(L, goal_mode="prior_based"))
    cap = never.row_capacity()
    had.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH)
    assert had.row_capacity()[0] == 27 * 10 and cap[0] == 27 * 7
    state, traj = start_inputs(ms, never.SEGV)
    with pytest.raises(L.LscError, match="no states"):
        had.plan(state, ms.goal, traj)
    out = np.zeros((8, 3, 30), np.float32); cost = np.zeros(8); status = np.zeros(8, np.int32)
    fp, dp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    rc = had.L.lsc_replan_tick(had.ctx, state.ctypes.data_as(fp), ms.goal.ctypes.data_as(fp), traj.ctypes.data_as(fp), 1, out.ctypes.data_as(fp),
                               cost.ctypes.data_as(dp), status.ctypes.data_as(ip), None, None, None, None)
    assert rc == ESTATE
    had.planner_seq = 0
    had.set_obstacles([])
    assert had.row_capacity() == cap
    for j in range(1, 11):
        a, b = never.plan(state, ms.goal, traj, want_constraints=True), had.plan(state, ms.goal, traj, want_constraints=True)
        for k in ("traj", "cost", "status", "iters", "normal", "d"):
            assert np.array_equal(a[k], b[k]), (j, k)
        assert np.array_equal(never.last_goals(), had.last_goals()) and np.array_equal(never.row_counts(), had.row_counts())
        traj = a["traj"]; state = next_state_host(traj)
    # lsc_set_agents drops the obstacles
    had.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH)
    r, d, v, ac, vn = (np.ascontiguousarray(x, np.float64) for x in (ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity))
    assert had.L.lsc_set_agents(had.ctx, 8, *(x.ctypes.data_as(dp) for x in (r, d, v, ac, vn))) == 0
    had.K = 0
    assert had.row_capacity() == cap
    state, traj = start_inputs(ms, had.SEGV)
    had.planner_seq = 0
    assert (had.plan(state, ms.goal, traj)["status"] == 0).all()
    pos, vel = hover_states(1)
    with pytest.raises(L.LscError, match="no dynamic obstacles"):
        had.obstacle_states(pos, vel)
    never.close(); had.close()


def _refused(L, pl, call, *words):
    with pytest.raises(L.LscError) as e:
        call()
    msg = str(e.value)
    assert f"lsc error {EINVAL}:" in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def test_refusals_name_their_cause(L):
    """Everything that is not built for a context with dynamic obstacles returns LSC_EINVAL with the cause; the context plans on afterwards."""
    import torch
    from lsc_planner_amd.planner import tick_device_fused_batch, replan_tick_batch
    ms = hover_mission()
    rad, dw = HOVER_RADIUS, HOVER_DOWNWASH
    pos, vel = hover_states(1)
    # contexts that cannot take obstacles at all: refused at lsc_set_obstacles
    for kw, word in ((dict(planner_mode="bvc"), "bvc"), (dict(slack_mode="dynamical_limit", planner_mode="bvc"), "slack mode"),
                     (dict(reset_threshold=0.15), "reset_threshold"), (dict(world_dimension=2), "world_dimension 2")):
        p = L.SwarmPlanner(ms, _cfg(L, **kw))
        _refused(L, p, lambda: p.set_obstacles(rad, dw), "lsc_set_obstacles", word)
        p.close()
    big = L.circle_swap(300, circle_radius=40.0, world=(-45, -45, 0, 45, 45, 2.5))
    p = L.SwarmPlanner(big, _cfg(L))
    _refused(L, p, lambda: p.set_obstacles(rad, dw), "more agents than the GPU has CUs")
    p.close()
    pl = L.SwarmPlanner(ms, _cfg(L))
    state, traj = start_inputs(ms, pl.SEGV)
    _refused(L, pl, lambda: pl.set_obstacles(np.full(65, 0.2), np.ones(65)), "K = 65")
    _refused(L, pl, lambda: pl.set_obstacles([0.2, 0.0], [1, 1]), "radius of obstacle 1")
    _refused(L, pl, lambda: pl.set_obstacles([np.inf], [1]), "radius of obstacle 0")
    _refused(L, pl, lambda: pl.set_obstacles([np.nan], [1]), "radius of obstacle 0")
    pl.phase_profile(1)
    _refused(L, pl, lambda: pl.set_obstacles(rad, dw), "lsc_phase_profile")
    pl.phase_profile(0)
    pl.set_obstacles(rad, dw)
    bad = pos.copy(); bad[1, 2] = np.nan
    _refused(L, pl, lambda: pl.obstacle_states(bad, vel), "obstacle 1", "not finite")
    pl.obstacle_states(pos, vel)
    first = pl.plan(state, ms.goal, traj)
    assert (first["status"] == 0).all()
    # a shard that is not the whole swarm: known at the tick only
    pl.set_shard(0, 4)
    _refused(L, pl, lambda: pl.plan(state, ms.goal, traj), "shard is not the whole swarm")
    pl.set_shard(0, 8)
    pl.planner_seq = 1
    _refused(L, pl, lambda: pl.phase_profile(1), "lsc_phase_profile", "dynamic obstacles")
    _refused(L, pl, lambda: pl.dump_qp(0, "/dev/null"), "lsc_dump_qp", "dynamic obstacles")
    _refused(L, pl, lambda: pl.flight_begin([0.0, 0.1], 4), "lsc_flight_begin", "dynamic obstacles")
    dev = torch.device("cuda", 0)
    st2 = [torch.zeros((8, 9), device=dev), torch.zeros((8, 9), device=dev)]
    tr2 = [torch.zeros((8, 90), device=dev), torch.zeros((8, 90), device=dev)]
    goal = torch.from_numpy(ms.goal).to(dev)
    cost, status, iters = torch.zeros(8, dtype=torch.float64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    _refused(L, pl, lambda: pl.fly(st2, goal, tr2, 1, 2, cost, status, iters), "lsc_fly_device", "dynamic obstacles")
    other = L.SwarmPlanner(ms, _cfg(L))
    for order in ((pl, other), (other, pl)):
        with pytest.raises(L.LscError, match="dynamic obstacles") as e:
            tick_device_fused_batch(list(order), [st2[0]] * 2, [goal] * 2, [tr2[0]] * 2, [tr2[1]] * 2, [st2[1]] * 2, [cost] * 2, [status] * 2, [iters] * 2, [1, 1])
        assert f"lsc error {EINVAL}:" in str(e.value)
        with pytest.raises(L.LscError, match="dynamic obstacles") as e:
            replan_tick_batch(list(order), [state] * 2, [ms.goal] * 2, [traj] * 2, [1, 1])
        assert f"lsc error {EINVAL}:" in str(e.value)
    torch.cuda.synchronize()
    assert not status.any().item() and not tr2[1].any().item()          # nothing was enqueued by the refused ticks
    other.close()
    # the context remains usable: the same tick gives the same bits as before the refusals
    pl.planner_seq = 0
    again = pl.plan(state, ms.goal, traj)
    assert np.array_equal(again["traj"], first["traj"]) and np.array_equal(again["cost"], first["cost"])
    pl.close()


SIM = os.path.join(ROOT, "lsc_planner_amd", "lsc_sim")
HDR_A, HDR_O = "id,t,px,py,pz,vx,vy,vz,ax,ay,az,planning_time,qp_cost,planning_report,size", "obs_id,t,px,py,pz,size"


def _sim(tmp, name, doc, *args):
    out = tmp / name
    out.mkdir()
    mp = out / "m.json"
    mp.write_text(json.dumps(doc))
    r = subprocess.run([SIM, "--mission", str(mp), "--csv", str(out), "--quiet", "--max-iter", "120"] + list(args), capture_output=True, text=True, timeout=120)
    return r, out / "result_LSC_3agents.csv"


def test_simulator_flies_a_mission_with_obstacles(tmp_path):
    """Three agents, one straight and one spin obstacle: the mission completes, the CSV has the reference's header and columns, --replay
    reads it back with `obstacles 2`, and --no-obstacles writes the CSV of the same mission without its "obstacles" -- cell for cell as
    text, except planning_time, which is the wall clock of that run's ticks."""
    assert os.path.exists(SIM), "lsc_sim not built"
    r, f = _sim(tmp_path, "with", sim_mission_doc(), "--reset-threshold", "0")
    assert r.returncode == 0, r.stderr[-2000:]
    rows = list(csv.reader(open(f)))
    assert ",".join(rows[0]) == ",".join([HDR_A] * 3 + [HDR_O] * 2)
    assert all(len(row) == 57 for row in rows[1:]) and len(rows) > 20
    last = rows[-1]
    for q, a in enumerate(sim_mission_doc()["agents"]):                       # every agent arrived
        assert np.linalg.norm(np.array(last[15 * q + 2:15 * q + 5], float) - np.array(a["goal"])) < 0.2, (q, last[15 * q + 2:15 * q + 5])
    rp = subprocess.run([SIM, "--replay", str(f)], capture_output=True, text=True, timeout=60)
    assert rp.returncode == 0 and "agents 3 obstacles 2" in rp.stdout, rp.stdout + rp.stderr
    # the obstacles moved the flight, and --no-obstacles is the mission without them
    r0, f0 = _sim(tmp_path, "none", sim_mission_doc(), "--no-obstacles")
    r1, f1 = _sim(tmp_path, "bare", sim_mission_doc(None))
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr[-1000:] + r1.stderr[-1000:]
    agents_only = lambda rs: [[c for i, c in enumerate(row[:45]) if i % 15 != 11] for row in rs[1:]]      # (11: planning_time)
    a, b = list(csv.reader(open(f0))), list(csv.reader(open(f1)))
    assert a[0] == b[0] and len(a[0]) == 45 and agents_only(a) == agents_only(b)
    assert agents_only(rows) != agents_only(a), "the obstacles never moved the flight"


@pytest.mark.parametrize("args,word", [(["--reset-threshold", "0", "--device-loop", "5"], "lsc_flight_begin"),
                                       (["--reset-threshold", "0", "--planner", "bvc"], "bvc"),
                                       (["--reset-threshold", "0", "--planner", "bvc", "--slack", "collision_constraint"], "slack mode"),
                                       (["--reset-threshold", "0", "--dimension", "2"], "world_dimension 2"),
                                       (["--reset-threshold", "0", "--concurrent", "2"], "batch ticks"),
                                       ([], "reset_threshold")])
def test_simulator_refusals_exit_with_status_2(tmp_path, args, word):
    """What the library does not serve with obstacles ends lsc_sim with the library's reason and exit status 2."""
    r, _ = _sim(tmp_path, "r", sim_mission_doc(), *args)
    assert r.returncode == 2 and word in r.stderr and "dynamic obstacles" in r.stderr, (r.returncode, r.stderr[-1500:])
