"""-m gpu: a context that is re-used plans what a new context plans, and contexts that come and go leave no device memory behind.

lsc_set_agents and lsc_set_distmap replace a context's device buffers (lsc_abi.cpp groups them by lifetime: swarm, map).  The
tests drive the C ABI directly (SwarmPlanner calls lsc_set_agents only once, from its constructor) through every optional buffer
of both groups, bring the context back to a small swarm and compare its ticks with those of a fresh context, bit for bit."""
import ctypes
import time

import numpy as np
import pytest

from harness import start_inputs

pytestmark = pytest.mark.gpu

_fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))        # noqa: E731
_dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))       # noqa: E731
_ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))          # noqa: E731


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


def _set_agents(pl, ms):
    f64 = lambda a: np.ascontiguousarray(a, np.float64)                 # noqa: E731
    pl._check(pl.L.lsc_set_agents(pl.ctx, ms.qn, _dp(f64(ms.radius)), _dp(f64(ms.downwash)), _dp(f64(ms.max_vel)), _dp(f64(ms.max_acc)),
                                  _dp(f64(ms.nominal_velocity))))


def _fly(pl, ms, ticks, want_constraints=False):
    """`ticks` host-buffer ticks of mission `ms` from its start (planner_seq 1 ..), on host arrays of this test's own."""
    from lsc_planner_amd.planner import next_state_host
    N, M, SEGV = ms.qn, pl.M, pl.SEGV
    state, traj = start_inputs(ms, SEGV)
    goal = np.ascontiguousarray(ms.goal, np.float32)
    cost = np.zeros(N)
    res = []
    for seq in range(1, ticks + 1):
        out = np.zeros((N, 3, SEGV), np.float32)
        status, iters = np.zeros(N, np.int32), np.zeros(N, np.int32)
        nrm = np.zeros((N, N - 1, M, 3), np.float32) if want_constraints else None
        dd = np.zeros((N, N - 1, M, 6), np.float64) if want_constraints else None
        sfc = np.zeros((N, M, 6), np.float32) if pl.cfg.use_octomap else None
        pl._check(pl.L.lsc_replan_tick(pl.ctx, _fp(state), _fp(goal), _fp(traj), seq, _fp(out), _dp(cost), _ip(status), _ip(iters),
                                       _fp(nrm) if want_constraints else None, _dp(dd) if want_constraints else None,
                                       _fp(sfc) if sfc is not None else None))
        res.append({"traj": out, "cost": cost.copy(), "status": status, "iters": iters, "sfc": sfc})
        traj = out
        state = next_state_host(traj)
    return res


def _assert_same_ticks(reused, fresh):
    assert len(reused) == len(fresh)
    for tick, (a, b) in enumerate(zip(reused, fresh), 1):
        for key in ("traj", "cost", "status", "iters"):
            assert np.array_equal(a[key], b[key]), (tick, key)
        if b["sfc"] is not None:
            assert np.array_equal(a["sfc"], b["sfc"]), (tick, "sfc")


def _block_field(world, res, seed, density):
    """A synthetic 'distance field' as in test_gpu_goal.py: 0 inside random blocks of 3 x 3 x 3 cells, 1 m elsewhere."""
    rng = np.random.default_rng(seed)
    wmin, wmax = world[:3], world[3:]
    kmin = np.array([np.floor(wmin[k] / res) + 32768 for k in range(3)], np.int32)
    dims = [int(np.floor(wmax[k] / res) + 32768 - kmin[k] + 1) for k in range(3)]
    coarse = rng.random((dims[0] // 3 + 1, dims[1] // 3 + 1, dims[2] // 3 + 1)) < density
    dist = np.where(np.kron(coarse, np.ones((3, 3, 3), bool))[:dims[0], :dims[1], :dims[2]], 0.0, 1.0).astype(np.float32)
    return dist, kmin


def test_reused_context_plans_like_a_fresh_one_swarm_buffers(L):
    """Swarm group: 8 agents with the disturbance checks on (hand-over workspaces, persistent flags), 70 agents with one row per control
    point (generic LSC build, second pass with its HBM rows: capacity 27 < 27 x 69) and a tick with constraint dumps, 512 agents
    (neighbour-list allocation), back to the first 8."""
    world = (-20, -20, 0, 20, 20, 5)
    cfg = dict(reset_threshold=0.15, max_rows_per_cp=1, prune=True)
    small, mid, large = (L.random_swarm(n, world=world, seed=40 + n) for n in (8, 70, 512))
    pl = L.SwarmPlanner(small, L.PlannerConfig(**cfg))
    assert pl.row_capacity()[0] == 27
    _fly(pl, small, 1)
    _set_agents(pl, mid)
    assert "generic pass (more than 64 obstacles)" in pl.note()
    _fly(pl, mid, 1, want_constraints=True)
    _set_agents(pl, large)
    units = np.zeros(large.qn, np.int32)
    assert pl.L.lsc_neighbour_counts(pl.ctx, _ip(units), None) == 0          # (the context holds the lists' allocation)
    _fly(pl, large, 1)
    _set_agents(pl, small)
    reused = _fly(pl, small, 3)
    pl.close()
    ref = L.SwarmPlanner(small, L.PlannerConfig(**cfg))
    fresh = _fly(ref, small, 3)
    ref.close()
    _assert_same_ticks(reused, fresh)


def test_reused_context_plans_like_a_fresh_one_map_buffers(L):
    """Map group (goal planner on a distance field) and the swarm group's goal trace, goal profile and safety buffers: a small field,
    trace + profile + safety ratio, a second field in place of the first, then the first swarm and field again."""
    world = (-3, -3, 0, 3, 3, 1.5)
    res = 0.1
    dist1, kmin = _block_field(world, res, 5, 0.06)
    dist2, _ = _block_field(world, res, 6, 0.10)
    assert not np.array_equal(dist1, dist2)
    open_in_both = np.minimum(dist1, dist2)
    ms = L.random_swarm(8, world=world, seed=3, edt=open_in_both, edt_key_min=kmin, min_clearance=0.5)
    cfg = dict(use_octomap=True, goal_mode="prior_based", grid_margin=0.05)
    pl = L.SwarmPlanner(ms, L.PlannerConfig(**cfg))
    pl.set_distmap(dist1, kmin, res)
    pl.set_goal_trace(256)
    pl.goal_profile(1)
    _fly(pl, ms, 1)
    pl.goal_trace()
    pl.goal_profile(-1)
    pl.safety_ratio([0.0, 0.5, 1.0])
    pl.set_distmap(dist2, kmin, res)
    _fly(pl, ms, 1)
    pl.goal_profile(0)              # (neither switch is an allocation: lsc_set_agents leaves both as they are)
    pl.set_goal_trace(0)
    _set_agents(pl, ms)
    pl.set_distmap(dist1, kmin, res)
    reused = _fly(pl, ms, 3)
    goals = pl.last_goals()
    pl.close()
    ref = L.SwarmPlanner(ms, L.PlannerConfig(**cfg))
    ref.set_distmap(dist1, kmin, res)
    fresh = _fly(ref, ms, 3)
    assert np.array_equal(goals, ref.last_goals())
    ref.close()
    _assert_same_ticks(reused, fresh)


def test_contexts_that_come_and_go_leave_no_device_memory_behind(L):
    """Ten rounds of create, set_agents(64), set_distmap, tick, destroy: the device's free memory falls by no more than what ONE round
    holds while it is alive (free-before minus free-during of the first round; ten leaked rounds would be ten times that, the margin
    of one round absorbs the runtime's own caching)."""
    import torch
    world = (-6, -6, 0, 6, 6, 2.5)
    res = 0.1
    dist, kmin = _block_field(world, res, 9, 0.04)
    ms = L.random_swarm(64, world=world, seed=8, edt=dist, edt_key_min=kmin, min_clearance=0.5)
    free = lambda: torch.cuda.mem_get_info()[0]                          # noqa: E731
    quiet0 = free()
    time.sleep(1.0)
    quiet1 = free()
    before = quiet1
    one_round = None
    for rnd in range(10):
        pl = L.SwarmPlanner(ms, L.PlannerConfig(use_octomap=True, goal_mode="prior_based", grid_margin=0.05))
        pl.set_distmap(dist, kmin, res)
        _fly(pl, ms, 1)
        if rnd == 0:
            one_round = before - free()
        pl.close()
    after = free()
    print(f"free memory: {quiet0} / {quiet1} B a second apart; one round holds {one_round} B; after ten rounds {before - after} B less")
    assert one_round > 0
    if abs(quiet1 - quiet0) > one_round / 10:
        pytest.skip(f"the device's free memory moved by {abs(quiet1 - quiet0)} B within a second with nothing running here "
                    f"(one round holds {one_round} B): another process is using the card")
    assert before - after <= one_round, (before - after, one_round)
