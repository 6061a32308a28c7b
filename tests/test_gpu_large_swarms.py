"""Neighbour lists and the in-kernel cull of phase B above 13 107 agents (M = 5) / 16 384 agents (M = 4), up to 65 536: a unit
(obstacle * M + segment) then needs more than 16 bits (lsc_kernels.h NEIGH_MAX_UNITS).  Every case plans the bits of prune = 3, the
context without any cull -- which is what such swarms planned before, when both culls switched off above that size."""
import os

import numpy as np
import pytest

from harness import start_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    return L


class _Env:
    """Environment variables lsc_set_agents reads (capacities / cell size of the neighbour lists) for the planners created inside."""

    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _swarm(L, n, seed=20260929):
    """n agents at BASELINE configs[4]'s density: a 40 m x sqrt(n / 1024) square, 5 m high (bench.py --workload random1024 --agents n)."""
    half = 20.0 * (n / 1024.0) ** 0.5
    return L.random_swarm(n, world=(-half, -half, 0, half, half, 5), seed=seed)


_REFS = {}


def _reference(L, n, cfg, ticks, push=None, lib=None, seed=20260929):
    """Inputs and outputs of `ticks` closed-loop ticks of the prune = 3 context (no cull at all), computed once per module.  push =
    (tick, agent): that agent is moved 0.3 m off its plan in front of that tick (the disturbance checks of reset_threshold)."""
    key = (n, tuple(sorted(cfg.items())), ticks, push, lib is not None, seed)
    if key not in _REFS:
        from lsc_planner_amd.planner import next_state_host
        LL = lib or L
        ms = _swarm(L, n, seed)
        p = LL.SwarmPlanner(ms, LL.PlannerConfig(prune=3, **cfg))
        dt = cfg.get("dt", 0.2)
        state, traj = start_inputs(ms, p.SEGV)
        steps = []
        for tick in range(1, ticks + 1):
            if push and tick == push[0]:
                state[push[1], 0] += 0.3
            g = p.plan(state, ms.goal, traj)
            steps.append((state.copy(), traj.copy(), {k: g[k].copy() for k in ("traj", "cost", "status", "iters")}, p.row_counts().copy()))
            traj = g["traj"]
            state = next_state_host(traj, dt=dt) if "dt" in cfg else next_state_host(traj)
        p.close()
        _REFS[key] = (ms, steps)
    return _REFS[key]


def _replay(planner, ms, steps, sl=slice(None), check_rows=True):
    """Plans the reference's inputs tick after tick and asserts the reference's bits; returns the list lengths of every tick."""
    counts = []
    for tick, (state, traj, ref, rows) in enumerate(steps, 1):
        g = planner.plan(state, ms.goal, traj)
        for k in ("traj", "cost", "status", "iters"):
            assert np.array_equal(g[k], ref[k][sl]), (tick, k)
        if check_rows:
            assert np.array_equal(planner.row_counts()[sl], rows[sl]), tick
        counts.append(planner.neighbour_counts())
    return counts


def test_a_16384_agent_swarm_gets_neighbour_lists(L):
    """Above 13 107 agents the lists used to switch off without a word (their units no longer fit 16 bits): every agent walked all
    5 (N - 1) units again.  Now nearly every agent of a 16 384-agent swarm of configs[4]'s density has a list, a small fraction of them."""
    n = 16384
    ms = _swarm(L, n)
    p = L.SwarmPlanner(ms, L.PlannerConfig(prune=1))
    state, traj = start_inputs(ms, p.SEGV)
    p.plan(state, ms.goal, traj)
    u = p.neighbour_counts()
    p.close()
    assert u is not None
    assert (u >= 0).mean() > 0.999, (u < 0).sum()
    assert 0 < u[u >= 0].mean() < 5 * (n - 1) / 100, u[u >= 0].mean()


@pytest.mark.parametrize("n,cfg,ticks,push", [(16384, dict(), 4, None),
                                              (16384, dict(goal_mode="prior_based", reset_threshold=0.15), 5, (3, 7)),
                                              (20000, dict(), 3, None),
                                              (8192, dict(goal_mode="prior_based", reset_threshold=0.15), 4, None),
                                              (65536, dict(), 2, None)])
def test_lists_and_the_in_kernel_cull_plan_the_bits_of_prune3(L, n, cfg, ticks, push):
    """Lists (wide units: the low 16 bits + where each 65 536-unit block starts) and the in-kernel cull (LSC_NO_NEIGHBOUR_LISTS, now
    active at this size too) against prune = 3: trajectories, costs, statuses, iterations and row counts bit for bit, tick after tick.
    With reset_threshold an agent pushed off its plan switches the swarm to the slack-variable QPs in every context alike."""
    ms, steps = _reference(L, n, cfg, ticks, push)
    a = L.SwarmPlanner(ms, L.PlannerConfig(prune=1, **cfg))
    counts = _replay(a, ms, steps)
    a.close()
    for tick, u in enumerate(counts, 1):
        assert u is not None, tick
        if push and tick >= push[0]:
            continue                                    # (a disturbed swarm plans in lsc_general_kernel: no LSC units at all)
        assert (u >= 0).mean() > 0.999 and u[u >= 0].mean() < 5 * (n - 1) / 100, tick
    with _Env(LSC_NO_NEIGHBOUR_LISTS=1):
        b = L.SwarmPlanner(ms, L.PlannerConfig(prune=1, **cfg))
    assert b.neighbour_counts() is None
    _replay(b, ms, steps)
    b.close()


@pytest.mark.parametrize("env", [dict(LSC_NEIGH_LIST_CAP=40),                          # lists too short for the crowded agents: those cull by themselves
                                 dict(LSC_NEIGH_CELL=1000.0, LSC_NEIGH_OVF_CAP=16)])   # one bucket, its overflow list overflows: nobody gets a list
def test_overflow_paths_above_the_old_limit_plan_the_same_bits(L, env):
    """Agents without a list cull by themselves through the wide in-kernel list, with the same bits."""
    n = 16384
    ms, steps = _reference(L, n, {}, 3)
    with _Env(**env):
        a = L.SwarmPlanner(ms, L.PlannerConfig(prune=1))
    counts = _replay(a, ms, steps)
    a.close()
    u = counts[-1]
    if "LSC_NEIGH_OVF_CAP" in env:
        assert (u == -1).all()
    else:
        assert (u == -1).any() and (u >= 0).any() and u.max() <= 40


def test_a_shard_of_a_16384_agent_swarm(L):
    """A shard (lsc_set_shard) gets wide lists for its own agents -- the grid holds the whole swarm -- and plans what the whole swarm
    plans for those agents."""
    n = 16384
    ms, steps = _reference(L, n, {}, 4)
    a = L.SwarmPlanner(ms, L.PlannerConfig(prune=1))
    a.set_shard(9000, 2500)
    counts = _replay(a, ms, steps, sl=slice(9000, 11500), check_rows=False)
    a.close()
    assert all((u[9000:11500] >= 0).all() for u in counts)


def test_the_four_segment_build_above_its_own_limit(L):
    """The M = 4 library (units obstacle * 4 + segment) crosses 16 bits above 16 384 agents: lists against prune = 3 at 17 000."""
    import lsc_planner_amd as LL
    n, cfg = 17000, dict(dt=0.5, horizon=2.0)
    ms, steps = _reference(L, n, cfg, 3, lib=LL)
    a = LL.SwarmPlanner(ms, LL.PlannerConfig(prune=1, **cfg))
    assert a.M == 4
    counts = _replay(a, ms, steps)
    a.close()
    assert all(u is not None and (u >= 0).mean() > 0.999 for u in counts)
