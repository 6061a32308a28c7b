"""-m gpu: launch timing bound to the launches themselves (lsc_set_timing / lsc_kernel_times_ms).  A timed group's start event rides on
its first launch and its stop event on its last (hipExtLaunchKernel), so a sample is the span of the dispatches and nothing else enters
the queue.  Timing must change no result bit, every sample must be a positive time that fits inside the host's wall clock around the
ticks (a stop bound before its start, or a pair spanning several ticks, does not), and the sample counts must be those of the ticks."""
import os
import time

import numpy as np
import pytest

from test_gpu_octomap_batch import mission, suite  # noqa: F401  (the golden forest worlds and their loader)
from harness import assert_same_flights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    return L


class _Env:
    """Environment variables read at context creation / lsc_set_agents, for the planners created inside."""

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


class Run:
    """One mission flown device-resident (tick_device_fused) on the current stream."""

    def __init__(self, L, ms, cfg=None, bt=None):
        import torch
        self.torch = torch
        dev = torch.device("cuda", 0)
        self.pl = L.SwarmPlanner(ms, cfg) if cfg is not None else L.SwarmPlanner(ms)
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

    def outputs(self):
        """device copies of (traj, state, cost, status, iters) after a tick: stream-ordered, no synchronise"""
        return [t.clone() for t in (self.prev, self.states[0], self.cost, self.status, self.iters)]


def fly(runs, ticks, batch_L=None):
    """`ticks` ticks of every run (one launch each, or ONE batched launch per tick) between two synchronises ->
    (per tick per run the outputs, wall clock in ms between the synchronises)."""
    torch = runs[0].torch
    out = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        if batch_L is not None:
            for r in runs:
                r.seq += 1
            batch_L.tick_device_fused_batch([r.pl for r in runs], [r.states[0] for r in runs], [r.goal for r in runs],
                                            [r.prev for r in runs], [r.nxt for r in runs], [r.states[1] for r in runs],
                                            [r.cost for r in runs], [r.status for r in runs], [r.iters for r in runs],
                                            [r.seq for r in runs], runs[0].stream)
            for r in runs:
                r.flip()
        else:
            for r in runs:
                r.tick()
        out.append([r.outputs() for r in runs])
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


NAMES = ("traj", "state", "cost", "status", "iters")


def assert_samples(pl, which, n, wall_ms):
    """n samples, each > 0 and, like their sum, inside the wall clock; the average entry point agrees with them"""
    k = pl.kernel_times_ms(which)
    print(f"which {which}: samples (ms) {np.round(k, 5).tolist()} sum {k.sum():.5f} wall {wall_ms:.5f}")
    assert len(k) == n
    assert (k > 0).all(), k
    assert (k <= wall_ms).all() and k.sum() <= wall_ms, (k, wall_ms)
    avg, cnt = pl.kernel_time_ms(which)
    assert cnt == n and abs(avg - k.mean()) < 1e-9
    return k


def circle8(L, radius=3.0):
    return L.circle_swap(8, circle_radius=radius, z=1.0, world=(-5, -5, 0, 5, 5, 2.5))


def test_timed_ticks_plan_the_same_bits_and_fit_the_wall_clock(L):
    """8-agent circle swap, 6 fused ticks: one launch per tick carries both events."""
    timed, plain = Run(L, circle8(L)), Run(L, circle8(L))
    try:
        timed.pl.set_timing(True)
        a, wall = fly([timed], 6)
        b, _ = fly([plain], 6)
        assert_same_flights(a, b, NAMES, "timed vs untimed")
        assert_samples(timed.pl, 0, 6, wall)
        assert len(plain.pl.kernel_times_ms(0)) == 0
        timed.pl.set_timing(True)                    # again: the count restarts
        assert len(timed.pl.kernel_times_ms(0)) == 0 and timed.pl.kernel_time_ms(0) == (0.0, 0)
        _, wall = fly([timed], 2)
        assert_samples(timed.pl, 0, 2, wall)
    finally:
        timed.pl.close()
        plain.pl.close()


def test_start_and_stop_on_different_launches(L, monkeypatch):
    """reset_threshold 0.15 with the hand-over launch kept (LSC_GENERAL_HANDOVER): the pair spans the plan kernel and lsc_general_kernel."""
    cfg = lambda: L.PlannerConfig(reset_threshold=0.15)
    monkeypatch.setenv("LSC_GENERAL_HANDOVER", "1")
    timed, plain = Run(L, circle8(L), cfg()), Run(L, circle8(L), cfg())
    monkeypatch.delenv("LSC_GENERAL_HANDOVER", raising=False)
    folded = Run(L, circle8(L), cfg())
    try:
        timed.pl.set_timing(True)
        a, wall = fly([timed], 6)
        b, _ = fly([plain], 6)
        c, _ = fly([folded], 6)
        assert_same_flights(a, b, NAMES, "timed vs untimed, hand-over launch")
        assert_same_flights(a, c, NAMES, "hand-over launch vs folded")
        assert_samples(timed.pl, 0, 6, wall)
        timed.pl.set_timing(True)
        assert len(timed.pl.kernel_times_ms(0)) == 0
    finally:
        for r in (timed, plain, folded):
            r.pl.close()


def test_start_on_the_neighbour_build_stop_on_the_last_launch(L):
    """512 agents with the neighbour lists forced: build, query and the plan launches in one pair."""
    from lsc_planner_amd.planner import PlannerConfig
    ms = L.random_swarm(512, world=(-14, -14, 0, 14, 14, 5), seed=20260930, min_sep=0.5)
    with _Env(LSC_NEIGH_ALWAYS=1):
        timed, plain = Run(L, ms, PlannerConfig()), Run(L, ms, PlannerConfig())
    try:
        timed.pl.set_timing(True)
        a, wall = fly([timed], 2)
        b, _ = fly([plain], 2)
        assert_same_flights(a, b, NAMES, "timed vs untimed, neighbour lists")
        assert_samples(timed.pl, 0, 2, wall)
        lists = timed.pl.neighbour_counts()
        assert lists is not None and (lists >= 0).any(), "the lists are meant to be in use"
    finally:
        timed.pl.close()
        plain.pl.close()


def test_goal_corridor_and_plan_groups_on_a_corridor_world(L, suite):  # noqa: F811
    """Six agents in a forest world, 3 ticks: goal search (which = 3), corridor update (4) and plan kernel (0), one launch each."""
    ms, bt = mission(L, suite, "forest", 11, 6)
    r = Run(L, ms, L.PlannerConfig(use_octomap=True, goal_mode="prior_based"), bt)
    try:
        r.pl.set_timing(True)
        _, wall = fly([r], 3)
        total = sum(assert_samples(r.pl, w, 3, wall).sum() for w in (3, 4, 0))
        assert total <= wall, (total, wall)
    finally:
        r.pl.close()


def test_batch_launch_timed_on_the_first_context(L):
    """Two 8-agent swarms in one launch per tick, 4 ticks: samples on context 0 only, plans those of each swarm ticking alone."""
    mk = lambda: [Run(L, circle8(L, 3.0)), Run(L, circle8(L, 2.6))]
    bat, solo = mk(), mk()
    try:
        bat[0].pl.set_timing(True)
        a, wall = fly(bat, 4, batch_L=L)
        b, _ = fly(solo, 4)
        assert_same_flights(a, b, NAMES, "batched and timed vs alone and untimed")
        assert_samples(bat[0].pl, 0, 4, wall)
        assert len(bat[1].pl.kernel_times_ms(0)) == 0
    finally:
        for r in bat + solo:
            r.pl.close()
