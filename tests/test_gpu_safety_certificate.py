"""-m gpu: every way the library plans a tick, held to the continuous-time separation certificate (tests/safety_certificate.py).

The product's claim is that agents planned in the same tick collide at no instant of the horizon.  The parity tests hold it by transitivity
-- rows bit-equal to the oracle, QPs pinned to HiGHS --, so a rule misread alike in kernel and oracle passes them.  Here the claim is
certified from the plans alone, in float64, with no oracle in between: for every pair and segment the distance from the origin to the hull of
the index-matched control-point differences (z divided by the pair's downwash) is at least r_i + r_j, down to

    tolerances.separation_shortfall_bound = float32 storage of two control points at the world's extent + the reference's own shortfall.

Every case asserts the premise (starts apart), the path it ran, that nobody was excluded (an agent without a plan masks its pairs; only on
the forest may that happen, to at most 2 of 12), and that it is not vacuous: at least one tick with a pair within 1 mm of touching, as
tests/test_safety_certificate.py shows the oracle to have on the same mission.  Each prints its worst margin (-s).

Out of scope, with the reasons in tests/safety_certificate.py: slack modes, agents after a disturbance reset, dynamic obstacles, goal planning.
"""
import os

import numpy as np
import pytest

from harness import fly
from safety_certificate import pair_certificate, starts_apart, storage_bound
from test_safety_certificate import BATCH_CIRCLES, FOREST_TICKS, THROUGHPUT_TICKS, TIGHT, circle, forest_mission, mixed_at_density, mixed_swarm
from tolerances import separation_shortfall_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


class Certifier:
    """An each_tick hook of harness.fly (or see() by hand): certifies the first planner's plans of every tick."""

    def __init__(self, what, ms, M=5, planar=False, may_exclude=0, planner=0):
        self.what, self.ms, self.M, self.planar, self.may_exclude, self.planner = what, ms, M, planar, may_exclude, planner
        self.bound = separation_shortfall_bound(ms.world_min, ms.world_max, ms.downwash)
        self.worst, self.where, self.tight, self.ticks, self.excluded = np.inf, None, [], 0, 0
        assert starts_apart(ms.start, ms.radius, ms.downwash) >= 0.0            # the premise of the induction

    def see(self, tick, traj, status):
        c = pair_certificate(traj, self.ms.radius, self.ms.downwash, self.M, status=status, planar=self.planar)
        self.ticks += 1
        self.excluded += c.excluded_agents
        if c.worst < self.worst:
            self.worst, self.where = c.worst, (tick,) + c.where
        if c.worst < TIGHT:
            self.tight.append(tick)
        assert c.excluded_agents <= self.may_exclude, (self.what, tick, np.nonzero(status)[0], status[status != 0])
        assert c.worst >= -self.bound, (self.what, "tick", tick, "(i, j, segment)", c.where, "dist - (r_i + r_j)", c.worst, "bound", self.bound)
        return c

    def __call__(self, tick, state, traj, outs):
        g = outs[self.planner]
        self.see(tick, g["traj"], g["status"])

    def done(self, require_tight=True):
        print(f"{self.what}: worst dist - (r_i + r_j) {self.worst:+.3g} m at (tick, i, j, segment) {self.where}; bound {self.bound:.3g} m "
              f"(storage {storage_bound(self.ms.world_min, self.ms.world_max, self.ms.downwash):.3g}); {len(self.tight)} of {self.ticks} ticks "
              f"with a pair within 1 mm; excluded agent-ticks {self.excluded}")
        assert len(self.tight) >= 1 or not require_tight, (self.what, "no tick with a pair within 1 mm: the case proves nothing", self.worst)


# ------------------------------------------------------------------------------------------------ mixed agents, default solver
def test_mixed_agents_under_the_default_solver(L):
    """24 agents of radii 0.1 .. 0.2 and downwash 1 .. 2.5: the pair downwash and the split of the margin between unequal agents."""
    ms = mixed_swarm(24, 2.5)
    pl = L.SwarmPlanner(ms, L.PlannerConfig(solver="active_set"))
    pl.iterations_total(reset=True)
    cert = Certifier("mixed24 / active_set", ms)
    fly(pl, ms, 40, each_tick=cert)
    st = pl.solver_stats()
    assert st["solved"] + st["handed_over"] == 24 * 40 and st["solved"] > 0, st
    pl.close()
    cert.done()


# ------------------------------------------------------------------------------------------------ every solver path
def _ran_active_set(pl, n):
    st = pl.solver_stats()
    assert st["solved"] + st["handed_over"] == n and st["solved"] > 0.9 * n, st


def _ran_interior_point(pl, n):
    st = pl.solver_stats()
    assert st["solved"] == 0 and st["handed_over"] == 0 and pl.iterations_total() > n, (st, pl.iterations_total())


def _ran_hand_over(pl, n):
    st = pl.solver_stats()
    assert st["solved"] == 0 and st["handed_over"] == n and st["ip_iterations"] > 0, st


def _ran_second_pass(pl, n):
    assert pl.row_capacity()[0] == 27 and (pl.row_counts() == 27 * 7).all(), (pl.row_capacity(), pl.row_counts())    # every agent beyond the LDS pass


SOLVER_PATHS = {"active_set": (dict(solver="active_set"), _ran_active_set),
                "interior_point": (dict(solver="interior_point"), _ran_interior_point),
                "hand_over": (dict(solver="hand_over"), _ran_hand_over),                             # switched as tests/test_gpu_round5.py does
                "second_pass": (dict(solver="active_set", max_rows_per_cp=1, prune=False), _ran_second_pass)}     # as test_second_pass_with_rows_in_hbm


@pytest.mark.parametrize("path", list(SOLVER_PATHS))
def test_every_solver_path_on_the_tight_circle(L, path):
    """circle_swap(8, 1.2): neighbours touch from tick 5 to the end.  Under active_set the sampled accounting is held too: every ratio of
    lsc_safety_ratio is a distance at one instant, so it is no smaller than the certified ratio of that pair's segment."""
    cfg, ran = SOLVER_PATHS[path]
    ms = circle(8, 1.2)
    pl = L.SwarmPlanner(ms, L.PlannerConfig(**cfg))
    pl.iterations_total(reset=True)
    cert = Certifier(f"circle8_r1.2 / {path}", ms)
    times = np.linspace(0.0, 1.0, 21)
    residual = [0.0]

    def each(tick, state, traj, outs):
        c = cert.see(tick, outs[0]["traj"], outs[0]["status"])
        if path != "active_set":                                # (the interior point's stopping residual; the active-set solve writes none)
            residual[0] = max(residual[0], float(np.abs(pl.solver_residuals()[:, 1]).max()))
        if path == "second_pass":
            ran(pl, 8)
        if path == "active_set":
            ratio, partner, mn = pl.safety_ratio(times)
            _assert_sampled_ratios_above_certified(ms, c, ratio, times, 0.2, 5, (path, tick))
    fly(pl, ms, 60, each_tick=each)
    if path != "second_pass":
        ran(pl, 8 * 60)
    pl.close()
    print(f"largest primal residual (lsc_solver_residuals) {residual[0]:.3g}")
    cert.done()


def _assert_sampled_ratios_above_certified(ms, c, ratio, times, dt, M, where):
    """ratio [T][N]: min over partners of (downwash-scaled distance at times[t]) / (r_i + r_j), sampled in float32.  The sampled point of
    a pair lies in the hull of its segment's differences, so the ratio is at least min_j (certified distance / (r_i + r_j)) -- up to the
    sample's own float32 arithmetic: each position rounded to float32 (one more storage_bound on the difference), the difference taken
    and the squared norm summed in float32 (a difference, a product and two sums on the way of every term, each within 2^-24 relative:
    the squared norm within 8 x 2^-24 of itself, the norm within 4 x 2^-24)."""
    n = len(ms.radius)
    rsum = ms.radius[c.i] + ms.radius[c.j]
    cert = (c.margin.filled(np.inf) + rsum[:, None]) / rsum[:, None]               # [pairs][M]
    per_agent = np.full((n, M), np.inf)
    np.minimum.at(per_agent, c.i, cert)
    np.minimum.at(per_agent, c.j, cert)
    slack = storage_bound(ms.world_min, ms.world_max, ms.downwash) / rsum.min()
    for t, time in enumerate(times):
        m = min(int(time / dt + 1e-9), M - 1)
        low = per_agent[:, m] - slack - 4 * 2.0 ** -24 * ratio[t]
        assert (ratio[t] >= low).all(), (where, time, ratio[t], per_agent[:, m])


# ------------------------------------------------------------------------------------------------ BVC
BVC_MISSIONS = {"circle8_r2.0": (lambda: circle(8, 2.0), 50), "mixed24": (lambda: mixed_swarm(24, 2.5), 40)}


@pytest.mark.parametrize("name", list(BVC_MISSIONS))
def test_bvc(L, name):
    """mode/planner = bvc: the dense interior point of lsc_general.hpp plans every agent (lsc_general_info says how it was reached)."""
    make, ticks = BVC_MISSIONS[name]
    ms = make()
    pl = L.SwarmPlanner(ms, L.PlannerConfig(planner_mode="bvc"))
    cert = Certifier(f"{name} / bvc", ms)
    reached = set()

    def each(tick, state, traj, outs):
        cert.see(tick, outs[0]["traj"], outs[0]["status"])
        reached.add(pl.general_info()[1])
    fly(pl, ms, ticks, each_tick=each)
    pl.close()
    assert reached and reached <= {1, 2}, reached                # folded into the plan kernel or a launch of lsc_general_kernel, every tick
    # (the oracle's BVC flight of the mixed mission comes no closer than 1.3 mm, tests/test_safety_certificate.py: the circle is this mode's tight case)
    cert.done(require_tight=name != "mixed24")


# ------------------------------------------------------------------------------------------------ planar, M = 4
def test_planar_world(L):
    """world/dimension = 2: the 60-variable model; the hull is taken in x, y."""
    ms = circle(8, 1.2)
    pl = L.SwarmPlanner(ms, L.PlannerConfig(world_dimension=2, world_z_2d=1.0, solver="active_set"))
    cert = Certifier("circle8_r1.2 / planar", ms, planar=True)

    def each(tick, state, traj, outs):
        assert (outs[0]["traj"][:, 2, :] == np.float32(1.0)).all(), tick         # the planar model stores z = world/z_2d: it was the one that ran
        cert(tick, state, traj, outs)
    fly(pl, ms, 60, each_tick=each, planar_z=1.0)
    pl.close()
    cert.done()


def test_four_segment_library(L):
    """dt 0.5, horizon 2.0: liblsc_hip_m4.so, four segments of half a second."""
    ms = circle(8, 1.2)
    pl = L.SwarmPlanner(ms, L.PlannerConfig(dt=0.5, horizon=2.0))
    assert pl.M == 4 and pl.L.lsc_segments() == 4 and pl.SEGV == 24
    cert = Certifier("circle8_r1.2 / M = 4", ms, M=4)
    fly(pl, ms, 60, each_tick=cert)
    pl.close()
    cert.done()


# ------------------------------------------------------------------------------------------------ neighbour lists, in-kernel cull
class _Env:
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


def test_forced_neighbour_lists_and_the_in_kernel_cull(L):
    """512 mixed agents at the 24-agent density -- the smallest swarm for which a context builds neighbour lists (NEIGH_MIN_AGENTS) --, one
    context with the lists forced, one held to the in-kernel cull: an agent dropped from a list, or culled wrongly, carries no row against a
    neighbour and shows up as a pair that is not certified."""
    ms = mixed_at_density(512)
    with _Env(LSC_NEIGH_ALWAYS=1):
        lists = L.SwarmPlanner(ms, L.PlannerConfig(prune=1))
    with _Env(LSC_NO_NEIGHBOUR_LISTS=1):
        cull = L.SwarmPlanner(ms, L.PlannerConfig(prune=1))
    assert lists.neighbour_counts() is not None and cull.neighbour_counts() is None
    certs = [Certifier("mixed512 / neighbour lists", ms, planner=0), Certifier("mixed512 / in-kernel cull", ms, planner=1)]

    def each(tick, state, traj, outs):
        units = lists.neighbour_counts()
        assert (units >= 0).mean() > 0.5 and (units[units >= 0] < 5 * 511).all(), tick       # the agents had lists, and shorter ones than everybody
        for c in certs:
            c(tick, state, traj, outs)
    fly((lists, cull), ms, 6, each_tick=each)
    lists.close(); cull.close()
    for c in certs:
        c.done()


# ------------------------------------------------------------------------------------------------ throughput build
def test_throughput_build(L):
    """One agent more than the chip has CUs: the 256-lane build (lsc_plan{,_alt}_tp_kernel) plans the shard."""
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count + 1
    ms = mixed_at_density(n)
    pl = L.SwarmPlanner(ms)
    lds, thr = pl.row_capacity()
    assert 0 < thr < lds, (lds, thr)                    # default capacities and more agents than CUs: this shard takes the throughput build
    cert = Certifier(f"mixed{n} / throughput build", ms)
    fly(pl, ms, THROUGHPUT_TICKS, each_tick=cert)
    pl.close()
    cert.done()


# ------------------------------------------------------------------------------------------------ batch launch
def test_batched_launch(L):
    """Four 8-agent circles as the blocks of one launch per tick (lsc_replan_tick_batch: lsc_plan_batch_kernel)."""
    from lsc_planner_amd.planner import next_state_host
    from harness import start_inputs
    missions = [circle(8, r) for r in BATCH_CIRCLES]
    pls = [L.SwarmPlanner(ms) for ms in missions]
    certs = [Certifier(f"circle8_r{r} / batch", ms) for r, ms in zip(BATCH_CIRCLES, missions)]
    ins = [start_inputs(ms, 30) for ms in missions]
    for tick in range(1, 31):
        outs = L.replan_tick_batch(pls, [s for s, _ in ins], [ms.goal for ms in missions], [t for _, t in ins], [tick] * 4)
        for k, (traj, cost, status, iters) in enumerate(outs):
            certs[k].see(tick, traj, status)
        ins = [(next_state_host(o[0]), o[0]) for o in outs]
    for p in pls:
        p.close()
    for c in certs:
        c.done()


# ------------------------------------------------------------------------------------------------ device-resident ticks
def test_fused_device_ticks(L):
    """lsc_tick_device_fused on device buffers: the tables read back after every tick."""
    from test_gpu_flight import Dev
    ms = circle(8, 1.2)
    d = Dev(L, ms, L.PlannerConfig())
    cert = Certifier("circle8_r1.2 / tick_device_fused", ms)
    try:
        for tick in range(1, 31):
            d.tick()
            snap = d.snapshot()
            cert.see(tick, snap["traj"].reshape(8, 3, 30), snap["status"])
    finally:
        d.close()
    cert.done()


def test_flight_kernel_and_its_safety_log(L):
    """lsc_fly_device, K = 10 ticks per call: the last plans of every call are read back and certified, and the flight log's ratios of those
    ticks are held to the certificate (a sampled distance is no smaller than its segment's certified one)."""
    from test_gpu_flight import Dev
    ms = circle(8, 1.2)
    times = np.linspace(0.0, 1.0, 21)
    d = Dev(L, ms, L.PlannerConfig())
    cert = Certifier("circle8_r1.2 / fly (K = 10)", ms)
    try:
        d.pl.flight_begin(times, 30)
        seen = {}
        for call in range(3):
            d.fly(10)
            snap = d.snapshot()
            seen[d.seq] = cert.see(d.seq, snap["traj"].reshape(8, 3, 30), snap["status"])
        log = d.pl.flight_read(0, 30)
        assert [int(s) for s in log["summary"]["planner_seq"]] == list(range(1, 31))
        assert (log["status"] == 0).all()                                       # every tick of the flight, not only the ones read back
        for seq, c in seen.items():
            _assert_sampled_ratios_above_certified(ms, c, log["ratio"][seq - 1], times, 0.2, 5, ("flight log", seq))
            assert log["summary"]["min_ratio"][seq - 1] == log["ratio"][seq - 1].min()
        d.pl.flight_end()
    finally:
        d.close()
    cert.done()


# ------------------------------------------------------------------------------------------------ octomap world
def test_forest_world_pairs_and_corridors(L, tmp_path):
    """12 agents on the packaged forest: corridor rows beside LSC rows.  The pair certificate on the agents with a plan; every plan inside
    the GPU's own corridor boxes (the mask of test_oracle_sfc.py::test_tick_with_sfc_rows_on_forest: the first three control points are
    the initial state's); and those boxes' interior cells clear of the cells closer to an obstacle than the agent's radius + half a cell
    (the rule of test_box_growth_properties, on the kernel's boxes)."""
    from lsc_planner_amd.maps import forest_leaves, write_bt
    bt = str(tmp_path / "forest.bt")
    write_bt(bt, *forest_leaves())
    wmin, wmax = np.asarray((-5, -5, 0), np.float32), np.asarray((5, 5, 2.5), np.float32)
    dist, kmin, res = L.edt_from_bt(bt, wmin, wmax)
    ms = forest_mission(dist, kmin)
    pl = L.SwarmPlanner(ms, L.PlannerConfig(use_octomap=True))
    pl.set_distmap(dist, kmin, res)
    cert = Certifier("forest12 / octomap", ms, may_exclude=2)
    blocked = dist < 0.15 + 0.05 - 1e-5
    boxes = [0]

    def each(tick, state, traj, outs):
        g = outs[0]
        cert(tick, state, traj, outs)
        t = g["traj"].reshape(12, 3, 5, 6)
        for q in np.nonzero(g["status"] == 0)[0]:
            for m in range(5):
                lo, hi = g["sfc"][q, m, :3], g["sfc"][q, m, 3:]
                pts = t[q, :, m, :] if m > 0 else t[q, :, m, 3:]
                assert (pts >= lo[:, None] - 1e-5).all() and (pts <= hi[:, None] + 1e-5).all(), (tick, q, m)
                assert (lo >= wmin - 1e-6).all() and (hi <= wmax + 1e-6).all(), (tick, q, m)
                a = np.round(lo.astype(np.float64) / 0.1).astype(int) + 32768 - kmin
                b = np.round(hi.astype(np.float64) / 0.1).astype(int) + 32768 - kmin
                assert not blocked[a[0] + 1:b[0], a[1] + 1:b[1], a[2] + 1:b[2]].any(), (tick, q, m)
                boxes[0] += 1
    fly(pl, ms, FOREST_TICKS, each_tick=each)
    pl.close()
    assert boxes[0] >= 10 * 5 * FOREST_TICKS
    cert.done()
