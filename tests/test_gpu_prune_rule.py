"""-m gpu: every copy of the row-pruning rule (csrc/lsc_kernels.hip `unit_rows` in each plan_agent instantiation, csrc/lsc_general.hpp),
held by COUNT: after a tick, row_counts() and bucket_max() of every agent against tests/prune_reference.kept_rows evaluated on the
reference's rows of the same tick.  Optimum comparisons cannot see a wrong box (tests/test_prune_soundness.py, which also proves the
rule itself by LP and shows that the counts of these scenes move under every wrong rule tried); the plans are still compared with the
oracle (harness.assert_tick_matches) -- on every tick of the closed loops, on every third to eighth scene of the sweeps, whose counts
are checked at every scene: an oracle tick of two agents takes 3 to 90 ms.

A row within 1e-9 of the threshold is borderline -- the kernel's scan adds in another order, the compiler may contract multiply-adds --:
the count must lie in [rows kept for sure, those + the borderline ones].  Every test asserts that borderline rows are at most 1 % of
its candidate rows, so no kernel hides behind the band.

The scenes (tests/prune_scenes.py): agent 0 flies along +-x, +-y, +-z or a diagonal towards a partner hovering at D = 0.45 .. 3 m in steps
of 0.02 m, one context per path -- only state and goal change between scenes, each planned as tick 1.  The general kernel reports its
collision rows plus one sign row per (slack obstacle, segment with a kept row): prune_reference.general_count; it writes no bucket_max.
"""
import numpy as np
import pytest

import prune_scenes as PS
from harness import assert_tick_matches
from obstacle_reference import ObstacleSwarm
from prune_reference import BAND, count_band, general_count
from tolerances import (ACTIVE_SET_TRAJ_ATOL, COST_ATOL, FUZZ_PLAN_COMPARED_BELOW_COST, FUZZ_TRAJ_ATOL, INTERIOR_POINT_TRAJ_ATOL,
                        TRAJ_ATOL)

pytestmark = pytest.mark.gpu
Z2D = 0.9


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


class Band:
    """Counts of one test against the reference, and the share of borderline rows among the candidates."""

    def __init__(self):
        self.edge = self.cand = self.agent_ticks = self.kept = 0

    def check(self, pl, kept, where, prune=1, slack=None, buckets=True):
        rc, bm = pl.row_counts(), pl.bucket_max()
        for q, (keep, gap, _) in kept.items():
            lo, hi, blo, bhi = count_band(keep, gap, prune)
            if slack is not None:                       # the general kernel: + its group sign rows
                edge = (np.abs(gap) <= BAND) if prune else np.zeros_like(keep)
                lo, hi = general_count(keep & ~edge, slack[q]), general_count(keep | edge, slack[q])
            assert lo <= rc[q] <= hi, (where, "agent", q, "rows", int(rc[q]), "reference", lo, hi)
            if buckets and slack is None:
                assert blo <= bm[q] <= bhi, (where, "agent", q, "fullest bucket", int(bm[q]), "reference", blo, bhi)
            if prune:
                self.edge += int((np.abs(gap) <= BAND).sum())
            self.cand += int(np.isfinite(gap).sum())
            self.kept += lo
            self.agent_ticks += 1

    def close(self):
        assert self.cand > 0 and self.edge <= 0.01 * self.cand, (self.edge, self.cand)


def _cost_floor(O, ms, dt, hovering):
    """Absolute floor of the cost comparison per agent: COST_ATOL, and for the agents in `hovering` (fillers at rest at their goals 25 m
    and more from the origin, whose optimum is exactly 0) what the cancellation in (1/2) x'Px + c'x + cst leaves of it at their
    coordinates p: 2^-52 p^2 (w_c sum |Q| over 3 axes and M segments + w_t) -- 3e-6 at 25 m (measured there: kernel 1.8e-7, oracle 1.5e-7)."""
    atol = np.full(ms.qn, COST_ATOL)
    p = np.abs(ms.start).max(axis=1).astype(np.float64)
    floor = 2.0 ** -52 * p * p * (0.01 * np.abs(O.qbase(dt)).sum() * 3 * O.M + 1.0)          # (PlannerConfig's weights: 0.01 and 1)
    atol[hovering] = np.maximum(COST_ATOL, floor[hovering])
    return atol


def _plan_twice(pl, state, goal, prev, seq):
    """The same tick with the dense dumps and without (the dumps switch the in-kernel cull and the general kernel's pruning off)."""
    pl.planner_seq = seq - 1
    dumped = pl.plan(state, goal, prev, want_constraints=True)
    pl.planner_seq = seq - 1
    return dumped, pl.plan(state, goal, prev)


def _sweep(L, O, *, n=2, companions=0, sweeps=PS.SWEEPS, every=1, cfg=None, planar=False, m4=False, oracle_every=1, traj_atol=ACTIVE_SET_TRAJ_ATOL,
           note=None, radius=PS.RADIUS, scenes=None, band=None, near=None, throughput=False):
    """One context, the sweep's scenes as tick 1 each, counts at every scene.  Rows: tests/prune_scenes.PairRows (oracle.lsc_pair, no QP
    solve).  Every oracle_every-th scene the oracle flies the tick too (3 .. 90 ms for two agents): its rows must be PairRows' and the
    kernel's dumps, its plans the kernel's.  near: after the first scene only these agents are counted (the others' inputs stand still)."""
    M, dt = (4, 0.5) if m4 else (5, 0.2)
    cfg = dict(cfg or {})
    prune = int(cfg.get("prune", 1))
    if m4:
        cfg.update(dt=dt, horizon=M * dt)
    kw = dict(world_dimension=2, world_z_2d=Z2D) if planar else {}
    band = band or Band()
    with O.segments(M):
        ms = PS.mission(n, companions=companions, planar_z=Z2D if planar else None, radius=radius)
        pl = L.SwarmPlanner(ms, L.PlannerConfig(solver="active_set", **cfg, **kw))
        assert pl.M == M and (note is None or note in pl.note()), pl.note()
        if throughput:
            lds, thr = pl.row_capacity()
            assert 0 < thr < lds, (lds, thr)                # default capacities: this shard takes the throughput build
        prm = O.make_params(dt=dt, world_min=ms.world_min, world_max=ms.world_max, obs_f32=True, **kw)
        sw = O.Swarm(prm, ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
        pairs = PS.PairRows(O, ms.radius, ms.downwash)
        prev = np.zeros((n, 3, O.SEGV), np.float32)
        if planar:
            prev[:, 2, :] = np.float32(Z2D)
        stale = prev.copy()
        cost_atol = _cost_floor(O, ms, dt, np.arange(n) >= 2 + companions)
        if scenes is None:
            scenes = PS.sweep_scenes(n, sweeps, every, companions, Z2D if planar else None)
        for k, (name, D, state, goal) in enumerate(scenes):
            where = (name, D)
            pred = PS.predictions(O, state, prev, 1, dt)
            with_oracle = k % oracle_every == 0
            if with_oracle:
                sw.stale[:] = stale
                o = sw.tick(state, goal, prev, 1, want_lsc=True, nthreads=1 if n <= 4 else 8)
                dumped, g = _plan_twice(pl, state, goal, prev, 1)
                assert_tick_matches(dumped, o, where, cost_atol=cost_atol[o["status"] == 0], traj_atol=traj_atol)
                assert_tick_matches(g, o, where, rows=False, cost_atol=cost_atol[o["status"] == 0], traj_atol=traj_atol)
            else:
                pl.planner_seq = 0
                g = pl.plan(state, goal, prev)
            agents = None if with_oracle and (k == 0 or near is None) else near
            normal, d = pairs.rows(pred, agents)
            if with_oracle:
                sel = slice(None) if agents is None else list(agents)
                assert np.array_equal(normal[sel], o["normal"][sel]) and np.array_equal(d[sel], o["d"][sel]), where
            kept = PS.kept_of_tick(state, pred, normal, d, ms.max_vel, ms.max_acc, dt, agents=agents, planar=planar, z2d=Z2D, prune=prune)
            band.check(pl, kept, where, prune)
            stale = np.where((g["status"] == 0)[:, None, None], g["traj"], stale).astype(np.float32)
        pl.close()
    return band


# ------------------------------------------------------------------------------------------------- the plan kernels
def test_small_swarm_build_pair(L, oracle):
    """N = 2: the one-wave-per-segment build, all seven sweeps (903 scenes), and the threshold scenes -- one context per radius -- whose
    chosen row lies 1e-8 on the kept side: ten times the band, a third of what a flipped pad moves."""
    band = _sweep(L, oracle, oracle_every=3, note="one wave per segment")
    assert band.agent_ticks == 2 * 7 * len(PS.DISTANCES) and band.kept > 0
    n_thr = 0
    for name, u, frac in PS.SWEEPS:
        for D in PS.THRESHOLD_DISTANCES:
            t = PS.threshold_scene(oracle, u, frac, D)
            if t is not None:
                radius, state, goal, row = t
                _sweep(L, oracle, radius=radius, scenes=[(name + " threshold", D, state, goal)], band=band)
                n_thr += 1
    assert n_thr >= 10, n_thr
    band.close()


def test_small_swarm_build_nine_agents(L, oracle):
    """N = 9: the pair, two companions beside the partner (up to three rows per control point) and five fillers; the z sweeps and the
    diagonal."""
    _sweep(L, oracle, n=9, companions=2, sweeps=PS.SWEEPS[4:], oracle_every=8, note="one wave per segment").close()


def test_generic_pass(L, oracle):
    """N = 66 (65 obstacles: the generic pass; 325 units, below the in-kernel cull's threshold): the pair plus fillers 25 m apart that
    contribute no row.  The oracle flies every eighth scene; the rows in between are lsc_pair's, checked against the oracle's on its scenes."""
    band = _sweep(L, oracle, n=66, sweeps=[PS.SWEEPS[6]], oracle_every=8, near=range(10),
                 note="generic pass (more than 64 obstacles)")
    assert band.kept > 0
    band.close()


def test_throughput_build(L, oracle):
    """N = 257 (more agents than the chip has CUs: the 256-lane throughput build, its in-kernel cull over 1280 units), the same fillers."""
    band = _sweep(L, oracle, n=257, sweeps=[PS.SWEEPS[6]], oracle_every=64, near=range(10), throughput=True)
    assert band.kept > 0
    band.close()


def test_second_pass_with_rows_in_hbm(L, oracle):
    """max_rows_per_cp = 1: 27 rows fit the LDS pass; with two companions beside the partner agent 0 carries up to 81 and is planned by
    the second pass (interior point, rows in HBM), which writes the count again."""
    n = 4
    ms = PS.mission(n, companions=2)
    pl = L.SwarmPlanner(ms, L.PlannerConfig(solver="active_set", max_rows_per_cp=1))
    cap = int(pl.row_capacity()[0])
    pl.close()
    assert cap == 27
    over = [0]

    class Counting(Band):
        def check(self, pl, kept, where, prune=1, **kw):
            over[0] += sum(count_band(keep, gap)[0] > cap for keep, gap, _ in kept.values())
            super().check(pl, kept, where, prune, **kw)

    band = _sweep(L, oracle, n=n, companions=2, sweeps=[PS.SWEEPS[6], PS.SWEEPS[0], PS.SWEEPS[5]], cfg=dict(max_rows_per_cp=1), oracle_every=4,
                  traj_atol=INTERIOR_POINT_TRAJ_ATOL, band=Counting())
    assert over[0] >= 20, over[0]                     # (by the reference's count: agent-ticks that did not fit the first pass)
    band.close()


def test_planar_world(L, oracle):
    """world_dimension = 2: the rows have no z term, z rests at z_2d; the in-plane sweeps."""
    _sweep(L, oracle, planar=True, sweeps=PS.PLANAR_SWEEPS, oracle_every=4).close()


def test_four_segment_library(L, oracle):
    """liblsc_hip_m4.so (dt = 0.5, horizon 2): K = 5 m + i - 2 up to 18, V and A of half-second segments."""
    _sweep(L, oracle, m4=True, oracle_every=4, traj_atol=INTERIOR_POINT_TRAJ_ATOL).close()


@pytest.mark.parametrize("prune", [0, 2, 3])
def test_prune_modes(L, oracle, prune):
    """prune = 0 keeps all 27 rows per obstacle, 2 applies the velocity-only formula, 3 the exact rule without the cull (1 is every
    other test of this file); N = 4 with two companions, three sweeps."""
    band = _sweep(L, oracle, n=4, companions=2, sweeps=[PS.SWEEPS[6], PS.SWEEPS[1], PS.SWEEPS[4]], cfg=dict(prune=prune), oracle_every=4)
    assert band.kept > 0 and (prune != 0 or band.kept == 27 * 3 * band.agent_ticks)
    band.close()


# ------------------------------------------------------------------------------------------------- dynamic obstacles
@pytest.mark.parametrize("n,k", [(1, 1), (2, 64)])
def test_dynamic_obstacles(L, oracle, n, k):
    """The OBS instantiations: the partner is a dynamic obstacle drifting at 0.05 m/s (predicted at constant velocity), K = 1 against a
    lone agent (one wave per segment) and K = 64 of which 63 stand at least 20 m away, with a far second agent (65 obstacles: the generic
    pass).  Reference tick and predicted points: tests/obstacle_reference.py."""
    O, dt = oracle, 0.2
    full = PS.mission(3)                                    # agent 0, the partner, one filler
    pick = [0, 2][:n]
    ms = L.Mission(full.start[pick].copy(), full.goal[pick].copy(), np.array([-130, -130, 0], np.float32), np.array([130, 130, 5.2], np.float32),
                   full.radius[pick].copy(), full.downwash[pick].copy(), full.max_vel[pick].copy(), full.max_acc[pick].copy(), full.nominal_velocity[pick].copy())
    rad, dw = np.full(k, 0.12), np.full(k, 1.5)
    far = PS.filler_positions(k + 7, PS.CENTRE[2])[8:]       # (the first ring holds the agents' filler)
    vel = np.zeros((k, 3), np.float32)
    vel[0] = (0.0, 0.05, 0.0)
    pl = L.SwarmPlanner(ms, L.PlannerConfig(solver="active_set"))
    pl.set_obstacles(rad, dw)
    ref = ObstacleSwarm(O, ms, rad, dw)
    prev = np.zeros((n, 3, O.SEGV), np.float32)
    band = Band()
    cost_atol = _cost_floor(O, ms, dt, np.arange(n) >= 1)
    for name, D, state3, goal3 in PS.sweep_scenes(3, [PS.SWEEPS[6], PS.SWEEPS[5]] if k == 1 else [PS.SWEEPS[6]]):
        state, goal = state3[pick], goal3[pick]
        pos = np.concatenate([state3[1:2, :3], far[:k - 1]]).astype(np.float32)
        pl.obstacle_states(pos, vel)
        r = ref.tick(state, goal, prev, 1, pos, vel)
        dumped, g = _plan_twice(pl, state, goal, prev, 1)
        assert_tick_matches(dumped, r, (name, D), rows="bits", cost_atol=cost_atol[r["status"] == 0], traj_atol=ACTIVE_SET_TRAJ_ATOL)
        assert_tick_matches(g, r, (name, D), rows=False, cost_atol=cost_atol[r["status"] == 0], traj_atol=ACTIVE_SET_TRAJ_ATOL)
        opts = PS.points_of(np.stack([O.const_vel_traj(pos[j], vel[j], dt) for j in range(k)]))
        kept = PS.kept_of_tick(state, PS.predictions(O, state, prev, 1, dt), r["normal"], r["d"], ms.max_vel, ms.max_acc, dt, obstacle_points=opts)
        band.check(pl, kept, (name, D))
    pl.close()
    assert band.kept > 0
    band.close()


# ------------------------------------------------------------------------------------------------- the general kernel's copy
def _rest(state, segv):
    """[N][3][SEGV]: every agent predicted at its current position (BVC, or after a disturbance reset)."""
    return np.repeat(np.asarray(state, np.float32)[:, :3, None], segv, axis=2)


@pytest.mark.parametrize("slack", ["none", "dynamical_limit"])
def test_general_kernel_bvc(L, oracle, slack):
    """lsc_general_kernel in BVC mode, tick 1 of three sweeps with a companion.  n_constraint_segments = 2: rows of segments 0 and 1 only
    (9 candidates per obstacle), pruned by the kernel's serial copy of the rule.  slack_mode = dynamical_limit: the velocity and
    acceleration rows are soft, the rule must be OFF -- every one of the 27 rows per obstacle is counted.  No obstacle carries collision
    slack in either, so no group sign row is counted."""
    O, n, dt = oracle, 3, 0.2
    ncs = 2 if slack == "none" else -1
    ms = PS.mission(n, companions=1)
    pl = L.SwarmPlanner(ms, L.PlannerConfig(planner_mode="bvc", slack_mode=slack, n_constraint_segments=ncs))
    prm = O.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True)
    sw = O.SwarmEx(prm, O.make_modes(planner="bvc", slack=slack, n_constraint_segments=ncs), ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
    prev = np.zeros((n, 3, O.SEGV), np.float32)
    stale = prev.copy()
    band = Band()
    no_slack = np.zeros((n, n - 1), bool)
    rule = 0 if slack == "dynamical_limit" else 1
    r32, dw32 = ms.radius.astype(np.float32).astype(np.float64), ms.downwash.astype(np.float32).astype(np.float64)
    normal, d = np.zeros((n, n - 1, O.M, 3), np.float32), np.zeros((n, n - 1, O.M, O.NC))
    for k, (name, D, state, goal) in enumerate(PS.sweep_scenes(n, [PS.SWEEPS[6], PS.SWEEPS[0], PS.SWEEPS[5]], 1, 1)):
        rest = _rest(state, O.SEGV)
        for qi in range(n):
            for oi, qj in enumerate(q for q in range(n) if q != qi):
                normal[qi, oi], d[qi, oi] = O.bvc_pair(rest[qi], rest[qj], ms.radius[qi], r32[qj], ms.downwash[qi], dw32[qj])
        if k % 4 == 0:                                   # the oracle flies every fourth scene: its rows are bvc_pair's and the kernel's dumps
            sw.disturbance_update(state, prev, 1)
            sw.stale[:] = stale
            o = sw.tick(state, goal, prev, 1, want_lsc=True)
            assert np.array_equal(normal, o["normal"]) and np.array_equal(d, o["d"]), (name, D)
            dumped, g = _plan_twice(pl, state, goal, prev, 1)
            # (as tests/test_gpu_fuzz.py: with the 1e5 penalty on a violated limit plans are compared below FUZZ_PLAN_COMPARED_BELOW_COST only)
            tame = (o["status"] != 0) | (np.abs(o["cost"]) < FUZZ_PLAN_COMPARED_BELOW_COST)
            assert_tick_matches(dumped, o, (name, D), cost_atol=COST_ATOL, traj_atol=FUZZ_TRAJ_ATOL if rule == 0 else TRAJ_ATOL, traj_mask=tame)
            assert_tick_matches(g, o, (name, D), rows=False, cost_atol=COST_ATOL, traj_atol=FUZZ_TRAJ_ATOL if rule == 0 else TRAJ_ATOL, traj_mask=tame)
        else:
            pl.planner_seq = 0
            g = pl.plan(state, goal, prev)
        kept = PS.kept_of_tick(state, rest, normal, d, ms.max_vel, ms.max_acc, dt, prune=rule, ncs=ncs)
        band.check(pl, kept, (name, D), prune=rule, slack=no_slack)
        if slack == "dynamical_limit":
            assert (pl.row_counts() == 27 * (n - 1)).all(), (name, D, pl.row_counts())
        stale = np.where((g["status"] == 0)[:, None, None], g["traj"], stale).astype(np.float32)
    pl.close()
    assert band.kept > 0
    band.close()


def test_general_kernel_after_a_gust(L, oracle):
    """reset_threshold = 0.15, LSC mode: the pair with a companion flies closed loops from eleven distances along three directions; before
    tick 3 a gust moves the partner 0.3 m off its plan, and from then on the whole swarm is planned by lsc_general_kernel: the disturbed
    agent is predicted at rest that tick, and every obstacle in the persistent slack set (the oracle's slack_set) adds one sign row per
    segment with a kept row."""
    from lsc_planner_amd.planner import next_state_host
    O, n, dt = oracle, 3, 0.2
    ms = PS.mission(n, companions=1)
    band, general_ticks = Band(), 0
    for name, u, frac in (PS.SWEEPS[6], PS.SWEEPS[0], PS.SWEEPS[5]):
        for D in PS.DISTANCES[10::11]:
            state, goal = PS.scene(n, u, frac, float(D), companions=1)
            pl = L.SwarmPlanner(ms, L.PlannerConfig(reset_threshold=0.15))
            prm = O.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True)
            sw = O.SwarmEx(prm, O.make_modes(reset_threshold=0.15), ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
            prev = np.zeros((n, 3, O.SEGV), np.float32)
            stale = prev.copy()
            for tick in range(1, 6):
                if tick == 3:
                    state[1, :3] += np.float32([0.1, 0.25, -0.12])
                own = sw.disturbance_update(state, prev, tick)
                sw.stale[:] = stale
                o = sw.tick(state, goal, prev, tick, want_lsc=True)
                dumped, g = _plan_twice(pl, state, goal, prev, tick)
                assert_tick_matches(dumped, o, (name, D, tick), cost_atol=COST_ATOL)
                assert_tick_matches(g, o, (name, D, tick), rows=False, cost_atol=COST_ATOL)
                pred = PS.predictions(O, state, prev, tick, dt)
                general = bool(sw.slack_set.any())
                if general:
                    pred = np.where(own.astype(bool)[:, None, None], _rest(state, O.SEGV), pred)
                    slack = np.array([np.delete(sw.slack_set[q], q) for q in range(n)], bool)
                    general_ticks += 1
                assert general or tick < 3, (name, D, tick)
                kept = PS.kept_of_tick(state, pred, o["normal"], o["d"], ms.max_vel, ms.max_acc, dt)
                band.check(pl, kept, (name, D, tick), slack=slack if general else None)
                ok = o["status"] == 0
                stale = np.where(ok[:, None, None], g["traj"], stale).astype(np.float32)
                prev = g["traj"]
                state = next_state_host(prev)
            pl.close()
    assert general_ticks >= 3 * 3 * len(PS.DISTANCES[10::11]) and band.kept > 0
    band.close()


# ------------------------------------------------------------------------------------------------- closed loop
def test_closed_loops_of_small_swarms(L, oracle):
    """The fuzz generator's swarms of 2 .. 8 agents (extreme radii, downwash, limits; coincident agents; moving first ticks), six ticks
    on the kernel's own plans: counts every tick.  From tick 2 on d0 comes from a float32 state with a non-zero acceleration and the
    predictions are shifted plans."""
    from lsc_planner_amd.planner import next_state_host
    O, dt = oracle, 0.2
    band = Band()
    for seed in range(300, 324):
        f = PS.fuzz_swarm(seed)
        ms = PS.fuzz_mission(f)
        n = ms.qn
        pl = L.SwarmPlanner(ms, L.PlannerConfig(solver="active_set"))
        sw = O.Swarm(O.make_params(world_min=f["wmin"], world_max=f["wmax"], obs_f32=True), f["radius"], f["dw"], f["vmax"], f["amax"], f["vnom"])
        state = np.zeros((n, 9), np.float32)
        state[:, :3], state[:, 3:6] = f["start"], f["vel0"]
        prev = np.zeros((n, 3, O.SEGV), np.float32)
        stale = prev.copy()
        for tick in range(1, 7):
            sw.stale[:] = stale
            o = sw.tick(state, f["goal"], prev, tick, want_lsc=True, nthreads=8)
            dumped, g = _plan_twice(pl, state, f["goal"], prev, tick)
            ok = o["status"] == 0
            tame = ~ok | (np.abs(o["cost"]) < FUZZ_PLAN_COMPARED_BELOW_COST)
            assert_tick_matches(dumped, o, (seed, tick), cost_atol=COST_ATOL, traj_atol=FUZZ_TRAJ_ATOL, traj_mask=tame)
            assert_tick_matches(g, o, (seed, tick), rows=False, cost_atol=COST_ATOL, traj_atol=FUZZ_TRAJ_ATOL, traj_mask=tame)
            kept = PS.kept_of_tick(state, PS.predictions(O, state, prev, tick, dt), o["normal"], o["d"], f["vmax"], f["amax"], dt)
            band.check(pl, kept, (seed, tick))
            stale = np.where(ok[:, None, None], g["traj"], stale).astype(np.float32)
            prev = g["traj"]
            state = next_state_host(prev)
        pl.close()
    assert band.agent_ticks >= 6 * 2 * 24 and band.kept > 0
    band.close()
