"""The neighbour-list kernels (lsc_planner_amd/csrc/lsc_neigh.hip: lsc_neigh_build_kernel, lsc_neigh_query_kernel<WIDE>) held by value to a
float64 statement of what they must compute (tests/neighbour_reference.py), through SwarmPlanner.neighbour_dump().

The lists decide which (obstacle, segment) units an agent's LSC build ever looks at; a unit wrongly left out is a collision constraint
that silently disappears from a QP.  The plan-against-plan tests (test_gpu_round6.py, test_gpu_large_swarms.py) notice that only when the
missing unit carries a row that survives pruning in the mission flown.  Here every link of the chain is compared on its own:

  a  the spheres contain their points, and are not absurdly loose;
  b  the closed-form reach B_m dominates phase B's cullB[m] and is tight against the kernel's own bound in exact arithmetic;
  c  the swarm-wide query radius G dominates every agent's contribution and is tight;
  d  the list IS the sphere test, two-sided and by brute force over all (N - 1) M units (cell box, clamp, hash, buckets, overflow list,
     bitmap, prefix sums and the wide decode all show here);
  e  the list keeps every unit phase B's own float64 pre-cull keeps;
  f  the priority candidates are the agents within priority_dist_threshold, as sets;
  g  the disturbance bit is the oracle's "somebody is or was off its plan";
  h  no scene passes by listing nothing: nearly every agent has a list, and both sides of (d) are met.

Every scene prints one line per checked tick ("neighbour lists: ..."): run time, share of agents with a list, units listed / must be
listed / either / must not be listed / kept by phase B's pre-cull.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import neighbour_reference as R
from harness import start_inputs
from test_gpu_round6 import _Env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N0 = 512                                   # the smallest swarm that gets lists
WORLD = (-14, -14, 0, 14, 14, 5)           # 512 agents at random1024's density (1024 in 40 x 40 x 5 m)


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    return L


def _swarm(L, seed, world=WORLD, n=N0):
    return L.random_swarm(n, world=world, seed=seed, min_sep=0.5)


def _planner(L, ms, env=None, **cfg):
    with _Env(LSC_NEIGH_ALWAYS=1, **(env or {})):
        return L.SwarmPlanner(ms, L.PlannerConfig(prune=1, **cfg))


def check_dump(O, pl, ms, state, traj, seq, what, *, agents=None, share=0.99, precull=True, t0=None):
    """Assertions (a)-(f), (h) on the dump of the tick just planned from (state, traj, seq).  agents: whose lists are checked (default: the
    shard).  Returns (dump, per-agent classification used by the scenes that look at particular units)."""
    t0 = time.perf_counter() if t0 is None else t0
    N, M, dt = pl.N, pl.M, pl.cfg.dt
    planar = pl.cfg.world_dimension == 2
    state = np.asarray(state, np.float32)
    d = pl.neighbour_dump()
    P = R.predicted_points(O, state, traj, seq, dt, M)
    pos = state[:, :3].astype(np.float64)
    r, dw = np.asarray(ms.radius, np.float64), np.asarray(ms.downwash, np.float64)
    sb, ob, reach = d["seg_bound"].astype(np.float64), d["obs_bound"].astype(np.float64), d["reach"].astype(np.float64)
    # ---- a: spheres contain their points (distances in float64 to the stored float32 centre), within ten times the kernel's own pad
    far = np.sqrt(((P - sb[:, :, None, :3]) ** 2).sum(-1)).max(-1)
    assert (far <= sb[:, :, 3]).all(), (what, "a point outside its segment's sphere", (far - sb[:, :, 3]).max())
    assert (sb[:, :, 3] <= (1.0 + 1e-4) * far + 1e-4).all(), (what, "segment sphere too loose", (sb[:, :, 3] - far).max())
    allp = np.concatenate([P.reshape(N, -1, 3), pos[:, None, :]], axis=1)
    faro = np.sqrt(((allp - ob[:, None, :3]) ** 2).sum(-1)).max(-1)
    assert (faro <= ob[:, 3]).all(), (what, "a point outside its agent's sphere", (faro - ob[:, 3]).max())
    assert (ob[:, 3] <= (1.0 + 1e-4) * faro + 1e-4).all(), (what, "agent sphere too loose", (ob[:, 3] - faro).max())
    # ---- b: the reach dominates phase B's cullB and is tight against the kernel's bound in exact arithmetic
    cullB, bound = R.cull_b(state, P, ms.max_vel, ms.max_acc, dt, planar, pl.cfg.world_z_2d)
    assert (reach >= cullB).all(), (what, "reach below cullB", (cullB - reach).max())
    assert (reach <= bound * (1.0 + 1e-4) + 1e-4).all(), (what, "reach above the kernel's own bound", (reach - bound).max())
    # ---- c: the query radius dominates 3 sc_max max_m rho_o^m + r_o + rho_o of every agent, and is tight
    sc_max = max(1.0, 1.0 / dw.min())
    g = 3.0 * sc_max * sb[:, :, 3].max(axis=1) + r.astype(np.float32).astype(np.float64) + ob[:, 3]
    G = d["query_radius"]
    assert G >= g.max() and G <= g.max() * (1.0 + 1e-4) + 1e-4, (what, "query radius", G, g.max())
    # ---- d, e: the list against the sphere test on the dumped spheres, and against phase B's pre-cull on the raw control points
    agents = list(range(pl.first, pl.first + pl.count)) if agents is None else list(agents)
    cnt = d["unit_count"]
    have = [q for q in agents if cnt[q] >= 0]
    assert len(have) >= share * len(agents), (what, "agents with a list", len(have), len(agents))
    n_units = (N - 1) * M
    tot = dict(listed=0, must=0, either=0, never=0, precull=0)
    cls = {}
    for q in have:
        u = d["units"][q]
        assert len(u) == cnt[q] and (np.diff(u) > 0).all() and (len(u) == 0 or (u[0] >= 0 and u[-1] < n_units)), (what, q, "list not ascending / out of range")
        idx = R.unit_index(q, N, M)
        other = idx >= 0
        flat = np.zeros(n_units, bool)
        flat[u] = True
        listed = np.zeros((N, M), bool)
        listed[other] = flat[idx[other]]
        base, dist = R.sphere_test(q, d["seg_bound"], d["reach"], r, dw)
        must = other & (dist < base + 2e-4)
        never = other & (dist >= base * (1.0 + 1e-4) + 1e-3)
        assert listed[must].all(), (what, q, "unit inside the sphere test is not listed", np.argwhere(must & ~listed)[:4], (base - dist)[must & ~listed][:4])
        assert not listed[never].any(), (what, q, "unit outside the sphere test is listed", np.argwhere(never & listed)[:4])
        if precull:
            idw, _ = R.pair_scale(r[q], dw[q], r, dw)
            keep = other & R.unit_test_keeps_all(P[q], P, idw, cullB[q], r[q] + r)
            assert listed[keep].all(), (what, q, "unit kept by phase B's pre-cull is not listed", np.argwhere(keep & ~listed)[:4])
            tot["precull"] += int(keep.sum())
        tot["listed"] += len(u); tot["must"] += int(must.sum()); tot["never"] += int(never.sum())
        tot["either"] += int((other & ~must & ~never).sum())
        cls[q] = (must, never, listed)
    # ---- h: both sides of (d) were met
    assert tot["must"] > 0 and tot["never"] > 0 and 0 < tot["listed"] < len(have) * n_units, (what, tot)
    # ---- f: priority candidates as sets
    if pl.cfg.goal_mode == "prior_based":
        thr = pl.cfg.priority_dist_threshold
        n_in = n_none = 0
        for q in agents:
            dd = R.priority_dist(state, q)
            dd[q] = np.inf
            inside = np.flatnonzero(dd < thr)
            pc = d["priority_count"][q]
            assert pc == -1 or len(inside) <= 64, (what, q, "more than 64 candidates and a count", pc, len(inside))
            if pc == -1:
                assert not (cnt[q] >= 0 and len(inside) <= 16), (what, q, "no candidate list", len(inside))
                n_none += 1
                continue
            cand = d["priority"][q]
            assert len(cand) == pc and q not in cand, (what, q)
            assert set(inside.tolist()) <= set(cand.tolist()), (what, q, "a candidate within the threshold is missing")
            assert (dd[cand] < thr * (1.0 + 1e-5) + 1e-6).all(), (what, q, "a candidate beyond the threshold")
            n_in += len(inside)
        tot["priority_inside"], tot["priority_no_list"] = n_in, n_none
    else:
        assert (d["priority_count"][agents] == 0).all(), what
    tot.update(scene=what, seconds=round(time.perf_counter() - t0, 2), with_list=round(len(have) / len(agents), 4), agents=len(agents))
    print("neighbour lists:", json.dumps(tot), flush=True)
    return d, cls


def fly_and_check(L, O, ms, what, ticks, dump_at, *, env=None, state=None, planar_z=None, share=0.99, **cfg):
    """Host-buffer ticks 1..ticks of one planner with forced lists; the ticks in dump_at are dumped and checked.  Returns the last dump."""
    from lsc_planner_amd.planner import next_state_host
    pl = _planner(L, ms, env, **cfg)
    state0, traj = start_inputs(ms, pl.SEGV)
    state = state0 if state is None else state
    out = None
    for tick in range(1, ticks + 1):
        t0 = time.perf_counter()
        g = pl.plan(state, ms.goal, traj)
        if tick in dump_at:
            out = check_dump(O, pl, ms, state, traj, tick, f"{what}, tick {tick}", share=share, t0=t0)
        traj = g["traj"]
        state = next_state_host(traj, dt=pl.cfg.dt)
        if planar_z is not None:
            state[:, 2] = planar_z; state[:, 5] = 0.0; state[:, 8] = 0.0
    pl.close()
    return out


def test_dump_says_when_there_is_nothing_to_dump(L):
    """lsc_neighbour_dump refuses (LSC_ESTATE, with the cause) before the first tick, on a context without lists, and after a tick whose
    lists would not pay -- 512 agents are one round of workgroups -- instead of handing out what an older tick left."""
    ms = _swarm(L, 1)
    forced, plain = _planner(L, ms), L.SwarmPlanner(ms, L.PlannerConfig(prune=1))
    with _Env(LSC_NO_NEIGHBOUR_LISTS=1):
        none = L.SwarmPlanner(ms, L.PlannerConfig(prune=1))
    with pytest.raises(L.LscError, match="no tick has run"):
        forced.neighbour_dump()
    state, traj = start_inputs(ms, forced.SEGV)
    for pl in (forced, plain, none):
        pl.plan(state, ms.goal, traj)
    assert forced.neighbour_dump()["query_radius"] > 0.0
    with pytest.raises(L.LscError, match="do not pay"):
        plain.neighbour_dump()
    with pytest.raises(L.LscError, match="builds no neighbour lists"):
        none.neighbour_dump()
    forced.plan(state, ms.goal, traj, want_constraints=True)          # (a tick that dumps its constraints walks all obstacles)
    with pytest.raises(L.LscError, match="dumps its constraints"):
        forced.neighbour_dump()
    for pl in (forced, plain, none):
        pl.close()


def test_baseline(L, oracle):
    """Scene 1: tick 1 (constant-velocity prediction) and tick 3 of the flown mission (shifted plans), priority candidates included."""
    fly_and_check(L, oracle, _swarm(L, 20261001), "baseline", 3, (1, 3), goal_mode="prior_based", priority_dist_threshold=1.5)


def test_agents_on_cell_boundaries(L, oracle):
    """Scene 2: LSC_NEIGH_CELL = 1: every agent sits on a lattice of integer multiples of the cell in x and y (negative, zero, positive)
    and of the tall cell (2 m: downwash 2) in z, half of them np.nextafter below it: the floor() of the insertion and the cell box of the
    query have to agree on which side of a boundary a centre lies."""
    rng = np.random.default_rng(2)
    sites = np.array([(x, y, z) for x in range(-13, 14) for y in range(-13, 14) for z in (2.0, 4.0)], np.float32)
    pick = rng.permutation(len(sites))
    start, goal = sites[pick[:N0]].copy(), sites[pick[N0:2 * N0]].copy()
    below = rng.random(N0) < 0.5
    start[below] = np.nextafter(start[below], np.float32(-np.inf))
    ms = _swarm(L, 2)
    ms.start[:], ms.goal[:] = start, goal
    fly_and_check(L, oracle, ms, "cell boundaries", 2, (1, 2), env=dict(LSC_NEIGH_CELL=1.0), goal_mode="prior_based", priority_dist_threshold=1.0)


def test_full_bucket(L, oracle):
    """Scene 3: 40 agents at 0.35 m spacing (0.8 m in z) inside one default cell (1.6 x 1.6 x 3.2 m), the rest spread out: a bucket holds
    twelve, the others go through the overflow list.  Every crowd agent must list more than twelve crowd partners -- so at least one that
    sat in a slot >= 12 --, (d) holds for them, and their lists stay below the 1024-unit capacity."""
    crowd = np.array([(0.2 + 0.35 * i, 0.2 + 0.35 * j, 0.6 + 0.8 * k) for k in range(3) for j in range(4) for i in range(4)], np.float32)[:40]
    ms = _swarm(L, 3)
    away = np.flatnonzero((np.abs(ms.start[:, :2] - 0.8).max(axis=1) > 2.0))[:N0 - 40]
    assert len(away) == N0 - 40
    ms.start[:] = np.concatenate([crowd, ms.start[away]])
    pl = _planner(L, ms)
    state, traj = start_inputs(ms, pl.SEGV)
    pl.plan(state, ms.goal, traj)
    d, cls = check_dump(oracle, pl, ms, state, traj, 1, "full bucket, tick 1", share=0.5)
    for q in range(40):
        assert 0 <= d["unit_count"][q] < 1024, (q, d["unit_count"][q])
        must, never, listed = cls[q]
        assert (must[:40].any(axis=1).sum() > 12) and listed[:40][must[:40]].all(), q
    pl.close()


def test_far_from_the_origin(L, oracle):
    """Scene 4: the baseline swarm translated by (1000, -2000, 50), two ticks: a float32 ulp of a coordinate is 1.2e-4 m there, which the
    1e-5 |coordinate| pads of B_m and of the cell box have to cover.  The geometric assertions only."""
    ms = _swarm(L, 20261001)
    off = np.array([1000.0, -2000.0, 50.0], np.float32)
    ms.start[:] = ms.start + off; ms.goal[:] = ms.goal + off
    ms.world_min[:] = ms.world_min + off; ms.world_max[:] = ms.world_max + off
    fly_and_check(L, oracle, ms, "far from the origin", 2, (1, 2), goal_mode="prior_based", priority_dist_threshold=1.5)


def test_heterogeneous_agents(L, oracle):
    """Scene 5: radius 0.1-0.3, downwash 0.5-3.7 (both sides of 1: s > 1 and tall z cells), per-axis max_vel 0.3-2.5 and max_acc 0.5-6;
    the priority threshold of 7 m puts more than 64 agents within it in the middle of the world and fewer at its corners."""
    rng = np.random.default_rng(5)
    ms = _swarm(L, 5)
    ms.radius[:] = rng.uniform(0.1, 0.3, N0)
    ms.downwash[:] = rng.uniform(0.5, 3.7, N0)
    ms.max_vel[:] = rng.uniform(0.3, 2.5, (N0, 3))
    ms.max_acc[:] = rng.uniform(0.5, 6.0, (N0, 3))
    d, _ = fly_and_check(L, oracle, ms, "heterogeneous agents", 2, (1, 2), goal_mode="prior_based", priority_dist_threshold=7.0)
    assert (d["priority_count"] == -1).any() and (d["priority_count"] > 16).any()


def test_states_at_and_beyond_the_limits(L, oracle):
    """Scene 6, planner_seq = 1: velocities exactly +-vmax, 1.3 vmax (nh = 0: every step clamped), accelerations +-1.3 amax, and zero
    velocity with the acceleration at its limit -- the branches of reach_hi / reach_lo and their floor()."""
    rng = np.random.default_rng(6)
    ms = _swarm(L, 6)
    ms.max_vel[:] = rng.uniform(0.5, 1.5, (N0, 3))
    ms.max_acc[:] = rng.uniform(1.0, 4.0, (N0, 3))
    state, _ = start_inputs(ms, 30)
    sign = np.where(rng.random((N0, 3)) < 0.5, -1.0, 1.0)
    kind = np.arange(N0) % 4
    v = np.where(kind[:, None] == 0, sign * ms.max_vel, np.where(kind[:, None] == 1, 1.3 * sign * ms.max_vel, rng.uniform(-1, 1, (N0, 3)) * ms.max_vel))
    v[kind == 3] = 0.0
    a = np.where(kind[:, None] == 2, 1.3 * sign * ms.max_acc, np.where(kind[:, None] == 3, sign * ms.max_acc, rng.uniform(-1, 1, (N0, 3)) * ms.max_acc))
    state[:, 3:6], state[:, 6:9] = v, a
    fly_and_check(L, oracle, ms, "at and beyond the limits", 1, (1,), state=state)


def test_units_on_the_threshold(L, oracle):
    """Scene 7: 256 far-apart pairs of hovering agents.  A first dump gives base_m of every pair; then partner j stands at
    |D| = base_m (1 + delta) from its agent, for every segment m, delta in {-1e-3, -1e-6, +2e-4, +2e-3} and the directions x, z (the downwash
    scaling) and a diagonal.  delta < 0 must be listed; + 2e-3 must not (from segment 1 on: there 2e-3 base exceeds the band); + 2e-4 lies
    within 1e-4 of the kernel's own threshold, where either is right."""
    M, pairs = 5, N0 // 2
    ij = np.array([(i, j) for i in range(16) for j in range(16)], np.float64)
    a_pos = np.concatenate([(ij - 7.5) * 8.0, np.full((pairs, 1), 2.0)], axis=1)
    ms = _swarm(L, 7, world=(-66, -66, 0, 66, 66, 10))

    def place(offsets):
        ms.start[:] = np.concatenate([a_pos, a_pos + offsets]).astype(np.float32)
        ms.goal[:] = ms.start
        pl = _planner(L, ms)
        state, traj = start_inputs(ms, pl.SEGV)
        pl.plan(state, ms.goal, traj)
        return pl, state, traj

    pl, state, traj = place(np.tile([1.0, 0.0, 0.0], (pairs, 1)))
    d = pl.neighbour_dump()
    pl.close()
    base = np.stack([R.sphere_test(j, d["seg_bound"], d["reach"], ms.radius, ms.downwash)[0][pairs + j] for j in range(pairs)])      # [pairs][M]
    dirs = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0] / np.sqrt(3.0)])
    deltas = (-1e-3, -1e-6, 2e-4, 2e-3)
    case = [(j % M, deltas[(j // M) % 4], (j // (4 * M)) % 3) for j in range(pairs)]
    scale = np.array([1.0, 1.0, float(ms.downwash[0])])                       # (D = S (C_a - C_o): z counts 1 / downwash)
    pl, state, traj = place(np.stack([dirs[k] * scale * base[j, m] * (1.0 + dl) for j, (m, dl, k) in enumerate(case)]))
    d, cls = check_dump(oracle, pl, ms, state, traj, 1, "on the threshold, tick 1")
    met = dict(must=0, either=0, never=0)
    for j, (m, dl, k) in enumerate(case):
        must, never, listed = cls[j]
        o = pairs + j
        met["must" if must[o, m] else ("never" if never[o, m] else "either")] += 1
        if dl < 0:
            assert must[o, m] and listed[o, m], (j, m, dl, k)
        if dl == 2e-3 and m >= 1:
            assert never[o, m] and not listed[o, m], (j, m, dl, k)
    print("neighbour lists: on the threshold, the placed units:", met, flush=True)
    assert met["must"] >= pairs // 2 and met["never"] > 0
    pl.close()


def test_planar_world(L, oracle):
    """Scene 8a: world_dimension 2 (every agent at z = world_z_2d; c_{0,2} and d0 pinned along z)."""
    ms = _swarm(L, 8, world=(-14, -14, 0.4, 14, 14, 1.6))
    ms.start[:, 2] = 1.0; ms.goal[:, 2] = 1.0
    fly_and_check(L, oracle, ms, "planar world", 3, (1, 3), planar_z=1.0, world_dimension=2, world_z_2d=1.0, goal_mode="prior_based",
                  priority_dist_threshold=1.5)


def test_four_segment_library(L, oracle):
    """Scene 8b: the M = 4 build (dt 0.5, horizon 2): four lanes per agent carry a segment, K = 5 m + i - 2 runs to 18."""
    fly_and_check(L, oracle, _swarm(L, 84), "four segments", 3, (1, 3), dt=0.5, horizon=2.0)


def test_shard(L, oracle):
    """Scene 8c: set_shard(128, 256): lists exist only inside the shard; spheres, reach and the grid exist for all 512 (check_dump holds
    (a)-(c) for everybody and takes the lists of the shard)."""
    from lsc_planner_amd.planner import next_state_host
    ms = _swarm(L, 85)
    part, full = _planner(L, ms), L.SwarmPlanner(ms, L.PlannerConfig(prune=1))
    part.set_shard(128, 256)
    state, traj = start_inputs(ms, part.SEGV)
    for tick in (1, 2, 3):
        t0 = time.perf_counter()
        part.plan(state, ms.goal, traj)
        if tick != 2:
            d, _ = check_dump(oracle, part, ms, state, traj, tick, f"shard, tick {tick}", t0=t0)
            outside = np.r_[0:128, 384:N0]
            assert (d["unit_count"][outside] == 0).all() and (d["unit_count"][128:384] > 0).all()
        traj = full.plan(state, ms.goal, traj)["traj"]
        state = next_state_host(traj)
    part.close(); full.close()


def test_wide_lists(L, oracle):
    """Scene 9: 13 200 agents, M = 5: (N - 1) M = 65 995 > 0xffff, so the wide query kernel writes 16-bit entries and the start of the high
    block.  (a)-(c) for everybody, (d) for 256 agents: those next to the agents of the highest indices -- whose units are >= 65 536 --, those
    agents themselves, and an even spread."""
    n, M = 13200, 5
    rng = np.random.default_rng(9)
    nx = 67                                                            # 67 x 67 x 3 sites, 2.1 x 2.1 x 1.6 m apart: 0.13 agents per m^3
    sites = np.array([(x, y, z) for x in range(nx) for y in range(nx) for z in range(3)], np.float64)
    sites = (sites - [nx / 2, nx / 2, 0]) * [2.1, 2.1, 1.6] + [0.0, 0.0, 0.9]
    half = 2.1 * nx / 2 + 1.0

    def sample():
        return (sites[rng.permutation(len(sites))[:n]] + rng.uniform(-0.6, 0.6, (n, 3)) * [1, 1, 0.5]).astype(np.float32)
    start, goal = sample(), sample()
    ms = L.Mission(start, goal, np.array([-half, -half, 0], np.float32), np.array([half, half, 5], np.float32), np.full(n, 0.15), np.full(n, 2.0),
                   np.ones((n, 3)), np.full((n, 3), 2.0), np.ones(n), name="wide13200")
    high = np.arange(13110, n)
    near = [int(np.argsort(((start[:13000] - start[o]) ** 2 * [1, 1, 0.25]).sum(axis=1))[0]) for o in high]
    agents = set(near) | set(high.tolist())
    for q in np.linspace(0, n - 1, 512).astype(int).tolist():
        if len(agents) < 256:
            agents.add(q)
    agents = sorted(agents)
    assert len(agents) == 256
    pl = _planner(L, ms)
    state, traj = start_inputs(ms, pl.SEGV)
    t0 = time.perf_counter()
    pl.plan(state, ms.goal, traj)
    t1 = time.perf_counter()
    d, cls = check_dump(oracle, pl, ms, state, traj, 1, "wide, tick 1", agents=agents, precull=False, t0=t0)
    print("neighbour lists: wide, the tick alone took", round(t1 - t0, 2), "s", flush=True)
    top = [q for q in agents if d["unit_count"][q] > 0 and d["units"][q][-1] >= 65536]
    assert top and any(cls[q][0][13110:].any() for q in top), "no sampled agent lists a unit of the high block"
    pl.close()


@pytest.mark.parametrize("reset_threshold", [0.15, 0.0])
def test_disturbance_bit(L, oracle, reset_threshold):
    """(g) With reset_threshold = 0.15 agent 7 is pushed 0.3 m at tick 3: the bit every agent of the shard is handed is the oracle's
    (SwarmEx.disturbance_update: somebody is, or was, off its plan): 0 at ticks 1 and 2, 1 from tick 3 on.  With reset_threshold = 0 the
    checks are off and it stays 0."""
    from lsc_planner_amd.planner import next_state_host
    ms = _swarm(L, 20261001)
    pl = _planner(L, ms, reset_threshold=reset_threshold)
    ref = oracle.SwarmEx(oracle.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True), oracle.make_modes(reset_threshold=reset_threshold),
                         ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
    state, traj = start_inputs(ms, pl.SEGV)
    for tick in range(1, 6):
        if tick == 3:
            state[7, 0] += np.float32(0.3)
        g = pl.plan(state, ms.goal, traj)
        ref.disturbance_update(state, traj, tick)
        want = int(ref.slack_set.any())
        assert want == (1 if reset_threshold > 0 and tick >= 3 else 0), tick
        bit = pl.neighbour_dump()["disturbed"]
        assert (bit == want).all(), (tick, want, np.unique(bit))
        traj = g["traj"]
        state = next_state_host(traj)
    pl.close()


def test_lds_poison_library():
    """The scenes once more through the LDS-poison libraries (the query kernels keep their queue, bitmap and prefix sums in LDS; the plan
    kernels read the lists into theirs)."""
    lib = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_poison.so")
    lib4 = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_m4_poison.so")
    assert os.path.exists(lib) and os.path.exists(lib4), "the poison libraries are not built (make -C lsc_planner_amd/csrc poison poison_m4)"
    env = dict(os.environ, LSC_HIP_LIB=lib, LSC_HIP_LIB_M4=lib4)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", "not poison_library"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
