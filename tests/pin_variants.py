"""What the HiGHS pins of the QP variants share (tests/golden/make_qp_pin_variants.py writes the fixtures, tests/test_oracle_pin_variants.py
and tests/test_gpu_highs_variants.py read them): the four families, how the oracle flies one of their missions, how one agent's QP of a
recorded tick is assembled and what HiGHS (tests/highs_qp.py) says about it.  A fifth family, obs (tests/golden/make_qp_pin_obstacles.py),
holds swarms that plan against dynamic obstacles.

Families -- each a way of building or solving an agent's QP that the 90-variable empty-map pins (tests/golden/qp_pin_ticks.npz) never reach:
    corridor  M = 5, 3-D, use_sfc on the forest map: six box half-spaces per segment; the boxes have a history, so every tick is recorded
    planar    world_dimension = 2, world_z_2d = 1.0: the 60-variable QP; every kept tick is replayed on its own
    m4        dt = 0.5, horizon = 2.0: the 72-variable QP of the four-segment build; every kept tick is replayed on its own
    tp        one tick of the 320-agent swarm of tests/test_gpu_round2.py::test_throughput_build_agrees_with_the_latency_build
    obs       dynamic obstacles behind the other agents in every agent's row set (tests/obstacle_reference.py composes the tick): missions
              crossing, pursuit and crowd (OBS_SCENES); the stale-trajectory rule has a history, so every tick from 1 is recorded and judged
    obs_m4    the obs family's mission at dt = 0.5, horizon = 2.0 (the four-segment build); it shares the obs family's file and conditions

Verdict of an agent's QP: 1 certified infeasible (phase-1 LP: minimal uniform violation of the rows > 1e-7), 0 optimal with this cost,
2 optimal with at most this cost (HiGHS stopped short of a feasible point with a lower objective), -1 no verdict (too close to call, HiGHS
gave up, or the corridor's seed box was blocked: status 4, no QP).

TEST INFRASTRUCTURE ONLY.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = {"corridor": "qp_pin_corridor.npz", "planar": "qp_pin_variants.npz", "m4": "qp_pin_variants.npz", "tp": "qp_pin_tp.npz",
         "obs": "qp_pin_obstacles.npz", "obs_m4": "qp_pin_obstacles.npz"}
OBS_FAMILIES = ("obs", "obs_m4")
MISSION_KEYS = ("start", "goal", "world_min", "world_max", "radius", "downwash", "max_vel", "max_acc", "nominal_velocity")

# What the generator printed; both test files assert these counts on the committed arrays.
#            family: (certified infeasible, optimal incl. upper bounds, no verdict, optimal with x_ok false, status-4 agent-ticks)
COUNTS = {"corridor": (20, 291, 0, 0, 1), "planar": (79, 125, 0, 0, 0), "m4": (19, 165, 2, 0, 0), "tp": (0, 40, 0, 0, 0),
          "obs": (91, 609, 0, 0, 0), "obs_m4": (0, 128, 0, 0, 0)}
# ... and what pin_variants.obs_conditions counts on the obs family's file (active: agent-ticks with an obstacle's row active at HiGHS's point)
OBS_COUNTS = {"infeasible": 91, "infeasible_pursuit": 34, "optimal_x_ok": 737, "no_verdict": 0, "judged": 828, "twice_infeasible_after_feasible": 17,
              "active": {"crossing": 56, "pursuit": 65, "crowd": 58, "crossing_m4": 59}}


def family_params(fam):
    """(M, dt, oracle parameters, PlannerConfig keywords) of a family."""
    if fam == "obs_m4":
        return 4, 0.5, dict(dt=0.5), dict(dt=0.5, horizon=2.0)
    if fam == "corridor":
        return 5, 0.2, dict(use_sfc=True), dict(use_octomap=True)
    if fam == "planar":
        return 5, 0.2, dict(world_dimension=2, world_z_2d=1.0), dict(world_dimension=2, world_z_2d=1.0)
    if fam == "m4":
        return 4, 0.5, dict(dt=0.5), dict(dt=0.5, horizon=2.0)
    return 5, 0.2, {}, {}


def load(fam):
    return np.load(os.path.join(GOLDEN, FILES[fam]))


def missions_of(Z, fam):
    return int(Z[fam + "_count"])


def mission(Z, fam, i):
    import lsc_planner_amd as L
    return L.Mission(*[Z[f"{fam}{i}_{k}"] for k in MISSION_KEYS])


def forest_distmap(O, world_min, world_max):
    """The forest map's distance field over a mission's world (the swarms of the corridor family fly in the middle of the map)."""
    from maputil import forest_leaves
    leaves, res = forest_leaves()
    return O.DistMap(leaves, res, world_min, world_max), res


def oracle_swarm(O, fam, ms, dm=None):
    """(params, Swarm) of the family's oracle for this mission.  Inside O.segments(M) of the family."""
    M, dt, okw, _ = family_params(fam)
    prm = O.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True, **okw)
    sw = O.Swarm(prm, ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
    if fam == "corridor":
        sw.set_distmap(dm)
    return prm, sw


def fly(O, fam, ms, ticks, dm=None, nthreads=8, obstacles=None):
    """The oracle flies the mission from its start: per tick (state, previous plans, the oracle's result with its LSC dump).
    obs families: `obstacles` is the mission's "obstacles" list; ObstacleSet moves them from the agents' float32 states (the first tick
    evaluates at t = dt), the composed reference plans, and a tick's result carries the obstacles' float32 [K][6] states as "obs"."""
    from lsc_planner_amd.planner import next_state_host
    M, dt, _, _ = family_params(fam)
    if fam in OBS_FAMILIES:
        from lsc_planner_amd.obstacles import ObstacleSet
        from obstacle_reference import ObstacleSwarm
        S = ObstacleSet(obstacles, n_agents=ms.qn)
        ref = ObstacleSwarm(O, ms, S.radius, S.downwash, dt=dt)
        state = np.zeros((ms.qn, 9), np.float32)
        state[:, :3] = ms.start
        traj = np.zeros((ms.qn, 3, 6 * M), np.float32)
        hist = []
        for tick in range(1, ticks + 1):
            pos, vel = S.at(dt * tick, state[:, :3])
            o = ref.tick(state, ms.goal, traj, tick, pos, vel)
            o["obs"] = np.concatenate([pos, vel], axis=1)
            hist.append((state.copy(), traj.copy(), o))
            traj = o["traj"]
            state = next_state_host(traj, dt=dt)
        return ref.prm, hist
    prm, sw = oracle_swarm(O, fam, ms, dm)
    n = ms.qn
    state = np.zeros((n, 9), np.float32)
    state[:, :3] = ms.start
    traj = np.zeros((n, 3, 6 * M), np.float32)
    if fam == "planar":
        # an agent whose FIRST solve fails keeps the plan it was created with: all zeros in the reference, which reads the agent's own height as
        # world/z_2d afterwards; the product starts that plan in the plane (lsc_set_agents) and refuses inputs outside it, so the recorded
        # inputs are in the plane too
        sw.stale[:, 2, :] = np.float32(prm.world_z_2d)
    hist = []
    for tick in range(1, ticks + 1):
        o = sw.tick(state, ms.goal, traj, tick, want_lsc=True, nthreads=nthreads)
        hist.append((state.copy(), traj.copy(), o))
        traj = o["traj"]
        state = next_state_host(traj, dt=dt)
    return prm, hist


def agent_qp(O, fam, prm, ms, a, state, traj, tick, o):
    """QP of agent a on a tick's inputs, from the oracle's assembly with the tick's LSC dump (and corridor boxes)."""
    M, dt, _, _ = family_params(fam)
    n = ms.qn
    others = [j for j in range(n) if j != a]
    obs = np.array([O.shift_traj(traj[j]) if tick >= 2 else O.const_vel_traj(state[j, :3], state[j, 3:6], dt) for j in others])
    if fam in OBS_FAMILIES:
        # an obstacle is predicted from its current state at every planner_seq and follows the other agents; its rows are the tick's dump
        # (lsc_pair(..., dw_a = 1.0, ...): tests/obstacle_reference.py; the oracle test holds the dump to lsc_pair on the recorded inputs)
        pv = o["obs"]
        obs = np.concatenate([obs.reshape(n - 1, 3, 6 * M), np.array([O.const_vel_traj(p[:3], p[3:], dt) for p in pv]).reshape(len(pv), 3, 6 * M)])
    own = state[a]
    if fam == "planar":
        own = own.copy()
        own[2] = np.float32(prm.world_z_2d)
    return O.qp_assemble(prm, own, ms.goal[a], float(ms.nominal_velocity[a]), ms.max_vel[a], ms.max_acc[a], obs, o["normal"][a], o["d"][a],
                         sfc=o["sfc"][a] if fam == "corridor" else None)


def highs_verdict(H, qp):
    """(verdict, cost, x) of one QP; x is HiGHS's point (None without an optimum)."""
    A, lo, hi = H.rows_of(qp)
    st, t = H.min_violation(A, lo, hi, qp.lo, qp.hi)
    if st == "Optimal" and t > 1e-7:
        return 1, 0.0, None                              # certificate: the rows cannot all hold
    if not (st == "Optimal" and t <= 1e-9):
        return -1, 0.0, None                             # too close to call
    ms_, x, obj, viol = H.solve_oracle_qp(qp)
    if not (ms_ == "Optimal" and viol <= 1e-7):
        return -1, 0.0, None
    verdict = 0
    # HiGHS's active-set code stops ~1e-6 short on a few instances: when a point that satisfies the ORIGINAL rows to 1e-9 has a lower
    # objective, HiGHS's number is only an upper bound of the optimum (the rule of tests/golden/make_qp_pin_ticks.py)
    st_o, xo, co, _, _ = qp.solve()
    if st_o == 0 and co < obj - (1e-7 * abs(obj) + 1e-9):
        vo = max(np.max(lo - A @ xo), np.max(A @ xo - hi), np.max(qp.lo - xo), np.max(xo - qp.hi))
        if vo <= 1e-9:
            verdict = 2
    return verdict, obj, x


def obstacle_row_active(O, H, fam, prm, ms, a, state, traj, tick, o, qp, x):
    """Whether a row of a dynamic obstacle is active (|a.x - b| < 1e-7) at the point x of agent a's QP.  The obstacles' rows are the rows
    the QP loses when it is assembled over the other agents alone: no assumption on the order of the assembly."""
    K = len(o["obs"])
    bare = dict(o, obs=o["obs"][:0], normal=o["normal"][:, :ms.qn - 1], d=o["d"][:, :ms.qn - 1])
    A0, lo0, hi0 = H.rows_of(agent_qp(O, fam, prm, ms, a, state, traj, tick, bare))
    A, lo, hi = H.rows_of(qp)
    agents_rows = {}
    for r in range(len(A0)):
        k = (A0[r].tobytes(), lo0[r], hi0[r])
        agents_rows[k] = agents_rows.get(k, 0) + 1
    mine = np.zeros(len(A), bool)
    for r in range(len(A)):
        k = (A[r].tobytes(), lo[r], hi[r])
        if agents_rows.get(k, 0) > 0:
            agents_rows[k] -= 1
        else:
            mine[r] = True
    assert mine.sum() == len(A) - len(A0) and (K == 0 or mine.sum() % K == 0), (mine.sum(), len(A), len(A0))
    ax = A[mine] @ np.asarray(x)
    return bool(((np.abs(ax - lo[mine]) < 1e-7) | (np.abs(ax - hi[mine]) < 1e-7)).any())


def tick_verdicts(O, H, fam, prm, ms, state, traj, tick, o, agents=None, active=None):
    """HiGHS on the QPs of one tick: (verdict int32 [N], cost [N], x float32 [N][dim][6 M], x_ok bool [N]); agents outside `agents`
    and status-4 agents get no verdict.  active (obs families): a bool [N] that is set where an obstacle's row is active at HiGHS's point."""
    from tolerances import ACTIVE_SET_TRAJ_ATOL as TRAJ_ATOL          # (TRAJ_ATOL, whatever LSC_SOLVER says)
    M = family_params(fam)[0]
    n, dim = ms.qn, 2 if fam == "planar" else 3
    verdict = np.full(n, -1, np.int32)
    cost = np.zeros(n)
    xs = np.zeros((n, dim, 6 * M), np.float32)
    x_ok = np.zeros(n, bool)
    for a in (range(n) if agents is None else agents):
        if o["status"][a] == 4:
            continue
        qp = agent_qp(O, fam, prm, ms, a, state, traj, tick, o)
        v, c, x = highs_verdict(H, qp)
        verdict[a], cost[a] = v, c
        if x is not None and active is not None:
            active[a] = obstacle_row_active(O, H, fam, prm, ms, a, state, traj, tick, o, qp, x)
        if x is not None:
            x = np.asarray(x)[:dim * 6 * M].reshape(dim, 6 * M)
            xs[a] = x.astype(np.float32)
            x_ok[a] = o["status"][a] == 0 and np.abs(x - o["traj"][a][:dim]).max() <= TRAJ_ATOL / 2
    return verdict, cost, xs, x_ok


def kept_ticks(Z, fam, i):
    """[(index into the mission's kept arrays, tick)]."""
    return list(enumerate(int(t) for t in np.atleast_1d(Z[f"{fam}{i}_kept"])))


def tick_inputs(Z, fam, i, k, tick):
    """(state, previous plans) of kept tick number k: the corridor family records every tick from 1, the others their kept ticks only."""
    if fam == "corridor" or fam in OBS_FAMILIES:
        return Z[f"{fam}{i}_states"][tick - 1], Z[f"{fam}{i}_trajs"][tick - 1]
    return Z[f"{fam}{i}_states"][k], Z[f"{fam}{i}_trajs"][k]


def counts(Z, fam):
    """(certified infeasible, optimal, no verdict, optimal with x_ok false, status-4 agent-ticks on kept ticks) over the family."""
    n_inf = n_opt = n_none = n_far = n_blocked = 0
    for i in range(missions_of(Z, fam)):
        v, ok = Z[f"{fam}{i}_verdict"], Z[f"{fam}{i}_xok"]
        judged = Z[f"{fam}{i}_judged"]                  # agents HiGHS was asked about (tp: a subset; status-4 agents never)
        opt = (v == 0) | (v == 2)
        n_inf += int((v == 1).sum()); n_opt += int(opt.sum()); n_none += int(((v < 0) & judged).sum()); n_far += int((opt & ~ok).sum())
        n_blocked += int((Z[f"{fam}{i}_ostatus_kept"] == 4).sum())
    return n_inf, n_opt, n_none, n_far, n_blocked


# ------------------------------------------------------------------------------------------------ the obs family's scenes and conditions
# Mission names by family, in the order of the file's mission numbers.
OBS_SCENES = {"obs": ("crossing", "pursuit", "crowd"), "obs_m4": ("crossing_m4",)}
# Picked on the CPU (speeds 0.3 to 0.6 m/s, seeds, chaser limits and targets) until the composed reference and HiGHS alone met OBS_CONDITIONS.
OBS_PARAMS = {
    # the 8-agent circle of hover_mission() (R = 3 m); hover's three spheres start on a 2 m circle and cross it through the middle
    "crossing": dict(speed=0.4, seed=3, ticks=40),
    # the same circle; a chaser faster than the agents' 1.0 m/s per target agent and one gaussian walker
    "pursuit": dict(targets=(0, 3, 5), max_vel=1.5, max_acc=3.0, ticks=40),
    # 12 agents and 54 small spheres inside their circle: N - 1 + K = 65, the generic LSC build with its in-kernel list
    "crowd": dict(n=12, k=54, circle=2.0, seed=5, ticks=5),
    "crossing_m4": dict(speed=0.4, seed=3, ticks=16),
}
# What the family's fixtures were made for (the issue's conditions); the generator and both test files assert them.
OBS_CONDITIONS = dict(min_infeasible=20, min_infeasible_pursuit=1, min_optimal_x_ok=100, max_no_verdict=0.01, min_twice_infeasible_after_feasible=1)


def obs_scene(name, **override):
    """(mission, the mission's "obstacles" list as ObstacleSet reads it, ticks flown) of a scene of the obs family."""
    import lsc_planner_amd as L
    from obstacle_reference import HOVER_DOWNWASH, HOVER_RADIUS, hover_mission
    p = dict(OBS_PARAMS[name], **override)
    if name in ("crossing", "crossing_m4"):
        ms = hover_mission()
        ang = np.random.default_rng(p["seed"]).uniform(0.0, 2.0 * np.pi, 3)
        obstacles = [{"type": "straight", "start": [2.0 * np.cos(a), 2.0 * np.sin(a), z], "goal": [-2.0 * np.cos(a), -2.0 * np.sin(a), z],
                      "size": float(r), "speed": p["speed"], "downwash": float(dw)}
                     for a, z, r, dw in zip(ang, (1.0, 1.3, 0.8), HOVER_RADIUS, HOVER_DOWNWASH)]
    elif name == "pursuit":
        from pursuit_scenario import WALKER_MAX_ACC, WALKER_STDDEV, acc_table, chaser
        ms = hover_mission()
        obstacles = []
        for t in p["targets"]:
            # each chaser starts 1.2 m in front of its target, on the target's way to the middle
            s = ms.start[t].astype(np.float64) * (1.8 / 3.0)
            obstacles.append(chaser([float(s[0]), float(s[1]), 1.0], int(t), max_vel=p["max_vel"], max_acc=p["max_acc"]))
        n_acc = int(np.floor((0.2 * p["ticks"] + 1e-5) / 0.5)) + 1            # _Walker.entries at the last tick's time
        obstacles.append({"type": "gaussian", "start": [-0.5, 0.4, 1.2], "initial_vel": [0.1, 0.0, 0.0], "size": 0.2, "max_vel": 0.25,
                          "stddev_acc": WALKER_STDDEV, "max_acc": WALKER_MAX_ACC, "acc_update_cycle": 0.5, "downwash": 1.5,
                          "acc_history": acc_table(n_acc).tolist()})
    else:
        n, k, R = p["n"], p["k"], p["circle"]
        ms = L.circle_swap(n, circle_radius=R, world=(-R - 2, -R - 2, 0, R + 2, R + 2, 2.5))
        rng = np.random.default_rng(p["seed"])
        ang, rad = rng.uniform(0, 2 * np.pi, k), R * (0.15 + 0.7 * np.sqrt(rng.uniform(0, 1, k)))
        start = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(0.5, 1.7, k)], axis=1)
        step = rng.normal(size=(k, 3)) * [1.0, 1.0, 0.2]
        size, dw = rng.uniform(0.08, 0.2, k), rng.uniform(1.0, 2.0, k)
        obstacles = [{"type": "straight", "start": start[j].tolist(), "goal": (start[j] + step[j]).tolist(), "size": float(size[j]), "speed": 0.05,
                      "downwash": float(dw[j])} for j in range(k)]
    return ms, obstacles, p["ticks"]


def obs_conditions(Z):
    """What OBS_CONDITIONS speaks of, counted on the arrays of the obs family's file (both of its families)."""
    got = dict(infeasible=0, infeasible_pursuit=0, optimal_x_ok=0, no_verdict=0, judged=0, twice_infeasible_after_feasible=0, active={})
    for fam in OBS_FAMILIES:
        for i, name in enumerate(OBS_SCENES[fam]):
            v, ok, judged = Z[f"{fam}{i}_verdict"], Z[f"{fam}{i}_xok"], Z[f"{fam}{i}_judged"]
            got["infeasible"] += int((v == 1).sum())
            if name == "pursuit":
                got["infeasible_pursuit"] += int((v == 1).sum())
            got["optimal_x_ok"] += int((((v == 0) | (v == 2)) & ok).sum())
            got["no_verdict"] += int(((v < 0) & judged).sum())
            got["judged"] += int(judged.sum())
            # (every tick is judged: rows t - 1, t, t + 1 of the verdicts are consecutive ticks)
            got["twice_infeasible_after_feasible"] += int(((v[:-2] == 0) & (v[1:-1] == 1) & (v[2:] == 1)).sum())
            got["active"][name] = int(Z[f"{fam}{i}_obs_active"].sum())
    return got


def assert_obs_conditions(got):
    c = OBS_CONDITIONS
    assert got["infeasible"] >= c["min_infeasible"] and got["infeasible_pursuit"] >= c["min_infeasible_pursuit"], got
    assert got["optimal_x_ok"] >= c["min_optimal_x_ok"], got
    assert got["no_verdict"] <= c["max_no_verdict"] * got["judged"], got
    assert got["twice_infeasible_after_feasible"] >= c["min_twice_infeasible_after_feasible"], got
    assert set(got["active"]) == {n for names in OBS_SCENES.values() for n in names} and all(n > 0 for n in got["active"].values()), got
