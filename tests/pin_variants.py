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
    modes     the alternate planner modes (tests/golden/make_qp_pin_modes.py): BVC, BVC with N_constraint_segments = 2, BVC with either
              slack mode, the disturbance reset in LSC mode, a 64-agent crowd and a planar world (MODES_SCENES); the QPs the dense interior
              point of csrc/lsc_general.hpp solves.  An infeasible agent keeps its last plan and the reset's slack set only grows, so every
              tick from 1 is recorded and judged
    modes_m4  a BVC slack mode and the reset at dt = 0.5, horizon = 2.0; it shares the modes family's file and conditions

Verdict of an agent's QP: 1 certified infeasible (phase-1 LP: minimal uniform violation of the rows > 1e-7), 0 optimal with this cost,
2 optimal with at most this cost (HiGHS stopped short of a feasible point with a lower objective), -1 no verdict (too close to call, HiGHS
gave up, or the corridor's seed box was blocked: status 4, no QP).

TEST INFRASTRUCTURE ONLY.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = {"corridor": "qp_pin_corridor.npz", "planar": "qp_pin_variants.npz", "m4": "qp_pin_variants.npz", "tp": "qp_pin_tp.npz",
         "obs": "qp_pin_obstacles.npz", "obs_m4": "qp_pin_obstacles.npz", "modes": "qp_pin_modes.npz", "modes_m4": "qp_pin_modes.npz"}
OBS_FAMILIES = ("obs", "obs_m4")
MISSION_KEYS = ("start", "goal", "world_min", "world_max", "radius", "downwash", "max_vel", "max_acc", "nominal_velocity")

# What the generator printed; both test files assert these counts on the committed arrays.
#            family: (certified infeasible, optimal incl. upper bounds, no verdict, optimal with x_ok false, status-4 agent-ticks)
COUNTS = {"corridor": (20, 291, 0, 0, 1), "planar": (79, 125, 0, 0, 0), "m4": (19, 165, 2, 0, 0), "tp": (0, 40, 0, 0, 0),
          "obs": (91, 609, 0, 0, 0), "obs_m4": (0, 128, 0, 0, 0), "modes": (71, 582, 3, 1, 0), "modes_m4": (0, 128, 0, 0, 0)}
# ... and what pin_variants.obs_conditions counts on the obs family's file (active: agent-ticks with an obstacle's row active at HiGHS's point)
OBS_COUNTS = {"infeasible": 91, "infeasible_pursuit": 34, "optimal_x_ok": 737, "no_verdict": 0, "judged": 828, "twice_infeasible_after_feasible": 17,
              "active": {"crossing": 56, "pursuit": 65, "crowd": 58, "crossing_m4": 59}}
# ... and what pin_variants.modes_conditions counts on the modes family's file, per scene: (agent-ticks judged, certified infeasible, optimal,
# no verdict, optimal with x_ok false, optimal with |f| >= 1e3, of those with x_ok, optimal with a positive slack variable at HiGHS's point)
MODES_COUNTS = {"bvc": (80, 5, 75, 0, 0, 0, 0, 0), "bvc_ncs2": (96, 64, 32, 0, 0, 0, 0, 0), "collision": (80, 1, 79, 0, 0, 1, 1, 75),
                "dynlimit": (80, 0, 79, 1, 1, 5, 4, 15), "reset": (112, 1, 111, 0, 0, 2, 2, 27), "crowd": (128, 0, 126, 2, 0, 1, 1, 25),
                "planar": (80, 0, 80, 0, 0, 1, 1, 76), "m4_collision": (64, 0, 64, 0, 0, 0, 0, 64), "m4_reset": (64, 0, 64, 0, 0, 1, 1, 17)}


def family_params(fam):
    """(M, dt, oracle parameters, PlannerConfig keywords) of a family."""
    if fam in ("obs_m4", "modes_m4"):
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


def tick_verdicts(O, H, fam, prm, ms, state, traj, tick, o, agents=None, active=None, qp_of=None, planar=None, x_atol=None, slack=None):
    """HiGHS on the QPs of one tick: (verdict int32 [N], cost [N], x float32 [N][dim][6 M], x_ok bool [N]); agents outside `agents`
    and status-4 agents get no verdict.  active (obs families): a bool [N] that is set where an obstacle's row is active at HiGHS's point.
    modes families: qp_of(a) assembles agent a's QP, planar says whether the world is, x_atol is the plan tolerance x_ok halves, and
    slack, a bool [N], is set where a slack variable is positive at HiGHS's point (slack_is_positive)."""
    from tolerances import ACTIVE_SET_TRAJ_ATOL as TRAJ_ATOL          # (TRAJ_ATOL, whatever LSC_SOLVER says)
    TRAJ_ATOL = TRAJ_ATOL if x_atol is None else x_atol
    M = family_params(fam)[0]
    n, dim = ms.qn, 2 if (fam == "planar" if planar is None else planar) else 3
    verdict = np.full(n, -1, np.int32)
    cost = np.zeros(n)
    xs = np.zeros((n, dim, 6 * M), np.float32)
    x_ok = np.zeros(n, bool)
    for a in (range(n) if agents is None else agents):
        if o["status"][a] == 4:
            continue
        qp = qp_of(a) if qp_of is not None else agent_qp(O, fam, prm, ms, a, state, traj, tick, o)
        v, c, x = highs_verdict(H, qp)
        verdict[a], cost[a] = v, c
        if x is not None and slack is not None:
            slack[a] = slack_is_positive(qp, x, c)
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


# ------------------------------------------------------------------------------------------------ the modes family: the alternate planner modes
MODES_FAMILIES = ("modes", "modes_m4")
# Mission names by family, in the order of the file's mission numbers.
MODES_SCENES = {"modes": ("bvc", "bvc_ncs2", "collision", "dynlimit", "reset", "crowd", "planar"), "modes_m4": ("m4_collision", "m4_reset")}
_BVC, _COLL, _DYN = dict(planner_mode="bvc"), dict(planner_mode="bvc", slack_mode="collision_constraint"), dict(planner_mode="bvc", slack_mode="dynamical_limit")
_RESET = dict(reset_threshold=0.15)
# cfg: the PlannerConfig keywords of the mode (modes_kw turns them into the oracle's).  events = {tick: [event]}, applied to the tick's
# input state before it is recorded: ("near", a, b, gap) puts agent a `gap` metres from agent b on the line between them -- closer than
# their buffered cells allow --, ("vel", a, v) gives agent a the velocity v (beyond max_vel = 1.0), ("acc", a, v) the acceleration v,
# ("gust", a, offset) moves agent a off its plan.  Picked on the CPU (pushes, seeds, tick counts) until the oracle and HiGHS alone met
# MODES_CONDITIONS.
MODES_PARAMS = {
    "bvc": dict(cfg=_BVC, n=8, circle=1.2, ticks=10, events={4: [("near", 0, 1, 0.22)], 7: [("vel", 5, (1.3, -0.4, 0.0))], 8: [("near", 3, 4, 0.22)]}),
    "bvc_ncs2": dict(cfg=dict(_BVC, n_constraint_segments=2), n=8, circle=1.2, ticks=12, events={}),
    "collision": dict(cfg=_COLL, n=8, circle=1.2, ticks=10, events={4: [("near", 0, 1, 0.22)], 7: [("vel", 5, (1.3, -0.4, 0.0))]}),
    "dynlimit": dict(cfg=_DYN, n=8, circle=1.2, ticks=10, events={4: [("near", 0, 1, 0.22)], 5: [("vel", 2, (-1.3, 0.5, 0.0))], 7: [("vel", 5, (1.3, -0.4, 0.0))],
                                                                  9: [("acc", 6, (3.0, -1.0, 0.0))]}),
    # gusts at ticks 5, 9 and 12 (the first four ticks are unflagged: every agent plans in plan_agent); the second and third come after the slack set has grown
    "reset": dict(cfg=_RESET, n=8, circle=1.2, ticks=14, events={5: [("gust", 3, (0.25, -0.2, 0.05))], 9: [("gust", 0, (-0.2, 0.25, 0.05)), ("vel", 6, (1.3, 0.3, 0.0))],
                                                                12: [("near", 2, 3, 0.22)]}),
    # 64 agents at random in an 8 x 8 x 2.5 m world: DYNAMICALLIMIT's slack switches the row pruning off, all 63 obstacles are kept
    "crowd": dict(cfg=_DYN, n=64, seed=11, ticks=2, events={2: [("vel", 7, (1.4, 0.2, 0.0))]}),
    "planar": dict(cfg=_COLL, n=8, circle=1.2, ticks=10, planar=True, events={4: [("near", 0, 1, 0.22)]}),
    "m4_collision": dict(cfg=_COLL, n=8, circle=1.5, ticks=8, events={3: [("near", 0, 1, 0.22)]}),
    "m4_reset": dict(cfg=_RESET, n=8, circle=1.5, ticks=8, events={3: [("gust", 3, (0.25, -0.2, 0.05))], 6: [("gust", 0, (-0.2, 0.25, 0.05))]}),
}
# What the family's fixture was made for (the issue's conditions); the generator and both test files assert them.  Per scene: at most
# max_no_verdict of its agent-ticks without a verdict, at most max_x_far of its optimal ones with x_ok false.
MODES_CONDITIONS = dict(min_infeasible=20, min_infeasible_bvc=3, min_infeasible_reset=1, min_large=3, min_large_x_ok=2, min_slack=10, min_slack_reset=5,
                        max_no_verdict=0.05, max_x_far=0.05)
LARGE_COST = 1e3            # tolerances.FUZZ_PLAN_COMPARED_BELOW_COST: the fuzzers compare no plan of a QP with |f| at or above it


def modes_scene_params(fam, name):
    """(M, dt, oracle parameter keywords, PlannerConfig keywords, the oracle's mode keywords, planar) of a scene of the modes families."""
    M, dt, okw, ckw = family_params(fam)
    p = MODES_PARAMS[name]
    planar = bool(p.get("planar"))
    if planar:
        okw, ckw = dict(okw, world_dimension=2, world_z_2d=1.0), dict(ckw, world_dimension=2, world_z_2d=1.0)
    cfg = p["cfg"]
    mkw = {}
    if cfg.get("planner_mode") == "bvc":
        mkw["planner"] = "bvc"
    if "slack_mode" in cfg:
        mkw["slack"] = cfg["slack_mode"]
    for k in ("n_constraint_segments", "reset_threshold"):
        if k in cfg:
            mkw[k] = cfg[k]
    return M, dt, okw, dict(ckw, **cfg), mkw, planar


def modes_scene(name):
    """(mission, {tick: [event]}, ticks flown) of a scene of the modes families."""
    import lsc_planner_amd as L
    p = MODES_PARAMS[name]
    if name == "crowd":
        n = p["n"]
        rng = np.random.default_rng(p["seed"])
        wmin, wmax = np.float32([-4, -4, 0]), np.float32([4, 4, 2.5])
        while True:
            start = rng.uniform(wmin + 0.3, wmax - 0.3, (n, 3)).astype(np.float32)
            gap = np.linalg.norm(start[:, None] - start[None], axis=2) + 9 * np.eye(n)
            if gap.min() > 0.45:
                break
        goal = rng.uniform(wmin + 0.3, wmax - 0.3, (n, 3)).astype(np.float32)
        ms = L.Mission(start, goal, wmin, wmax, np.full(n, 0.15), np.full(n, 2.0), np.full((n, 3), 1.0), np.full((n, 3), 2.0), np.full(n, 1.0))
    else:
        ms = L.circle_swap(p["n"], p["circle"], world=(-5, -5, 0, 5, 5, 2.5))
    return ms, p["events"], p["ticks"]


def apply_events(state, events):
    """The tick's events on its input state, in place."""
    for ev in events:
        if ev[0] == "near":
            _, a, b, gap = ev
            u = (state[a, :3] - state[b, :3]).astype(np.float64)
            state[a, :3] = (state[b, :3] + gap * u / np.linalg.norm(u)).astype(np.float32)
        elif ev[0] == "gust":
            state[ev[1], :3] += np.float32(ev[2])
        else:
            state[ev[1], {"vel": slice(3, 6), "acc": slice(6, 9)}[ev[0]]] = np.float32(ev[2])


def modes_swarm(O, fam, name, ms):
    """(params, modes, SwarmEx) of the scene's oracle.  Inside O.segments(M) of the family."""
    M, dt, okw, _, mkw, planar = modes_scene_params(fam, name)
    prm = O.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True, **okw)
    md = O.make_modes(**mkw)
    sw = O.SwarmEx(prm, md, ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
    if planar:
        sw.stale[:, 2, :] = np.float32(prm.world_z_2d)          # (as fly() does for the planar family)
    return prm, md, sw


def modes_tick(sw, ms, state, traj, tick, nthreads=8):
    """One tick of the scene's oracle: the disturbance checks, then the plans with their rows; the result carries the slack set the
    tick planned with."""
    sw.disturbance_update(state, traj, tick)
    o = sw.tick(state, ms.goal, traj, tick, want_lsc=True, nthreads=nthreads)
    o["slack_set"] = sw.slack_set.copy()
    return o


def fly_modes(O, fam, name, nthreads=8):
    """The oracle flies the scene from its start: (mission, params, modes, [(state, previous plans, result)] per tick)."""
    from lsc_planner_amd.planner import next_state_host
    M, dt, _, _, _, planar = modes_scene_params(fam, name)
    ms, events, ticks = modes_scene(name)
    prm, md, sw = modes_swarm(O, fam, name, ms)
    n = ms.qn
    state = np.zeros((n, 9), np.float32)
    state[:, :3] = ms.start
    traj = np.zeros((n, 3, 6 * M), np.float32)
    hist = []
    for tick in range(1, ticks + 1):
        apply_events(state, events.get(tick, ()))
        o = modes_tick(sw, ms, state, traj, tick, nthreads)
        hist.append((state.copy(), traj.copy(), o))
        traj = o["traj"]
        state = next_state_host(traj, dt=dt)
    return ms, prm, md, hist


def modes_agent_qp(O, fam, name, prm, md, ms, a, state, traj, tick, o):
    """QP of agent a on a tick's inputs, from the oracle's assembly with the tick's rows and slack set (as tests/fuzz_modes.py calls it):
    in BVC mode, and for an agent in a's slack set that is off its plan, the obstacle's prediction is its current position."""
    M, dt, _, cfg, mkw, planar = modes_scene_params(fam, name)
    n = ms.qn
    others = [j for j in range(n) if j != a]
    bvc = mkw.get("planner") == "bvc"
    thr = mkw.get("reset_threshold", 0.0)
    flags = o["slack_set"][a, others]
    obs = []
    for j in others:
        pred = O.shift_traj(traj[j]) if tick >= 2 else O.const_vel_traj(state[j, :3], state[j, 3:6], dt)
        moved = o["slack_set"][a, j] and np.linalg.norm(pred[:, 0] - state[j, :3]) > thr
        obs.append(np.repeat(state[j, :3, None], 6 * M, axis=1) if (bvc or moved) else pred)
    own = state[a]
    if planar:
        own = own.copy()
        own[2] = np.float32(prm.world_z_2d)
    return O.qp_assemble_ex(prm, md, own, ms.goal[a], float(ms.nominal_velocity[a]), ms.max_vel[a], ms.max_acc[a], np.array(obs, np.float32),
                            o["normal"][a], o["d"][a], slack_flags=flags)


def slack_is_positive(qp, x, cost):
    """Whether a slack variable is positive at the point x of a QP with optimum `cost`, against the slack's own scale: the slack
    variables' own terms of the objective -- the 1e5-weighted squares the modes add -- come to more than the cost comparison's bound
    COST_RTOL |f| + COST_ATOL.  A solver that held the slack variables at zero could not pass that comparison."""
    from tolerances import COST_ATOL, COST_RTOL
    xs = np.asarray(x)[qp.n_cp:]
    if xs.size == 0:
        return False
    own = 0.5 * xs @ qp.P[qp.n_cp:, qp.n_cp:] @ xs + qp.c[qp.n_cp:] @ xs
    return bool(own > COST_RTOL * abs(cost) + COST_ATOL)


def modes_tick_verdicts(O, H, fam, name, prm, md, ms, state, traj, tick, o, agents=None, slack=None):
    """tick_verdicts for a scene of the modes families: x_ok at half the interior point's plan tolerance (the tolerance of the half-second
    segments is the same number)."""
    from tolerances import FUZZ_TRAJ_ATOL_HALF_SECOND, INTERIOR_POINT_TRAJ_ATOL
    from tolerances import COST_ATOL
    planar = modes_scene_params(fam, name)[5]
    v, c, x, ok = tick_verdicts(O, H, fam, prm, ms, state, traj, tick, o, agents=agents, planar=planar, slack=slack,
                         x_atol=FUZZ_TRAJ_ATOL_HALF_SECOND if fam == "modes_m4" else INTERIOR_POINT_TRAJ_ATOL,
                         qp_of=lambda a: modes_agent_qp(O, fam, name, prm, md, ms, a, state, traj, tick, o))
    # An upper bound (verdict 2) is held from below at 1e-5 relative by every test.  Where HiGHS stopped shorter than that -- the oracle's
    # point satisfies the rows to 1e-9 at a cost more than 1e-5 relative below HiGHS's: seen on one 2 000-row QP of the crowd -- its
    # number pins nothing: no verdict.
    short = (v == 2) & (o["cost"] < c * (1 - 1e-5) - COST_ATOL)
    v[short], c[short], ok[short] = -1, 0.0, False
    x[short] = 0.0
    if slack is not None:
        slack[short] = False
    return v, c, x, ok


def modes_conditions(Z):
    """What MODES_CONDITIONS speaks of, counted on the arrays of the modes family's file (both of its families); per scene
    (agent-ticks judged, certified infeasible, optimal, no verdict, optimal with x_ok false, optimal with |f| >= LARGE_COST, of those with
    x_ok, optimal with a positive slack variable)."""
    got = {}
    for fam in MODES_FAMILIES:
        for i, name in enumerate(MODES_SCENES[fam]):
            v, ok, judged = Z[f"{fam}{i}_verdict"], Z[f"{fam}{i}_xok"], Z[f"{fam}{i}_judged"]
            opt = (v == 0) | (v == 2)
            large = opt & (np.abs(Z[f"{fam}{i}_cost"]) >= LARGE_COST)
            got[name] = (int(judged.sum()), int((v == 1).sum()), int(opt.sum()), int(((v < 0) & judged).sum()), int((opt & ~ok).sum()),
                         int(large.sum()), int((large & ok).sum()), int((opt & Z[f"{fam}{i}_slack"]).sum()))
    return got


def assert_modes_conditions(got):
    c = MODES_CONDITIONS
    assert set(got) == {n for names in MODES_SCENES.values() for n in names}, got
    assert sum(g[1] for g in got.values()) >= c["min_infeasible"] and got["bvc"][1] >= c["min_infeasible_bvc"], got
    assert got["reset"][1] + got["m4_reset"][1] >= c["min_infeasible_reset"], got
    assert sum(g[5] for g in got.values()) >= c["min_large"] and sum(g[6] for g in got.values()) >= c["min_large_x_ok"], got
    for name, g in got.items():
        assert g[3] <= c["max_no_verdict"] * g[0] and g[4] <= c["max_x_far"] * g[2], (name, g)
        cfg = MODES_PARAMS[name]["cfg"]
        if "slack_mode" in cfg and name != "crowd":
            assert g[7] >= c["min_slack"], (name, g)
    assert got["reset"][7] >= c["min_slack_reset"], got
