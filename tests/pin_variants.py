"""What the HiGHS pins of the QP variants share (tests/golden/make_qp_pin_variants.py writes the fixtures, tests/test_oracle_pin_variants.py
and tests/test_gpu_highs_variants.py read them): the four families, how the oracle flies one of their missions, how one agent's QP of a
recorded tick is assembled and what HiGHS (tests/highs_qp.py) says about it.

Families -- each a way of building or solving an agent's QP that the 90-variable empty-map pins (tests/golden/qp_pin_ticks.npz) never reach:
    corridor  M = 5, 3-D, use_sfc on the forest map: six box half-spaces per segment; the boxes have a history, so every tick is recorded
    planar    world_dimension = 2, world_z_2d = 1.0: the 60-variable QP; every kept tick is replayed on its own
    m4        dt = 0.5, horizon = 2.0: the 72-variable QP of the four-segment build; every kept tick is replayed on its own
    tp        one tick of the 320-agent swarm of tests/test_gpu_round2.py::test_throughput_build_agrees_with_the_latency_build

Verdict of an agent's QP: 1 certified infeasible (phase-1 LP: minimal uniform violation of the rows > 1e-7), 0 optimal with this cost,
2 optimal with at most this cost (HiGHS stopped short of a feasible point with a lower objective), -1 no verdict (too close to call, HiGHS
gave up, or the corridor's seed box was blocked: status 4, no QP).

TEST INFRASTRUCTURE ONLY.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = {"corridor": "qp_pin_corridor.npz", "planar": "qp_pin_variants.npz", "m4": "qp_pin_variants.npz", "tp": "qp_pin_tp.npz"}
MISSION_KEYS = ("start", "goal", "world_min", "world_max", "radius", "downwash", "max_vel", "max_acc", "nominal_velocity")

# What the generator printed; both test files assert these counts on the committed arrays.
#            family: (certified infeasible, optimal incl. upper bounds, no verdict, optimal with x_ok false, status-4 agent-ticks)
COUNTS = {"corridor": (20, 291, 0, 0, 1), "planar": (79, 125, 0, 0, 0), "m4": (19, 165, 2, 0, 0), "tp": (0, 40, 0, 0, 0)}


def family_params(fam):
    """(M, dt, oracle parameters, PlannerConfig keywords) of a family."""
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


def fly(O, fam, ms, ticks, dm=None, nthreads=8):
    """The oracle flies the mission from its start: per tick (state, previous plans, the oracle's result with its LSC dump)."""
    from lsc_planner_amd.planner import next_state_host
    M, dt, _, _ = family_params(fam)
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


def tick_verdicts(O, H, fam, prm, ms, state, traj, tick, o, agents=None):
    """HiGHS on the QPs of one tick: (verdict int32 [N], cost [N], x float32 [N][dim][6 M], x_ok bool [N]); agents outside `agents`
    and status-4 agents get no verdict."""
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
        v, c, x = highs_verdict(H, agent_qp(O, fam, prm, ms, a, state, traj, tick, o))
        verdict[a], cost[a] = v, c
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
    if fam == "corridor":
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
