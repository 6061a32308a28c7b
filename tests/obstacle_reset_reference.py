"""Reference tick of a swarm that plans against dynamic obstacles WITH the disturbance reset (reset_threshold > 0), composed per agent
from what the oracle exports -- the oracle itself is untouched.

What the reference does with a non-agent obstacle once the checks are on (src/traj_planner.cpp):

    prediction   const_vel_traj(pos, vel) at every planner_seq (:838-846): obstaclePredictionCheck (:866-878) can never fire for it
    slack set    initialTrajPlanningCheck (:1047-1061) puts EVERY obstacle into obs_slack_indices when the agent itself is off its plan,
                 and the set only grows: sphere k is in agent qi's set from the first tick on which qi is off its plan -- ever[qi]
    margin       of a sphere in the set: obs_pred_sizes[oi][m][i] + agent.radius (:1395-1400), not half the separation; normal, downwash
                 of the pair and the anchor stay those of tests/obstacle_reference.py
    size         obstacleSizePredictionWithConstAcc (:880-919), restated in float64 below (obstacle_size)
    slack rows   M slack variables per obstacle of the set, agents and spheres alike (src/traj_optimizer.cpp:317-326, 455-456)

The agents' part is SwarmEx's: disturbance_update gives their sets and own_reset, a disturbed agent's prediction rests at its position,
lsc_pair is called as ObstacleSwarm calls it, qp_assemble_ex(..., slack_flags = agents' flags + K x ever_i).solve() plans, and an
infeasible agent keeps the optimiser's stale plan.
"""
import numpy as np

from obstacle_reference import HOVER_DOWNWASH, HOVER_RADIUS, hover_mission, hover_states      # noqa: F401  (the scene's parts)

DEG = 5


def uncertainty_segments(uncertainty_horizon, dt):
    """M_u = int((obs/uncertainty_horizon + SP_EPSILON) / dt), SP_EPSILON = 1e-9 (:882)."""
    return int((uncertainty_horizon + 1e-9) / dt)


def obstacle_size(r_o, max_acc, dt, M_u, size_prediction, m, i):
    """Predicted size at control point (m, i), every operation a correctly rounded float64 one in this order (Python floats):
    r_o + 0.5 a dt^2 (m^2 + 2 m i / n + i (i - 1) / (n (n - 1))) for m < M_u, r_o + 0.5 a (M_u dt)^2 from M_u on, r_o without size
    prediction."""
    r_o, max_acc, dt = float(r_o), float(max_acc), float(dt)
    if not size_prediction:
        return r_o
    half_a = 0.5 * max_acc
    if m >= M_u:
        T = float(M_u) * dt
        return r_o + half_a * (T * T)
    md, idd, n = float(m), float(i), float(DEG)
    poly = (md * md + (2.0 * md * idd) / n) + (idd * (idd - 1.0)) / (n * (n - 1.0))
    return r_o + (half_a * (dt * dt)) * poly


def size_table(radius, max_acc, dt, M, size_prediction=True, uncertainty_horizon=1.0):
    """[K][M][6] float64 from the float32 radii the rows use."""
    M_u = uncertainty_segments(uncertainty_horizon, dt)
    assert M_u <= M
    return np.array([[[obstacle_size(float(np.float32(r)), a, dt, M_u, size_prediction, m, i) for i in range(DEG + 1)] for m in range(M)]
                     for r, a in zip(radius, max_acc)]).reshape(len(radius), M, DEG + 1)


class ObstacleResetSwarm:
    """margins: "rule" the reference's; "half" a sphere in the slack set keeps the half-separation margin; "no_growth" it takes
    r_o + r_a (the two wrong kernels the tests must be able to see)."""

    def __init__(self, O, ms, obs_radius, obs_downwash, max_acc, size_prediction=True, uncertainty_horizon=1.0, reset_threshold=0.15, dt=0.2):
        self.O, self.ms, self.dt = O, ms, dt
        self.N = ms.qn
        self.prm = O.make_params(dt=dt, world_min=ms.world_min, world_max=ms.world_max, obs_f32=True)
        self.modes = O.make_modes(reset_threshold=reset_threshold)
        self.sw = O.SwarmEx(self.prm, self.modes, ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
        self.obs_radius = np.asarray(obs_radius, np.float64)
        self.obs_downwash = np.asarray([1.0 if d == 0 else d for d in np.asarray(obs_downwash, np.float64)])
        self.K = len(self.obs_radius)
        self.size = size_table(self.obs_radius, np.broadcast_to(np.asarray(max_acc, np.float64), (self.K,)), dt, O.M, size_prediction, uncertainty_horizon)
        self.plain = size_table(self.obs_radius, np.zeros(self.K), dt, O.M, False, 0.0)
        self.ever = np.zeros(self.N, bool)
        self.stale = np.zeros((self.N, 3, O.SEGV), np.float32)
        self.cost = np.zeros(self.N)

    def tick(self, state, goal, prev_traj, seq, obs_pos, obs_vel, margins="rule", commit=True):
        """One tick of every agent.  Returns dict(traj, cost, status, goal, normal, d, own, ever, alt, slack_min): normal / d as
        ObstacleSwarm's; own [N] the agents found off their plans now; ever [N]; alt [N] whether the agent's QP carried a slack variable;
        slack_min [N] its smallest slack variable (0 without).  commit=False leaves the persistent state (ever, stale, cost) alone."""
        O, N, K, ms = self.O, self.N, self.K, self.ms
        state = np.ascontiguousarray(state, np.float32).reshape(N, 9)
        goal = np.ascontiguousarray(goal, np.float32).reshape(N, 3)
        prev = np.ascontiguousarray(prev_traj, np.float32).reshape(N, 3, O.SEGV)
        own = self.sw.disturbance_update(state, prev, seq).astype(bool)          # (idempotent: the sets only grow, by the same test)
        ever = self.ever | own
        pred = []
        for q in range(N):
            if own[q]:
                pred.append(np.repeat(state[q, :3, None], O.SEGV, axis=1).astype(np.float32))      # reset: at rest at its position
            elif seq < 2:
                pred.append(O.const_vel_traj(state[q, :3], state[q, 3:6], self.dt))
            else:
                pred.append(O.shift_traj(prev[q]).reshape(3, O.SEGV))
        obs_pred = [O.const_vel_traj(np.asarray(obs_pos[k], np.float32), np.asarray(obs_vel[k], np.float32), self.dt) for k in range(K)]
        n_obs = N - 1 + K
        out = np.zeros((N, 3, O.SEGV), np.float32)
        status = np.zeros(N, np.int32)
        cost = self.cost.copy()
        stale = self.stale.copy()
        normal = np.zeros((N, n_obs, O.M, 3), np.float32)
        dd = np.zeros((N, n_obs, O.M, O.NC))
        alt, slack_min = np.zeros(N, bool), np.zeros(N)
        for qi in range(N):
            trajs, flags, oi = [], [], 0
            for qj in range(N):
                if qj == qi:
                    continue
                normal[qi, oi], dd[qi, oi] = O.lsc_pair(pred[qi], pred[qj], ms.radius[qi], float(np.float32(ms.radius[qj])), ms.downwash[qi],
                                                        float(np.float32(ms.downwash[qj])))
                trajs.append(pred[qj]); flags.append(int(self.sw.slack_set[qi, qj])); oi += 1
            for k in range(K):
                normal[qi, oi], dd[qi, oi] = O.lsc_pair(pred[qi], obs_pred[k], ms.radius[qi], float(np.float32(self.obs_radius[k])), 1.0,
                                                        float(np.float32(self.obs_downwash[k])))
                if ever[qi] and margins != "half":
                    dd[qi, oi] = (self.size if margins == "rule" else self.plain)[k] + float(ms.radius[qi])
                trajs.append(obs_pred[k]); flags.append(int(ever[qi])); oi += 1
            qp = O.qp_assemble_ex(self.prm, self.modes, state[qi], goal[qi], ms.nominal_velocity[qi], ms.max_vel[qi], ms.max_acc[qi],
                                  np.stack(trajs), normal[qi], dd[qi], slack_flags=np.array(flags, np.uint8))
            st, x, c, _, _ = qp.solve()
            status[qi] = st
            alt[qi] = qp.nv > qp.n_cp
            if st == 0:
                out[qi] = x[:qp.n_cp].astype(np.float32).reshape(3, O.SEGV)
                stale[qi] = out[qi]; cost[qi] = c
                slack_min[qi] = x[qp.n_cp:].min(initial=0.0)
            else:
                out[qi] = stale[qi]              # src/traj_planner.cpp:1553-1584: the optimiser's previous trajectory is kept
        if commit:
            self.ever, self.stale, self.cost = ever, stale, cost
        return {"traj": out, "cost": cost.copy(), "status": status, "goal": goal.copy(), "normal": normal, "d": dd, "own": own, "ever": ever.copy(),
                "alt": alt, "slack_min": slack_min}


# ---- the scene "pushed hover": hover_mission() with its three spheres, agent 2 moved by +0.3 m in x in front of tick 12
PUSHED_MAX_ACC = np.array([1.0, 0.5, 2.0])
PUSHED_TICKS, PUSHED_TICK, PUSHED_AGENT, PUSHED_BY = 20, 12, 2, (0.3, 0.0, 0.0)
PUSHED_THRESHOLD = 0.15


def fly_reference(ref, ms, ticks, states_of, gusts, dt=0.2, variants=(), variant_ticks=None):
    """The reference alone in closed loop, static goals: a list of per-tick dicts (the tick's result + its inputs state / traj_in / pos /
    vel).  states_of(tick) -> (pos, vel) float32 [K][3]; gusts = {tick: (agent, offset)}.  variants: margin rules ("half", "no_growth")
    the same inputs are planned with as well, in front of the tick and without touching the persistent state, on variant_ticks (None:
    every tick with a flagged agent); their plans and statuses go into the tick's dict as traj_<rule>, status_<rule>."""
    from lsc_planner_amd.planner import next_state_host
    O = ref.O
    state = np.zeros((ms.qn, 9), np.float32); state[:, :3] = ms.start
    traj = np.zeros((ms.qn, 3, O.SEGV), np.float32)
    flight = []
    for tick in range(1, ticks + 1):
        if tick in gusts:
            q, off = gusts[tick]
            state[q, :3] += np.asarray(off, np.float32)
        pos, vel = states_of(tick)
        extra = {}
        for rule in variants:
            v = ref.tick(state, ms.goal, traj, tick, pos, vel, margins=rule, commit=False)
            if (variant_ticks is None and v["ever"].any()) or (variant_ticks is not None and tick in variant_ticks):
                extra["traj_" + rule], extra["status_" + rule] = v["traj"], v["status"]
        r = ref.tick(state, ms.goal, traj, tick, pos, vel)
        r.update(state=state.copy(), traj_in=traj.copy(), pos=pos, vel=vel, **extra)
        flight.append(r)
        traj = r["traj"]
        state = next_state_host(traj, dt=dt)
    return flight


def scene_is_telling(flight, min_move=1e-3):
    """What a generated scene must show, on the reference alone (flown with variants=("half",)): at most a quarter of the agent-ticks
    infeasible, and at least one sphere's full-margin row moving a plan by more than min_move against the same inputs planned with the
    half-separation margins.  Returns that largest distance."""
    status = np.stack([t["status"] for t in flight])
    assert (status != 0).sum() * 4 <= status.size, (status != 0).sum()
    moved = 0.0
    for t in flight:
        if "traj_half" not in t:
            continue
        ok = (t["status_half"] == 0) & (t["status"] == 0) & t["ever"]
        if ok.any():
            moved = max(moved, float(np.abs(t["traj_half"] - t["traj"])[ok].max()))
    assert moved > min_move, moved
    return moved


# ---- the two generated scenes of the GPU tests; scene_is_telling holds each on the reference alone (tests/test_obstacle_reset.py)
# the hover circle through the M = 4 build: dt 0.5, horizon 2.0, uncertainty horizon 1.0 (M_u = 2), the push in front of tick 4
M4_DT, M4_TICKS, M4_PUSH_TICK = 0.5, 8, 4
# the obs family's crowd (tests/pin_variants.py: 12 agents, 54 spheres, 65 obstacles per agent), max_acc 1.0, agent 0 pushed in front of tick 3
CROWD_TICKS, CROWD_PUSH_TICK, CROWD_AGENT, CROWD_MAX_ACC = 5, 3, 0, 1.0


def crowd_scene():
    """(mission, radius [54], downwash [54], states_of(tick)) of the crowd."""
    from lsc_planner_amd.obstacles import ObstacleSet
    from pin_variants import obs_scene
    ms, obstacles, _ = obs_scene("crowd")
    oset = ObstacleSet(obstacles, n_agents=ms.qn)
    return ms, oset.radius, oset.downwash, lambda tick: oset.at(0.2 * (tick - 1))
