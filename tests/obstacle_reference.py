"""Reference tick of a swarm that plans against dynamic obstacles, composed per agent from what the oracle exports.

The oracle's own Swarm.tick knows cooperating agents only.  What the reference does with a non-agent obstacle
(ObstacleType::DYNAMICOBSTACLE) is three substitutions in the same sequence (src/traj_planner.cpp:829-864, 1336-1406):

    prediction   const_vel_traj(pos, vel) at EVERY planner_seq          (agents: shift_traj of the previous plan from planner_seq 2 on)
    rows         lsc_pair(init, obs, r_a, float32(r_o), 1.0, float32(dw_o))   -- with dw_a = 1.0 its (dw_a r_a + dw_o r_o) / (r_a + r_o)
                 is the non-agent rule (r_a + dw_o r_o) / (r_a + r_o) to the bit
    plan         qp_assemble(...).solve() over the other N - 1 agents followed by the K obstacles

Goal planning walks agents only (:553), so prior-based goals come from goal_prior_based over the agents; corridor boxes of an octomap
world are handed in (sfc=), taken from an agents-only tick.  The swarm keeps the optimiser's stale plans as Swarm does.
"""
import numpy as np


class ObstacleSwarm:
    def __init__(self, O, ms, obs_radius, obs_downwash, goal_mode="static", dt=0.2, use_sfc=False):
        self.O, self.ms, self.dt, self.goal_mode = O, ms, dt, goal_mode
        self.N = ms.qn
        self.prm = O.make_params(dt=dt, world_min=ms.world_min, world_max=ms.world_max, obs_f32=True, use_sfc=use_sfc)
        self.obs_radius = np.asarray(obs_radius, np.float64)
        self.obs_downwash = np.asarray([1.0 if d == 0 else d for d in np.asarray(obs_downwash, np.float64)])
        self.K = len(self.obs_radius)
        self.stale = np.zeros((self.N, 3, O.SEGV), np.float32)
        self.cost = np.zeros(self.N)

    def predictions(self, state, prev, seq):
        """Every agent's predicted / initial trajectory [N][3][SEGV]."""
        O = self.O
        if seq < 2:
            return np.stack([O.const_vel_traj(state[q, :3], state[q, 3:6], self.dt) for q in range(self.N)])
        return np.stack([O.shift_traj(prev[q]).reshape(3, O.SEGV) for q in range(self.N)])

    def tick(self, state, goal, prev_traj, seq, obs_pos, obs_vel, sfc=None, with_obstacles=True):
        """One tick of every agent.  obs_pos, obs_vel: float32 [K][3].  Returns dict(traj, cost, status, goal, normal, d) with
        normal [N][N-1+K][M][3] float32 and d [N][N-1+K][M][6] float64 in the product's order: the other agents by index, then the obstacles.
        with_obstacles=False: the same inputs planned against the agents alone (what the obstacles moved is the difference)."""
        O, N, ms = self.O, self.N, self.ms
        K = self.K if with_obstacles else 0
        state = np.ascontiguousarray(state, np.float32).reshape(N, 9)
        goal = np.ascontiguousarray(goal, np.float32).reshape(N, 3)
        prev = np.ascontiguousarray(prev_traj, np.float32).reshape(N, 3, O.SEGV)
        pred = self.predictions(state, prev, seq)
        obs_pred = [O.const_vel_traj(np.asarray(obs_pos[k], np.float32), np.asarray(obs_vel[k], np.float32), self.dt) for k in range(K)]
        if self.goal_mode == "prior_based" and sfc is None:
            cur_goal = O.goal_prior_based(state, goal, prev.reshape(N, -1), seq, dt=self.dt)
        else:
            cur_goal = goal
        n_obs = N - 1 + K
        out = np.zeros((N, 3, O.SEGV), np.float32)
        status = np.zeros(N, np.int32)
        normal = np.zeros((N, max(n_obs, 1), O.M, 3), np.float32)
        dd = np.zeros((N, max(n_obs, 1), O.M, O.NC))
        for qi in range(N):
            trajs, oi = [], 0
            for qj in range(N):
                if qj == qi:
                    continue
                normal[qi, oi], dd[qi, oi] = O.lsc_pair(pred[qi], pred[qj], ms.radius[qi], float(np.float32(ms.radius[qj])), ms.downwash[qi],
                                                        float(np.float32(ms.downwash[qj])))
                trajs.append(pred[qj]); oi += 1
            for k in range(K):
                normal[qi, oi], dd[qi, oi] = O.lsc_pair(pred[qi], obs_pred[k], ms.radius[qi], float(np.float32(self.obs_radius[k])), 1.0,
                                                        float(np.float32(self.obs_downwash[k])))
                trajs.append(obs_pred[k]); oi += 1
            obs_traj = np.stack(trajs) if trajs else np.zeros((0, 3, O.SEGV), np.float32)
            qp = O.qp_assemble(self.prm, state[qi], cur_goal[qi], ms.nominal_velocity[qi], ms.max_vel[qi], ms.max_acc[qi], obs_traj,
                               normal[qi, :n_obs], dd[qi, :n_obs], sfc=None if sfc is None else sfc[qi])
            st, x, cost, _, _ = qp.solve()
            status[qi] = st
            if st == 0:
                out[qi] = x.astype(np.float32).reshape(3, O.SEGV)
                if with_obstacles:
                    self.stale[qi] = out[qi]
                    self.cost[qi] = cost
            else:
                out[qi] = self.stale[qi]          # src/traj_planner.cpp:1553-1584: the optimiser's previous trajectory is kept
        return {"traj": out, "cost": self.cost.copy(), "status": status, "goal": np.asarray(cur_goal, np.float32), "normal": normal, "d": dd}


# the "hover" scenario: 8 agents swap across a circle while three slow spheres drift through its middle
HOVER_START = np.array([[-0.8, 0.5, 1.0], [0.6, 0.9, 1.3], [0.7, -0.9, 0.8]])
HOVER_VEL = np.array([[0.05, 0, 0], [0, -0.05, 0], [0, 0.05, 0]])
HOVER_RADIUS = np.array([0.25, 0.2, 0.3])
HOVER_DOWNWASH = np.array([1.0, 1.5, 2.0])
HOVER_TICKS = 50


def hover_mission():
    import lsc_planner_amd as L
    return L.circle_swap(8, circle_radius=3.0)


def hover_states(j, dt=0.2):
    """State of the obstacles at tick j (1-based): start + vel * dt (j - 1) in doubles, then float32."""
    return (HOVER_START + HOVER_VEL * (dt * (j - 1))).astype(np.float32), HOVER_VEL.astype(np.float32)


# a three-agent mission with one straight and one spin obstacle beside the agents' ways, for the simulator's tests
SIM_OBSTACLES = [
    {"type": "straight", "start": [0.9, 1.2, 1.0], "goal": [0.9, 2.2, 1.3], "size": 0.2, "speed": 0.05, "max_acc": 1.0, "downwash": 1.5},
    {"type": "spin", "axis_position": [-1.0, -1.3, 1.0], "axis_ori": [0.0, 0.0, 1.0], "start": [-0.6, -1.3, 1.0], "size": 0.25, "speed": 0.1,
     "max_acc": 1.0, "downwash": 0},
]


def sim_mission_doc(obstacles=SIM_OBSTACLES):
    # (no symmetry: a perfectly symmetric swap ties in the priority rule and the simulator's remedy draws random noise)
    agents = [{"type": "crazyflie", "start": [float(r * np.cos(a)), float(r * np.sin(a)), z], "goal": [float(-r * np.cos(a)), float(-r * np.sin(a)), 2.2 - z]}
              for a, r, z in ((0.1, 2.5, 1.0), (2.3, 2.2, 1.2), (4.0, 2.8, 0.9))]
    doc = {"quadrotors": {"crazyflie": {"max_vel": [1.0, 1.0, 1.0], "max_acc": [2.0, 2.0, 2.0], "radius": 0.15, "nominal_velocity": 1.0, "downwash": 2.0}},
           "world": [{"dimension": [-5, -5, 0, 5, 5, 2.5]}], "agents": agents}
    if obstacles is not None:
        doc["obstacles"] = obstacles
    return doc
