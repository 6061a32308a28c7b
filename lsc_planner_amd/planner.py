"""Host-side mirror of the reference's per-agent planner surface, batched over the swarm.

The reference drives N TrajPlanner objects sequentially (src/multi_sync_simulator.cpp:320-328); each owns a
TrajOptimizer (include/traj_optimizer.hpp:20-28).  SwarmPlanner keeps the same vocabulary --
set_current_state / set_obs_prev_trajs / plan / get_traj / get_qp_cost / get_planning_report -- but one
`plan()` is one C-ABI call for all agents (include/lsc_planner_amd.h).
"""
import ctypes
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import LscConfig, LscError, M, NC, NV, SEGV


@dataclass
class PlannerConfig:
    dt: float = 0.2                  # traj/dt
    control_input_weight: float = 0.01
    terminal_weight: float = 1.0
    use_octomap: bool = False
    world_resolution: float = 0.1
    device: int = 0
    max_rows_per_cp: int = 0
    max_iters: int = 50
    prune: bool = True
    warm_start_mu: float = 0.03    # 0 = cold (Mehrotra) start only
    goal_mode: str = "static"       # mode/goal: "static", "prior_based" (the goal input is the desired goal) or "right_hand" (the goal stage
                                    # moves a deadlocked agent's goal to its right; the tick behind it plans as "static")
    deadlock_seq_threshold: int = 5         # right_hand: isDeadlock's thresholds (src/param.cpp:79-80)
    deadlock_velocity_threshold: float = 0.1
    goal_threshold: float = 0.1
    priority_dist_threshold: float = 0.4
    goal_radius: float = 2.0
    grid_resolution: float = 0.3    # grid/resolution (goal planner's search grid; goal_mode prior_based + use_octomap)
    grid_margin: float = 0.2        # grid/margin
    horizon: float = 1.0            # traj/horizon; M = horizon / dt: 5 (liblsc_hip.so) or 4 (liblsc_hip_m4.so)
    goal_row_cap: int = 0           # > 0: smaller OPEN-row capacity of the goal search (tests of the overflow path)
    planner_mode: str = "lsc"       # mode/planner: "lsc" or "bvc"
    slack_mode: str = "none"        # SlackMode: "none", "dynamical_limit", "collision_constraint"
    slack_collision_weight: float = 100000.0
    n_constraint_segments: int = -1
    reset_threshold: float = 0.0    # multisim/reset_threshold; > 0 switches the disturbance checks on (launch files: 0.15)
    gap_tolerance: float = 1e-9     # interior point: relative duality gap at the optimum
    world_dimension: int = 3        # world/dimension: 2 = planar goal grid at z = world_z_2d
    world_z_2d: float = 1.0         # world/z_2d
    goal_search: str = "auto"      # goal planner's grid search: "auto" (register-resident, 32-bit keys when their table fits), "general", "key64" (register-resident, the double as key), "hbm" (OPEN rows in HBM; grids too large for LDS take it anyway)
    goal_lds_row_cap: int = 0       # > 0: smaller LDS OPEN-row capacity of the goal search; an overflowing row restarts the search in HBM (tests of the restart)
    # QP solver of the LSC fast path: "active_set" (dual active set first, interior point as fallback: the library's default) or
    # "interior_point" (the interior point alone, rounds 1-4).  LSC_SOLVER in the environment changes the default of this harness, so that
    # whole test files can be run through the other solver (tests/test_gpu_round5.py).
    solver: str = field(default_factory=lambda: os.environ.get("LSC_SOLVER", "active_set"))
    comm: tuple = None              # (world_size, rank, id bytes from comm_unique_id()): agent-sharded multi-GPU over RCCL


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


class SwarmPlanner:
    """All agents' TrajPlanner + TrajOptimizer state behind one context of liblsc_hip.so."""

    def __init__(self, mission, config=None):
        self.cfg = config or PlannerConfig()
        # M = horizon / dt picks the library (the kernels are unrolled for their segment count): 5 -> liblsc_hip.so, 4 -> liblsc_hip_m4.so
        self.M = _lib.segments_of(self.cfg.horizon, self.cfg.dt)
        self.SEGV, self.NV = NC * self.M, 3 * NC * self.M
        if self.M not in _lib.BUILT_SEGMENTS:
            raise LscError(f"horizon / dt = {self.cfg.horizon} / {self.cfg.dt} gives M = {self.M} segments; libraries are built for M in "
                           f"{_lib.BUILT_SEGMENTS} (the segment count is a build parameter: make LSC_SEGMENTS=k, src/traj_optimizer.cpp:9 "
                           "computes it at run time)")
        self.L = _lib.load_library(self.M)
        self.mission = mission
        c = LscConfig()
        self.L.lsc_default_config(ctypes.byref(c))
        c.dt, c.control_weight, c.terminal_weight = self.cfg.dt, self.cfg.control_input_weight, self.cfg.terminal_weight
        for k in range(3):
            c.world_min[k] = float(mission.world_min[k])
            c.world_max[k] = float(mission.world_max[k])
        c.use_octomap = int(self.cfg.use_octomap)
        c.world_resolution = self.cfg.world_resolution
        c.device = self.cfg.device
        c.max_rows_per_cp = self.cfg.max_rows_per_cp
        c.max_iters = self.cfg.max_iters
        c.prune = int(self.cfg.prune)           # bool or the ABI's 0..3
        c.warm_start_mu = float(self.cfg.warm_start_mu)
        c.goal_mode = {"static": 0, "prior_based": 1, "right_hand": 0}[self.cfg.goal_mode]      # (right_hand: lsc_set_goal_rule below)
        c.goal_threshold, c.priority_dist_threshold, c.goal_radius = (self.cfg.goal_threshold, self.cfg.priority_dist_threshold,
                                                                       self.cfg.goal_radius)
        c.grid_resolution, c.grid_margin = self.cfg.grid_resolution, self.cfg.grid_margin
        c.horizon, c.goal_row_cap = self.cfg.horizon, self.cfg.goal_row_cap
        c.planner_mode = {"lsc": 0, "bvc": 1}[self.cfg.planner_mode]
        c.slack_mode = {"none": 0, "dynamical_limit": 1, "collision_constraint": 2}[self.cfg.slack_mode]
        c.slack_collision_weight, c.n_constraint_segments = self.cfg.slack_collision_weight, self.cfg.n_constraint_segments
        c.reset_threshold = self.cfg.reset_threshold
        c.gap_tolerance = self.cfg.gap_tolerance
        c.world_dimension, c.world_z_2d = int(self.cfg.world_dimension), float(self.cfg.world_z_2d)
        c.goal_search = {"auto": 0, "general": 1, "key64": 2, "hbm": 3}[self.cfg.goal_search]
        c.goal_lds_row_cap = self.cfg.goal_lds_row_cap
        c.solver = {"active_set": 1, "interior_point": 0, "hand_over": 2}[self.cfg.solver]      # (hand_over: test mode, see lsc_config.solver)
        self._c = c
        self.ctx = self.L.lsc_create(ctypes.byref(c))
        if not self.ctx:
            raise LscError("lsc_create failed: no usable gfx950 device (there is no CPU fallback)")
        self.N = mission.qn
        self.K = 0                   # dynamic obstacles (set_obstacles)
        if self.cfg.goal_mode == "right_hand":
            self._check(self.L.lsc_set_goal_rule(self.ctx, _lib.GOAL_RULE_RIGHT_HAND, int(self.cfg.deadlock_seq_threshold),
                                                 float(self.cfg.deadlock_velocity_threshold)))
        if self.cfg.comm is not None:
            world, rank, token = self.cfg.comm
            buf = (ctypes.c_ubyte * _lib.COMM_ID_BYTES).from_buffer_copy(bytes(token))
            self._check(self.L.lsc_comm_init(self.ctx, int(world), int(rank), buf))
        self._check(self.L.lsc_set_agents(self.ctx, self.N, _dp(np.ascontiguousarray(mission.radius, np.float64)),
                                          _dp(np.ascontiguousarray(mission.downwash, np.float64)),
                                          _dp(np.ascontiguousarray(mission.max_vel, np.float64)),
                                          _dp(np.ascontiguousarray(mission.max_acc, np.float64)),
                                          _dp(np.ascontiguousarray(mission.nominal_velocity, np.float64))))
        w, r, sr, tr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self.L.lsc_comm_info(self.ctx, ctypes.byref(w), ctypes.byref(r), ctypes.byref(sr), ctypes.byref(tr)))
        self.world, self.rank, self.shard_rows, self.table_rows = w.value, r.value, sr.value, tr.value
        self.first = min(self.rank * self.shard_rows, self.N)
        self.count = min(self.shard_rows, self.N - self.first)
        # TrajPlanner state (src/traj_planner.cpp:41-48)
        self.planner_seq = 0
        self.traj_curr = np.zeros((self.N, 3, self.SEGV), np.float32)
        self.qp_cost = np.zeros(self.N)
        self.planning_report = np.zeros(self.N, np.int32)
        self.iters = np.zeros(self.N, np.int32)

    def _check(self, rc):
        if rc != 0:
            raise LscError(f"lsc error {rc}: {self.L.lsc_last_error(self.ctx).decode()}")

    def note(self):
        """Informational remarks of the context (lsc_last_note): fixed-up modes, the goal planner's search, which LSC build phase B takes."""
        return self.L.lsc_last_note(self.ctx).decode()

    def close(self):
        if getattr(self, "ctx", None):
            self.L.lsc_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- TrajPlanner::setDistMap --------------------------------------------------------------------------
    def set_distmap(self, dist, key_min, res):
        """dist: float32 [nx][ny][nz] metres (DynamicEDTOctomap semantics), key_min: octomap key of cell (0,0,0)."""
        dist = np.ascontiguousarray(dist, np.float32)
        km = np.ascontiguousarray(key_min, np.int32)
        self._check(self.L.lsc_set_distmap(self.ctx, _fp(dist), dist.shape[0], dist.shape[1], dist.shape[2], _ip(km), float(res)))

    def load_octomap(self, bt_path, maxdist=1.0, on_device=False):
        """MultiSyncSimulator::setOctomap (src/multi_sync_simulator.cpp:153-167): .bt -> distance field -> every agent.
        on_device: .bt -> occupancy -> the device builds the field and everything derived from it (set_occupancy), and map_update
        changes it between ticks; returns (occupancy, key_min, res) then."""
        if on_device:
            occ, key_min, res = occupancy_from_bt(bt_path, self.mission.world_min, self.mission.world_max)
            self.set_occupancy(occ, key_min, res, maxdist)
            return occ, key_min, res
        dist, key_min, res = edt_from_bt(bt_path, self.mission.world_min, self.mission.world_max, maxdist)
        self.set_distmap(dist, key_min, res)
        return dist, key_min, res

    # ---- the map from occupancy, built and changed on the device (lsc_map.hip) ------------------------------------
    def set_occupancy(self, occ, key_min, res, maxdist=1.0):
        """occ: [nx][ny][nz], non-zero = occupied; key_min: octomap key of cell (0,0,0).  The distance field of edt_from_bt(maxdist), the
        corridor kernel's integral images and the goal planner's occupancy are built from it on the device (lsc_set_occupancy)."""
        occ = np.ascontiguousarray(np.asarray(occ) != 0, np.uint8)
        if occ.ndim != 3:
            raise LscError(f"set_occupancy: the grid has {occ.ndim} dimensions, not 3")
        km = np.ascontiguousarray(key_min, np.int32)
        self._check(self.L.lsc_set_occupancy(self.ctx, occ.ctypes.data, occ.shape[0], occ.shape[1], occ.shape[2], _ip(km), float(res), float(maxdist)))

    def map_update(self, boxes, values=None, regrow=False, stream=None):
        """Changes the map between two ticks (lsc_map_update): boxes int [n][6] of field cells (x0, y0, z0, x1, y1, z1; lo inclusive, hi
        exclusive), values [n] of 0 (free) / 1 (occupied), applied in order.  Or `boxes` is a torch uint8 tensor [nx][ny][nz] on the
        device: the whole grid (lsc_map_update_device).  The rebuild is enqueued on `stream` (None: the context's own) and not waited for.
        regrow: every agent regrows its corridor from its current position at the next tick."""
        flags = _lib.MAP_REGROW_CORRIDORS if regrow else 0
        st = None if not stream else int(stream)
        if hasattr(boxes, "data_ptr"):
            nx, ny, nz = (int(v) for v in self.map_dims()[:3])
            if str(boxes.dtype) != "torch.uint8" or tuple(boxes.shape) != (nx, ny, nz) or not boxes.is_contiguous() or not boxes.is_cuda:
                raise LscError(f"map_update: the grid must be a contiguous uint8 device tensor of shape {(nx, ny, nz)}")
            self._check(self.L.lsc_map_update_device(self.ctx, boxes.data_ptr(), flags, st))
            return
        if values is None:
            raise LscError("map_update: boxes need values (0 free / 1 occupied, one per box); only a whole device grid goes without")
        b = np.ascontiguousarray(boxes, np.int32)
        if b.size % 6:
            raise LscError(f"map_update: boxes must be [n][6] (x0, y0, z0, x1, y1, z1), got shape {b.shape}")
        b = b.reshape(-1, 6)
        v = np.ascontiguousarray(values, np.uint8).ravel()
        if len(v) != len(b):
            raise LscError(f"map_update: {len(b)} boxes, {len(v)} values")
        self._check(self.L.lsc_map_update(self.ctx, len(b), _ip(b), v.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), flags, st))

    def map_dims(self):
        """lsc_map_read(LSC_MAP_DIMS): nx, ny, nz, n_radii, H, W, A, 1 when the map is a device occupancy."""
        d = np.zeros(_lib.MAP_DIMS_INTS, np.int32)
        self._check(self.L.lsc_map_read(self.ctx, _lib.MAP_DIMS, d.ctypes.data, d.nbytes))
        return d

    def map_read(self):
        """The map as the kernels read it (lsc_map_read; diagnostics, synchronises): dict(edt float32 [nx][ny][nz], integral int32
        [n_radii][nx+1][ny+1][nz+1], goal_occupancy uint8 [n_radii][A][H][W] (index H W k + W i + j), occupancy uint8 [nx][ny][nz] or
        None on a map from set_distmap, dims)."""
        d = self.map_dims()
        nx, ny, nz, R, H, W, A, dev = (int(v) for v in d)
        out = {"dims": d, "occupancy": np.zeros((nx, ny, nz), np.uint8) if dev else None, "edt": np.zeros((nx, ny, nz), np.float32),
               "integral": np.zeros((R, nx + 1, ny + 1, nz + 1), np.int32), "goal_occupancy": np.zeros((R, A, H, W), np.uint8)}
        for which, key in ((_lib.MAP_OCCUPANCY, "occupancy"), (_lib.MAP_EDT, "edt"), (_lib.MAP_INTEGRAL, "integral"),
                           (_lib.MAP_GOAL_OCCUPANCY, "goal_occupancy")):
            if out[key] is not None and out[key].nbytes:
                self._check(self.L.lsc_map_read(self.ctx, which, out[key].ctypes.data, out[key].nbytes))
        return out

    def set_shard(self, first, count):
        self._check(self.L.lsc_set_shard(self.ctx, first, count))
        self.first, self.count = first, count

    # ---- TrajPlanner::setObstacles for the mission's dynamic obstacles ---------------------------------------
    def set_obstacles(self, radius, downwash=None, max_acc=None, size_prediction=True, uncertainty_horizon=1.0):
        """K non-cooperating moving spheres behind the other agents in every agent's obstacle list (lsc_set_obstacles); radius,
        downwash [K] (downwash 0 or None: 1).  An empty list removes them.  Their states come through obstacle_states().
        With max_acc [K] (the obstacles' acceleration bound) they go through lsc_set_obstacles_ex, which also serves a context with
        reset_threshold > 0: an agent that was ever off its plan then keeps the sphere's whole predicted size as its margin
        (obs/size_prediction, obs/uncertainty_horizon of the reference's parameters)."""
        r = np.ascontiguousarray(radius, np.float64).ravel()
        dw = np.ones(len(r)) if downwash is None else np.ascontiguousarray(downwash, np.float64).ravel()
        if len(dw) != len(r):
            raise LscError(f"set_obstacles: {len(r)} radii, {len(dw)} downwash values")
        if max_acc is not None:
            ma = np.full(len(r), float(max_acc)) if np.ndim(max_acc) == 0 else np.ascontiguousarray(max_acc, np.float64).ravel()
            if len(ma) != len(r):
                raise LscError(f"set_obstacles: {len(r)} radii, {len(ma)} max_acc values")
            self._check(self.L.lsc_set_obstacles_ex(self.ctx, len(r), _dp(r) if len(r) else None, _dp(dw) if len(r) else None,
                                                    _dp(ma) if len(r) else None, 1 if size_prediction else 0, float(uncertainty_horizon)))
        else:
            self._check(self.L.lsc_set_obstacles(self.ctx, len(r), _dp(r) if len(r) else None, _dp(dw) if len(r) else None))
        self.K = len(r)
        self._obstacle_states = None

    def obstacle_states(self, pos, vel=None):
        """Position and velocity of every obstacle for the next ticks.  Host form: pos, vel [K][3] (any float arrays; read as float32)
        -- the next tick uploads them.  Device form: pos is a torch float32 tensor [K][6] (position | velocity) on the context's
        device -- the ticks read it where it lies, and the caller orders its writes on the tick's stream."""
        K = getattr(self, "K", 0)
        if vel is None and hasattr(pos, "data_ptr"):
            if pos.numel() != 6 * K or str(pos.dtype) != "torch.float32" or not pos.is_contiguous():
                raise LscError(f"obstacle_states: the device form takes a contiguous float32 tensor [{K}][6]")
            self._check(self.L.lsc_obstacle_states_device(self.ctx, pos.data_ptr()))
            self._obstacle_states = pos              # (kept alive: the ticks read it)
            return
        pv = np.ascontiguousarray(np.concatenate([np.asarray(pos, np.float32).reshape(-1, 3), np.asarray(vel, np.float32).reshape(-1, 3)], axis=1))
        if len(pv) != K and K > 0:
            raise LscError(f"obstacle_states: {len(pv)} states for {K} obstacles")
        self._check(self.L.lsc_obstacle_states(self.ctx, _fp(pv)))
        self._obstacle_states = None

    # ---- motion models: the context moves its obstacles itself (lsc_obstacle_motion, csrc/lsc_obstacles.hip) -----
    def set_obstacle_motion(self, obstacles):
        """Installs the motion models of the mission's obstacles: an ObstacleSet, a mission's "obstacles" list (dicts), or a list of
        (kind, speed, points) as ObstacleSet.models() returns it.  Radius and downwash are set too (set_obstacles) when the argument
        carries them and the context has no obstacles yet.  An empty list or None removes the models.  Every tick then evaluates the
        models at the clock's time (obstacle_clock) in a launch of its own in front of everything else."""
        from .obstacles import ObstacleSet
        if obstacles is None or len(obstacles) == 0:
            if getattr(self, "K", 0) > 0:
                self._check(self.L.lsc_obstacle_motion(self.ctx, 0, None))
            return
        if not isinstance(obstacles, ObstacleSet) and isinstance(obstacles[0], dict):
            obstacles = ObstacleSet(obstacles, n_agents=self.N)
        chasers, walkers = [], []
        if isinstance(obstacles, ObstacleSet):
            if getattr(self, "K", 0) == 0:
                self.set_obstacles(obstacles.radius, obstacles.downwash)
            chasers, walkers = obstacles.chasers(), obstacles.walkers()
            obstacles = obstacles.models()
        arr = (_lib.LscObstacleModel * len(obstacles))()
        for m, (kind, speed, points) in zip(arr, obstacles):
            if len(points) > _lib.OBSTACLE_POINTS_MAX:
                raise LscError(f"set_obstacle_motion: {len(points)} points (at most {_lib.OBSTACLE_POINTS_MAX})")
            m.kind, m.n_points, m.speed = int(kind), len(points), float(speed)
            for i, p in enumerate(points):
                for k in range(3):
                    m.points[i][k] = float(p[k])
        if chasers or walkers:
            self.set_obstacle_motion_ex(arr, chasers, walkers)
        else:
            self._check(self.L.lsc_obstacle_motion(self.ctx, len(obstacles), arr))
        self._obstacle_states = None

    def set_obstacle_motion_ex(self, models, chasers, walkers):
        """lsc_obstacle_motion_ex: models as set_obstacle_motion takes them (a list of (kind, speed, points), kind 3 chasing / 4
        gaussian with no points) or a ctypes array; chasers / walkers: the records ObstacleSet.chasers() / walkers() return (dicts
        with the fields of lsc_obstacle_chaser / lsc_obstacle_walker; acc: float64 [n_acc][3])."""
        if not isinstance(models, ctypes.Array):
            arr = (_lib.LscObstacleModel * len(models))()
            for m, (kind, speed, points) in zip(arr, models):
                m.kind, m.n_points, m.speed = int(kind), len(points), float(speed)
                for i, p in enumerate(points[:_lib.OBSTACLE_POINTS_MAX]):
                    for k in range(3):
                        m.points[i][k] = float(p[k])
            models = arr
        ch = (_lib.LscObstacleChaser * max(len(chasers), 1))()
        for r, d in zip(ch, chasers):
            r.obstacle, r.target = int(d["obstacle"]), int(d["target"])
            r.start[:] = [float(x) for x in d["start"]]
            r.radius, r.max_vel, r.max_acc = float(d["radius"]), float(d["max_vel"]), float(d["max_acc"])
            r.gamma_target, r.gamma_obs = float(d["gamma_target"]), float(d["gamma_obs"])
        wk = (_lib.LscObstacleWalker * max(len(walkers), 1))()
        keep = []
        for r, d in zip(wk, walkers):
            acc = np.ascontiguousarray(d["acc"], np.float64).reshape(-1, 3)
            keep.append(acc)
            r.obstacle, r.n_acc = int(d["obstacle"]), int(d.get("n_acc", len(acc)))
            r.start[:] = [float(x) for x in d["start"]]
            r.initial_vel[:] = [float(x) for x in d["initial_vel"]]
            r.max_vel, r.acc_update_cycle = float(d["max_vel"]), float(d["acc_update_cycle"])
            r.acc = _dp(acc) if len(acc) else None
        self._check(self.L.lsc_obstacle_motion_ex(self.ctx, len(models), models, len(chasers), ch if chasers else None, len(walkers), wk if walkers else None))
        self._obstacle_states = None

    def chaser_states_read(self):
        """float64 [K][7]: position | velocity | t_last of every chasing obstacle as the last tick left it, NaN rows for the others
        (lsc_obstacle_chaser_states_read).  Synchronises the device."""
        s = np.zeros((max(getattr(self, "K", 0), 1), 7), np.float64)
        self._check(self.L.lsc_obstacle_chaser_states_read(self.ctx, _dp(s)))
        return s[:self.K].copy()

    def obstacle_clock(self, start, now, step):
        """The obstacles' clock: every tick that moves them evaluates the models at now - start, then now += step."""
        self._check(self.L.lsc_obstacle_clock(self.ctx, float(start), float(now), float(step)))

    def obstacle_clock_read(self):
        now = ctypes.c_double(0.0)
        self._check(self.L.lsc_obstacle_clock_read(self.ctx, ctypes.byref(now)))
        return now.value

    def obstacle_states_read(self):
        """(pos, vel) float32 [K][3] each: the states the last tick read, whoever wrote them.  Synchronises the device."""
        pv = np.zeros((max(getattr(self, "K", 0), 1), 6), np.float32)
        self._check(self.L.lsc_obstacle_states_read(self.ctx, _fp(pv)))
        pv = pv[:self.K]
        return pv[:, :3].copy(), pv[:, 3:].copy()

    def obstacle_positions_read(self):
        """float64 [K][3]: the positions of the last tick's stage before the rounding to float32 (lsc_obstacle_positions_read)."""
        p = np.zeros((max(getattr(self, "K", 0), 1), 3), np.float64)
        self._check(self.L.lsc_obstacle_positions_read(self.ctx, _dp(p)))
        return p[:self.K].copy()

    def flight_obstacles_read(self, first, n):
        """Rows first .. first + n - 1 of the obstacle track beside the flight log: dict(min_ratio [n] float64, below_one [n] int32,
        pos_vel [n][K][6] float32, ratio [n][T][N] float64, partner [n][T][N] int32, positions [n][K][3] float64: the stage's positions
        before the rounding to float32)."""
        if getattr(self, "_flight", None) is None:
            raise LscError("flight_obstacles_read: no flight log is open")
        T, n, N, K = self._flight[0], int(n), self.N, getattr(self, "K", 0)
        out = {"min_ratio": np.zeros(max(n, 0)), "below_one": np.zeros(max(n, 0), np.int32), "pos_vel": np.zeros((max(n, 0), K, 6), np.float32),
               "ratio": np.zeros((max(n, 0), T, N)), "partner": np.zeros((max(n, 0), T, N), np.int32)}
        self._check(self.L.lsc_flight_obstacles_read(self.ctx, int(first), n, _dp(out["min_ratio"]), _ip(out["below_one"]), _fp(out["pos_vel"]),
                                                     _dp(out["ratio"]), _ip(out["partner"])))
        out["positions"] = np.zeros((max(n, 0), K, 3), np.float64)
        if n > 0:
            self._check(self.L.lsc_flight_obstacle_positions_read(self.ctx, int(first), n, _dp(out["positions"])))
        return out

    # ---- the goal stage: patrol missions on the device (lsc_mission_*) -------------------------------------
    PLANNER_STATES = {"goto": _lib.MISSION_GOTO, "patrol": _lib.MISSION_PATROL, "goback": _lib.MISSION_GOBACK}

    def mission_open(self, start=None, goal=None, state="goto"):
        """Opens the context's mission state from start, goal [N][3] (default: the mission's).  While it is open every tick ignores its
        goal argument and plans towards the state's desired goals, which the tick's first launch updates: in "patrol" an agent that has
        arrived swaps desired goal and start, in "goback" everybody flies to the mission's start (TrajPlanner::goalPlanning)."""
        st = np.ascontiguousarray(self.mission.start if start is None else start, np.float32).reshape(self.N, 3)
        gl = np.ascontiguousarray(self.mission.goal if goal is None else goal, np.float32).reshape(self.N, 3)
        self._check(self.L.lsc_mission_open(self.ctx, _fp(st), _fp(gl)))
        self.mission_state(state)

    def mission_state(self, state):
        """startPatrolCallback / stopPatrolCallback: "goto", "patrol" or "goback" from the next tick on."""
        self._check(self.L.lsc_mission_set_state(self.ctx, self.PLANNER_STATES[state]))

    def mission_read(self):
        """dict(desired [N][3], start [N][3], legs int32 [N]: swaps made since mission_open).  Synchronises."""
        out = dict(desired=np.zeros((self.N, 3), np.float32), start=np.zeros((self.N, 3), np.float32), legs=np.zeros(self.N, np.int32))
        self._check(self.L.lsc_mission_read(self.ctx, _fp(out["desired"]), _fp(out["start"]), _ip(out["legs"])))
        return out

    def mission_close(self):
        self._check(self.L.lsc_mission_close(self.ctx))

    def set_goal_rule(self, rule, seq_threshold=5, velocity_threshold=0.1):
        """"config" (PlannerConfig.goal_mode alone) or "right_hand" with isDeadlock's two thresholds (lsc_set_goal_rule)."""
        r = {"config": _lib.GOAL_RULE_CONFIG, "right_hand": _lib.GOAL_RULE_RIGHT_HAND}[rule]
        self._check(self.L.lsc_set_goal_rule(self.ctx, r, int(seq_threshold), float(velocity_threshold)))

    # ---- host-buffer tick: TrajPlanner::plan for every agent of the shard -----------------------------
    def plan(self, state, current_goal, obs_prev_trajs, want_constraints=False):
        """state [N][9], current_goal [N][3] (None while a mission state is open: ignored then), obs_prev_trajs [N][3][30] (every agent's
        previous getTraj()).  Returns dict(traj [count][3][30], cost, status, iters[, normal, d])."""
        N, cnt = self.N, self.count
        state = np.ascontiguousarray(state, np.float32).reshape(N, 9)
        goal = None if current_goal is None else np.ascontiguousarray(current_goal, np.float32).reshape(N, 3)
        prev = np.ascontiguousarray(obs_prev_trajs, np.float32).reshape(N, 3, self.SEGV)
        self.planner_seq += 1                                   # src/traj_planner.cpp:127
        out = np.zeros((cnt, 3, self.SEGV), np.float32)
        cost = self.qp_cost[self.first:self.first + cnt].copy()
        status = np.zeros(cnt, np.int32)
        iters = np.zeros(cnt, np.int32)
        nobs = max(N - 1 + getattr(self, "K", 0), 1)            # the other agents, then the dynamic obstacles
        nrm = np.zeros((cnt, nobs, self.M, 3), np.float32) if want_constraints else None
        dd = np.zeros((cnt, nobs, self.M, NC), np.float64) if want_constraints else None
        sfc = np.zeros((cnt, self.M, 6), np.float32) if self.cfg.use_octomap else None
        self._check(self.L.lsc_replan_tick(self.ctx, _fp(state), _fp(goal) if goal is not None else None, _fp(prev), self.planner_seq, _fp(out), _dp(cost),
                                           _ip(status), _ip(iters), _fp(nrm) if want_constraints else None,
                                           _dp(dd) if want_constraints else None, _fp(sfc) if sfc is not None else None))
        sl = slice(self.first, self.first + cnt)
        self.traj_curr[sl] = out
        self.qp_cost[sl] = cost
        self.planning_report[sl] = status
        self.iters[sl] = iters
        res = {"traj": out, "cost": cost, "status": status, "iters": iters}
        if sfc is not None:
            res["sfc"] = sfc
        if want_constraints:
            res["normal"], res["d"] = nrm, dd
        return res

    def plan_all(self, state, current_goal, obs_prev_trajs):
        """Multi-GPU form of plan(): every rank passes all N agents' inputs, plans its shard and receives ALL N outputs
        (one RCCL all-gather group inside lsc_replan_tick_all)."""
        N = self.N
        state = np.ascontiguousarray(state, np.float32).reshape(N, 9)
        goal = np.ascontiguousarray(current_goal, np.float32).reshape(N, 3)
        prev = np.ascontiguousarray(obs_prev_trajs, np.float32).reshape(N, 3, self.SEGV)
        self.planner_seq += 1
        out = np.zeros((N, 3, self.SEGV), np.float32)
        cost = self.qp_cost.copy()
        status = np.zeros(N, np.int32)
        iters = np.zeros(N, np.int32)
        goals = np.zeros((N, 3), np.float32)
        self._check(self.L.lsc_replan_tick_all(self.ctx, _fp(state), _fp(goal), _fp(prev), self.planner_seq, _fp(out), _dp(cost),
                                               _ip(status), _ip(iters), _fp(goals)))
        self.traj_curr[:] = out
        self.qp_cost[:] = cost
        self.planning_report[:] = status
        self.iters[:] = iters
        return {"traj": out, "cost": cost, "status": status, "iters": iters, "goal": goals}

    # ---- getters with the reference's names ------------------------------------------------------------
    def get_traj(self):
        return self.traj_curr

    def get_qp_cost(self):
        return self.qp_cost

    def get_planning_report(self):
        return self.planning_report

    def get_planner_seq(self):
        return self.planner_seq

    def last_goals(self):
        """current_goal_position used by the last tick (getCurrentGoalPosition of every agent)."""
        g = np.zeros((self.N, 3), np.float32)
        self._check(self.L.lsc_last_goals(self.ctx, _fp(g)))
        return g

    def goal_storage(self):
        """Where each agent's grid search of the last tick kept its OPEN rows: 0 LDS, 1 LDS restarted in HBM, 2 HBM (int [count])."""
        out = np.zeros(self.count, np.int32)
        self._check(self.L.lsc_goal_storage(self.ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out

    def set_goal_trace(self, path_cap=512):
        """Keep every agent's grid path of the following ticks (goal_mode prior_based + use_octomap)."""
        self._goal_path_cap = path_cap
        self._check(self.L.lsc_set_goal_trace(self.ctx, path_cap))

    def goal_trace(self):
        """dict(paths = list of int[n][3] grid cells, flags, expansions, grid_dims, grid_min) of the last tick."""
        cap = getattr(self, "_goal_path_cap", 0)
        cnt = self.count
        cells = np.zeros((cnt, max(cap, 1), 3), np.int32)
        plen = np.zeros(cnt, np.int32)
        flags = np.zeros(cnt, np.int32)
        exp = np.zeros(cnt, np.int32)
        dims = np.zeros(3, np.int32)
        gmin = np.zeros(3)
        self._check(self.L.lsc_get_goal_trace(self.ctx, _ip(cells) if cap else None, _ip(plen) if cap else None, _ip(flags), _ip(exp),
                                              _ip(dims), _dp(gmin)))
        return {"paths": [cells[q, :min(plen[q], cap)].copy() for q in range(cnt)], "path_len": plen, "flags": flags,
                "expansions": exp, "grid_dims": dims, "grid_min": gmin}

    def row_counts(self):
        rows = np.zeros(self.N, np.int32)
        self._check(self.L.lsc_last_row_counts(self.ctx, _ip(rows)))
        return rows

    def neighbour_counts(self, priority=False):
        """Units (obstacle, segment) the LSC build of each agent was handed in the last tick (-1: no list) -- with priority=True also the
        number of candidates of the priority rule -- or None when the context builds no neighbour lists (swarms below 512 or above 65 536 agents)."""
        units, prio = np.zeros(self.N, np.int32), np.zeros(self.N, np.int32)
        if self.L.lsc_neighbour_counts(self.ctx, _ip(units), _ip(prio) if priority else None) != 0:
            return None
        return (units, prio) if priority else units

    def neighbour_dump(self):
        """Everything the grid kernels of the neighbour lists wrote in the last tick (lsc_neighbour_dump; diagnostics): dict(obs_bound
        float32 [N][4], seg_bound [N][M][4], reach [N][M], query_radius float, unit_count int32 [N] (-1: no list), units = list of N int32
        arrays (obstacle * M + segment, decoded to 32 bits), priority_count [N], priority = list of N int32 arrays, disturbed [N]).  Raises
        LscError with the cause when the context has no lists or the last tick built none."""
        N, M = self.N, self.M
        caps = np.zeros(2, np.int32)
        self._check(self.L.lsc_neighbour_dump(self.ctx, _ip(caps), None, None, None, None, None, None, None, None, None))
        d = dict(obs_bound=np.zeros((N, 4), np.float32), seg_bound=np.zeros((N, M, 4), np.float32), reach=np.zeros((N, M), np.float32),
                 unit_count=np.zeros(N, np.int32), priority_count=np.zeros(N, np.int32), disturbed=np.zeros(N, np.int32))
        g = ctypes.c_float()
        units, prio = np.zeros((N, int(caps[0])), np.int32), np.zeros((N, int(caps[1])), np.int32)
        self._check(self.L.lsc_neighbour_dump(self.ctx, _ip(caps), _fp(d["obs_bound"]), _fp(d["seg_bound"]), _fp(d["reach"]), ctypes.byref(g),
                                              _ip(d["unit_count"]), _ip(units), _ip(d["priority_count"]), _ip(prio), _ip(d["disturbed"])))
        d["query_radius"] = float(g.value)
        d["units"] = [units[q, :max(int(n), 0)].copy() for q, n in enumerate(d["unit_count"])]
        d["priority"] = [prio[q, :max(int(n), 0)].copy() for q, n in enumerate(d["priority_count"])]
        return d

    def row_capacity(self):
        """(rows of the LDS pass in the latency build, rows in the throughput build or 0)."""
        a, b = ctypes.c_int(), ctypes.c_int()
        self._check(self.L.lsc_row_capacity(self.ctx, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def bucket_max(self):
        """Rows of every agent's fullest control-point bucket in the last tick (first-pass LDS capacity needed)."""
        rows = np.zeros(self.N, np.int32)
        self._check(self.L.lsc_last_bucket_max(self.ctx, _ip(rows)))
        return rows

    def gjk_batch(self, pts):
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 6, 3)
        v = np.zeros((len(pts), 3))
        d = np.zeros(len(pts))
        self._check(self.L.lsc_gjk_batch(self.ctx, _dp(pts), len(pts), _dp(v), _dp(d)))
        return v, d

    # ---- device-resident stepping (torch tensors own the memory) ---------------------------------------
    def tick_device(self, state, goal, traj_prev, traj_next, cost, status, iters, planner_seq, stream=0):
        self._check(self.L.lsc_tick_device(self.ctx, state.data_ptr(), goal.data_ptr(), traj_prev.data_ptr(), planner_seq,
                                           traj_next.data_ptr(), cost.data_ptr(), status.data_ptr(), iters.data_ptr(), stream))

    def tick_device_fused(self, state, goal, traj_prev, traj_next, state_next, cost, status, iters, planner_seq, stream=0):
        """One launch per tick: goal planning + LSC + QP + next ideal state of every agent of the shard."""
        self._check(self.L.lsc_tick_device_fused(self.ctx, state.data_ptr(), goal.data_ptr(), traj_prev.data_ptr(), planner_seq,
                                                 traj_next.data_ptr(), state_next.data_ptr(), cost.data_ptr(), status.data_ptr(),
                                                 iters.data_ptr(), stream))

    def tick_device_sharded(self, state, goal, traj_prev, traj_next, cost, status, iters, planner_seq, stream=0):
        """Sharded tick, everything enqueued on `stream`: plan the rank's agents, in-place RCCL all-gather of traj_next
        ([table_rows][90], padded), next ideal state of all N agents into `state`."""
        self._check(self.L.lsc_tick_device_sharded(self.ctx, state.data_ptr(), goal.data_ptr(), traj_prev.data_ptr(), planner_seq,
                                                   traj_next.data_ptr(), cost.data_ptr(), status.data_ptr(), iters.data_ptr(), stream))

    # ---- K closed-loop ticks per call, with the mission's bookkeeping in a device-side flight log ------------------
    def flight_begin(self, times, capacity, samples=True, safety=True, agents=True):
        """Opens a flight log of `capacity` ticks: per tick the summary (lsc_flight_tick) and, as chosen, the record samples of every
        agent at `times` (seconds into the new plan), the agent-agent safety ratios and partners at those times, and cost / status /
        end point per agent.  fly() then appends one row per tick; flight_read() brings rows to the host."""
        t = np.ascontiguousarray(times, np.float64).ravel()
        if not 1 <= len(t) <= _lib.FLIGHT_MAX_TIMES:
            raise LscError(f"flight_begin: {len(t)} record times (1..{_lib.FLIGHT_MAX_TIMES})")
        fc = _lib.LscFlightConfig()
        fc.capacity_ticks, fc.n_times = int(capacity), len(t)
        for i, v in enumerate(t):
            fc.times[i] = float(v)
        fc.what = (_lib.FLIGHT_SAMPLES if samples else 0) | (_lib.FLIGHT_SAFETY if safety else 0) | (_lib.FLIGHT_AGENTS if agents else 0)
        self._check(self.L.lsc_flight_begin(self.ctx, ctypes.byref(fc)))
        self._flight = (len(t), fc.what)

    def flight_reset(self):
        self._check(self.L.lsc_flight_reset(self.ctx))

    def flight_end(self):
        self._check(self.L.lsc_flight_end(self.ctx))
        self._flight = None

    def fly(self, states, goal, trajs, first_seq, n_ticks, cost, status, iters, stream=0):
        """n_ticks closed-loop ticks enqueued by one call (lsc_fly_device): tick j reads states[j & 1] / trajs[j & 1] with planner_seq
        first_seq + j and writes trajs[(j + 1) & 1] / states[(j + 1) & 1], exactly as tick_device_fused would; with a flight log open
        one record launch follows each tick.  No host synchronisation.  states, trajs: pairs of torch tensors."""
        vp = ctypes.c_void_p
        st = (vp * 2)(states[0].data_ptr(), states[1].data_ptr())
        tr = (vp * 2)(trajs[0].data_ptr(), trajs[1].data_ptr())
        self._check(self.L.lsc_fly_device(self.ctx, st, goal.data_ptr(), tr, int(first_seq), int(n_ticks), cost.data_ptr(), status.data_ptr(),
                                          iters.data_ptr(), stream))

    FLIGHT_TICK = np.dtype([("planner_seq", np.int32), ("unmet", np.int32), ("end_unmet", np.int32), ("moved", np.int32),
                            ("n_status", np.int32, (6,)), ("min_ratio", np.float64), ("pad", np.int32, (4,))])

    def flight_read(self, first, n):
        """Rows first .. first + n - 1 of the flight log (synchronises the stream last flown on): dict(summary = structured array [n]
        of FLIGHT_TICK, and the recorded parts: samples [n][T][N][9], ratio / partner [n][T][N], cost / status [n][N], end [n][N][3])."""
        if getattr(self, "_flight", None) is None:
            raise LscError("flight_read: no flight log is open")
        T, what = self._flight
        n, N = int(n), self.N
        out = {"summary": np.zeros(max(n, 0), self.FLIGHT_TICK)}
        if what & _lib.FLIGHT_SAMPLES:
            out["samples"] = np.zeros((n, T, N, 9), np.float32)
        if what & _lib.FLIGHT_SAFETY:
            out["ratio"], out["partner"] = np.zeros((n, T, N), np.float64), np.zeros((n, T, N), np.int32)
        if what & _lib.FLIGHT_AGENTS:
            out["cost"], out["status"], out["end"] = np.zeros((n, N), np.float64), np.zeros((n, N), np.int32), np.zeros((n, N, 3), np.float32)

        def ptr(name, conv):
            return conv(out[name]) if name in out else None
        self._check(self.L.lsc_flight_read(self.ctx, int(first), n, out["summary"].ctypes.data_as(ctypes.POINTER(_lib.LscFlightTick)),
                                           ptr("samples", _fp), ptr("ratio", _dp), ptr("partner", _ip), ptr("cost", _dp),
                                           ptr("status", _ip), ptr("end", _fp)))
        return out

    def propagate_device(self, traj, state, stream=0):
        self._check(self.L.lsc_propagate_device(self.ctx, traj.data_ptr(), state.data_ptr(), stream))

    def sweep_device(self, state, traj_prev, planner_seq, normal, d, stream=0):
        """Dense LSC sweep; d float64 (what the QP reads) or float32 (the compact dump: 180 B per ordered pair)."""
        import torch
        fn = self.L.lsc_sweep_device_f32 if d.dtype == torch.float32 else self.L.lsc_sweep_device
        self._check(fn(self.ctx, state.data_ptr(), traj_prev.data_ptr(), planner_seq, normal.data_ptr(), d.data_ptr(), stream))

    PHASES = ("setup", "lsc_build", "ip_init", "residual_pass", "row_reduce", "assemble", "cholesky", "tri_solves",
              "affine_pass", "corrector_pass", "step_update", "output", "(row_reduce: buckets, wave 0)", "(row_reduce: axis gather, last lane)",
              "(tri_solves: the substitutions of wave 0 alone)", "(spare)")

    def phase_profile(self, enable=-1):
        out = np.zeros((self.N, 16), np.int64)
        self._check(self.L.lsc_phase_profile(self.ctx, enable, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return out

    GOAL_SECTIONS = ("prologue", "grid_setup", "search", "path_los", "find_min", "delete_min", "screening", "insertions",
                     "general_pop_cycles", "general_pops", "general_insert_cycles", "general_inserts")

    def goal_profile(self, enable=-1):
        out = np.zeros((self.N, 16), np.int64)
        self._check(self.L.lsc_goal_profile(self.ctx, enable, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return out

    def safety_ratio(self, times):
        """savePlanningResult's agent-agent accounting for the plans of the last plan() call: (ratio [T][count], partner [T][count],
        minimum over everything -- over all ranks with a communicator)."""
        t = np.ascontiguousarray(times, np.float64)
        ratio = np.zeros((len(t), self.count), np.float64)
        partner = np.zeros((len(t), self.count), np.int32)
        mn = ctypes.c_double()
        self._check(self.L.lsc_safety_ratio(self.ctx, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(t),
                                            ratio.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                            partner.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(mn)))
        return ratio, partner, mn.value

    GENERAL_SECTIONS = ("setup", "start", "residual_pass", "row_reduce", "assemble", "factor", "solves", "affine_pass",
                        "corrector_rhs", "row_reduce_2", "assemble_2", "step", "iterations", "solves_of_agent")

    def general_profile(self):
        """Sections of lsc_general_kernel, collected while phase_profile is enabled: [N][16] shader cycles / counts."""
        out = np.zeros((self.N, 16), np.int64)
        self._check(self.L.lsc_general_profile(self.ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return out

    def general_info(self):
        """(kept obstacles of one agent up to which the alternate-mode solver has every row array in LDS -- beyond, its generic-pointer build
        runs --, how the last tick reached that solver: 0 not at all, 1 folded into the plan kernel, 2 lsc_general_kernel, 3 its batch form)."""
        a, b = ctypes.c_int(), ctypes.c_int()
        self._check(self.L.lsc_general_info(self.ctx, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def dump_qp(self, agent, path):
        """TrajOptimizer::solve's failure export (log/QPmodel.lp): the agent's QP of the last plan() call as a CPLEX LP file."""
        self._check(self.L.lsc_dump_qp(self.ctx, int(agent), str(path).encode()))

    def solver_residuals(self):
        out = np.zeros((self.N, 4))
        self._check(self.L.lsc_solver_residuals(self.ctx, _dp(out)))
        return out

    def solver_trace(self, agent, read=False):
        ny = 3 * (3 * (self.M - 1) + 1)
        kld = ny + 2 - (ny % 2 == 0)
        wsz = 3 * self.NV + 6 * self.SEGV
        out = np.zeros(64 * 8 + ny * kld + wsz + 512)
        self._check(self.L.lsc_solver_trace(self.ctx, agent, _dp(out) if read else None))
        self.trace_K = out[512:512 + ny * kld].reshape(ny, kld)[:, :ny]
        self.trace_W = out[512 + ny * kld:512 + ny * kld + wsz]
        self.trace_kconst = out[512 + ny * kld + wsz:]
        return out[:512].reshape(64, 8)

    def iterations_total(self, reset=False):
        t = ctypes.c_longlong()
        self._check(self.L.lsc_iterations_total(self.ctx, ctypes.byref(t), int(reset)))
        return t.value

    def row_iterations_total(self):
        """Sum over agents of iterations x LSC rows carried since the last iterations_total(reset=True)."""
        t = ctypes.c_longlong()
        self._check(self.L.lsc_row_iterations_total(self.ctx, ctypes.byref(t)))
        return t.value

    def solver_stats(self):
        """Counters of the active-set solve since the last iterations_total(reset=True): dict(solved, handed_over, changes, ip_iterations)."""
        out = (ctypes.c_longlong * 4)()
        self._check(self.L.lsc_solver_stats(self.ctx, out))
        return dict(solved=out[0], handed_over=out[1], changes=out[2], ip_iterations=out[3])

    def working_set_peaks(self):
        """Largest working set of every agent's last active-set solve (lsc_working_set_peaks): int32 [N]; 13 = the solve asked for a
        thirteenth row and handed the agent over.  The first call switches the counter on and reads zeros."""
        out = np.zeros(self.N, np.int32)
        self._check(self.L.lsc_working_set_peaks(self.ctx, _ip(out)))
        return out

    def set_timing(self, on):
        self._check(self.L.lsc_set_timing(self.ctx, int(on)))

    def kernel_time_ms(self, which=0):
        ms = ctypes.c_double()
        n = ctypes.c_long()
        self._check(self.L.lsc_kernel_time_ms(self.ctx, which, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def kernel_times_ms(self, which=0):
        """Per-launch device times (ms) since set_timing(True).  A sample is the launch's own dispatch time, begin of its first kernel to
        end of its last (the events ride on the dispatches, hipExtLaunchKernel: what rocprofv3 reports for the kernel), not the time
        between two markers in the stream: the way to the kernel is not in it.  which = 2 (the RCCL exchange) stays a recorded pair.
        Samples of which = 0 are stamped by the kernels themselves where they can be (first workgroup's entry to last exit, by the
        device's clock; include/lsc_planner_amd.h says when events time them instead): kernel_samples_stamped() counts those."""
        n = ctypes.c_long()
        self._check(self.L.lsc_kernel_times_ms(self.ctx, which, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), np.float64)
        self._check(self.L.lsc_kernel_times_ms(self.ctx, which, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n.value,
                                               ctypes.byref(n)))
        return out[:n.value]

    def kernel_samples_stamped(self):
        """How many samples of kernel_times_ms(0) since set_timing(True) the kernels stamped themselves (the others rode on events)."""
        return self.kernel_time_ms(100)[1]          # LSC_TIME_STAMPED_COUNT


def tick_device_fused_batch(planners, states, goals, trajs_prev, trajs_next, states_next, costs, statuses, iters, planner_seqs, stream=0):
    """One tick of several independent swarms -- one SwarmPlanner (context) each, all on one device -- in ONE launch
    (lsc_tick_device_fused_batch): every argument is a list with one entry per swarm; results are those of tick_device_fused."""
    n = len(planners)
    L = planners[0].L
    # one library (liblsc_hip.so and liblsc_hip_m4.so lay the same lsc_ctx symbol out with different array sizes: a context of the other
    # build would be read with the wrong sizes) and every context once (its stale-plan / hand-over buffers belong to ONE swarm of the launch)
    if not all(p.L is L for p in planners):
        raise LscError("tick_device_fused_batch: planners of different libraries (segment counts) in one batch")
    if len({int(getattr(p.ctx, "value", p.ctx) or 0) for p in planners}) != n:
        raise LscError("tick_device_fused_batch: the same planner (context) more than once in one batch")
    vp = ctypes.c_void_p

    def ptrs(ts):
        return (vp * n)(*[t.data_ptr() for t in ts])
    ctxs = (vp * n)(*[p.ctx for p in planners])
    seqs = (ctypes.c_int * n)(*[int(q) for q in planner_seqs])
    rc = L.lsc_tick_device_fused_batch(ctxs, n, ptrs(states), ptrs(goals), ptrs(trajs_prev), seqs, ptrs(trajs_next), ptrs(states_next),
                                       ptrs(costs), ptrs(statuses), ptrs(iters), stream)
    if rc != 0:
        raise LscError(f"lsc error {rc}: {L.lsc_last_error(planners[0].ctx).decode()}")


def replan_tick_batch(planners, states, goals, prev_trajs, planner_seqs):
    """Host-buffer tick of several independent swarms in one batched tick (lsc_replan_tick_batch): every argument is a list with one
    entry per planner (state [N][9], goal [N][3], prev_traj [N][3][SEGV], planner_seq after its increment).  Returns per planner
    (traj [count][3][SEGV], cost, status, iters): the bits lsc_replan_tick gives each planner alone.  Planner state (traj_curr ...)
    is not updated: the caller owns the loop, as with tick_device_fused_batch."""
    n = len(planners)
    L = planners[0].L
    if not all(p.L is L for p in planners):
        raise LscError("replan_tick_batch: planners of different libraries (segment counts) in one batch")
    if len({int(getattr(p.ctx, "value", p.ctx) or 0) for p in planners}) != n:
        raise LscError("replan_tick_batch: the same planner (context) more than once in one batch")
    ins, outs = [], []
    for p, st, g, pr in zip(planners, states, goals, prev_trajs):
        ins.append((np.ascontiguousarray(st, np.float32).reshape(p.N, 9), np.ascontiguousarray(g, np.float32).reshape(p.N, 3),
                    np.ascontiguousarray(pr, np.float32).reshape(p.N, 3, p.SEGV)))
        outs.append((np.zeros((p.count, 3, p.SEGV), np.float32), np.zeros(p.count), np.zeros(p.count, np.int32), np.zeros(p.count, np.int32)))
    vp = ctypes.c_void_p

    def arr(xs):
        return (vp * n)(*[x.ctypes.data for x in xs])
    rc = L.lsc_replan_tick_batch((vp * n)(*[p.ctx for p in planners]), n, arr([i[0] for i in ins]), arr([i[1] for i in ins]),
                                 arr([i[2] for i in ins]), (ctypes.c_int * n)(*[int(q) for q in planner_seqs]),
                                 arr([o[0] for o in outs]), arr([o[1] for o in outs]), arr([o[2] for o in outs]), arr([o[3] for o in outs]))
    if rc != 0:
        raise LscError(f"lsc error {rc}: {L.lsc_last_error(planners[0].ctx).decode()}")
    return outs


def flight_weights(dt, times, segments=5):
    """Host only (lsc_flight_weights): the Bernstein weights (w5 [T][6], w4 [T][5], w3 [T][4]) and the segment [T] of each record time, as
    the record kernel of the library built for `segments` is handed them.  Raises LscError for a time outside the horizon."""
    L = _lib.load_library(segments)
    t = np.ascontiguousarray(times, np.float64).ravel()
    w5, w4, w3, seg = np.zeros((len(t), 6)), np.zeros((len(t), 5)), np.zeros((len(t), 4)), np.zeros(len(t), np.int32)
    rc = L.lsc_flight_weights(float(dt), _dp(t), len(t), _dp(w5), _dp(w4), _dp(w3), _ip(seg))
    if rc != 0:
        raise LscError(f"lsc_flight_weights failed: {rc} (1..64 times inside the horizon of {segments} segments of {dt} s)")
    return w5, w4, w3, seg


def comm_unique_id():
    """Rendezvous token of the RCCL communicator (ncclGetUniqueId): rank 0 makes it, every rank passes it to PlannerConfig.comm."""
    L = _lib.load_library()
    buf = (ctypes.c_ubyte * _lib.COMM_ID_BYTES)()
    rc = L.lsc_comm_unique_id(buf)
    if rc != 0:
        raise LscError(f"lsc_comm_unique_id failed: {rc} (librccl.so not loadable?)")
    return bytes(buf)


def edt_from_bt(bt_path, world_min, world_max, maxdist=1.0):
    """Host-only: octomap .bt -> (dist float32 [nx][ny][nz], key_min int32[3], res).  No GPU needed."""
    L = _lib.load_library()
    fpp = ctypes.POINTER(ctypes.c_float)
    wm = np.ascontiguousarray(world_min, np.float32)
    wM = np.ascontiguousarray(world_max, np.float32)
    edt = fpp()
    dims = (ctypes.c_int * 3)()
    kmin = (ctypes.c_int * 3)()
    res = ctypes.c_double()
    rc = L.lsc_edt_from_bt(str(bt_path).encode(), _fp(wm), _fp(wM), float(maxdist), ctypes.byref(edt), dims, kmin, ctypes.byref(res))
    if rc != 0:
        raise LscError(f"lsc_edt_from_bt({bt_path}) failed: {rc}")
    arr = np.ctypeslib.as_array(edt, shape=tuple(dims)).copy()
    L.lsc_free_host(edt)
    return arr, np.array(list(kmin), np.int32), res.value


def occupancy_from_bt(bt_path, world_min, world_max):
    """Host-only: octomap .bt -> (occupancy uint8 [nx][ny][nz], key_min int32[3], res): the cells where edt_from_bt is 0."""
    L = _lib.load_library()
    ubp = ctypes.POINTER(ctypes.c_ubyte)
    wm = np.ascontiguousarray(world_min, np.float32)
    wM = np.ascontiguousarray(world_max, np.float32)
    occ = ubp()
    dims = (ctypes.c_int * 3)()
    kmin = (ctypes.c_int * 3)()
    res = ctypes.c_double()
    rc = L.lsc_occupancy_from_bt(str(bt_path).encode(), _fp(wm), _fp(wM), ctypes.byref(occ), dims, kmin, ctypes.byref(res))
    if rc != 0:
        raise LscError(f"lsc_occupancy_from_bt({bt_path}) failed: {rc}")
    arr = np.ctypeslib.as_array(occ, shape=tuple(dims)).copy()
    L.lsc_free_host(occ)
    return arr, np.array(list(kmin), np.int32), res.value


def next_state_host(traj, dt=0.2):
    """getStateFromControlPoints at t = dt in float32 (include/polynomial.hpp:63-97), numpy, all agents."""
    t = np.asarray(traj, np.float32)
    t = t if t.ndim == 3 else t.reshape(len(t), 3, -1)          # [N][3][M (n + 1)] for any M (or the same rows flattened)
    c1 = t[:, :, NC:NC + 3]
    fn, fn1, finv = np.float32(5), np.float32(4), np.float32(dt ** -1)
    v0 = ((c1[:, :, 1] - c1[:, :, 0]) * fn) * finv
    v1 = ((c1[:, :, 2] - c1[:, :, 1]) * fn) * finv
    a0 = ((v1 - v0) * fn1) * finv
    return np.concatenate([c1[:, :, 0], v0, a0], axis=1).astype(np.float32)
