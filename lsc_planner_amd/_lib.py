"""ctypes binding of the C ABI declared in include/lsc_planner_amd.h.

There is no CPU fallback: if liblsc_hip.so is missing this raises, and every compute entry point fails
when no gfx950 device is usable.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBS = {}

# M = 5 (every shipped launch file) is the default build; load_library(4) loads the M = 4 build of the same sources
M, DEG, NC, SEGV, NV = 5, 5, 6, 30, 90


def segments_of(horizon, dt):
    """M = static_cast<int>((horizon + SP_EPSILON) / dt), src/traj_optimizer.cpp:9."""
    return int((horizon + 1e-9) / dt)

STATUS_OK, STATUS_INFEASIBLE, STATUS_SFC_BLOCKED, STATUS_GOAL_CAPACITY = 0, 1, 4, 5
COMM_ID_BYTES = 128


class LscError(RuntimeError):
    pass


class LscConfig(ctypes.Structure):
    _fields_ = [
        ("dt", ctypes.c_double),
        ("control_weight", ctypes.c_double),
        ("terminal_weight", ctypes.c_double),
        ("world_min", ctypes.c_float * 3),
        ("world_max", ctypes.c_float * 3),
        ("use_octomap", ctypes.c_int),
        ("world_resolution", ctypes.c_double),
        ("device", ctypes.c_int),
        ("max_rows_per_cp", ctypes.c_int),
        ("max_iters", ctypes.c_int),
        ("prune", ctypes.c_int),
        ("goal_mode", ctypes.c_int),
        ("goal_threshold", ctypes.c_double),
        ("priority_dist_threshold", ctypes.c_double),
        ("goal_radius", ctypes.c_double),
        ("warm_start_mu", ctypes.c_double),
        ("grid_resolution", ctypes.c_double),
        ("grid_margin", ctypes.c_double),
        ("horizon", ctypes.c_double),
        ("goal_row_cap", ctypes.c_int),
        ("planner_mode", ctypes.c_int),
        ("slack_mode", ctypes.c_int),
        ("slack_collision_weight", ctypes.c_double),
        ("n_constraint_segments", ctypes.c_int),
        ("reset_threshold", ctypes.c_double),
        ("gap_tolerance", ctypes.c_double),
        ("world_dimension", ctypes.c_int),
        ("world_z_2d", ctypes.c_double),
        ("goal_search", ctypes.c_int),
        ("solver", ctypes.c_int),
        ("goal_lds_row_cap", ctypes.c_int),
    ]


# every symbol include/lsc_planner_amd.h declares
EXPORTS = [
    "lsc_default_config", "lsc_create", "lsc_destroy", "lsc_last_error", "lsc_last_note", "lsc_segments", "lsc_set_agents", "lsc_set_shard",
    "lsc_set_distmap", "lsc_replan_tick", "lsc_tick_device", "lsc_tick_device_fused", "lsc_propagate_device", "lsc_safety_ratio", "lsc_sweep_device", "lsc_sweep_device_f32",
    "lsc_gjk_batch", "lsc_kernel_time_ms", "lsc_kernel_times_ms", "lsc_set_timing", "lsc_last_row_counts", "lsc_iterations_total", "lsc_phase_profile", "lsc_goal_profile", "lsc_goal_key_table", "lsc_general_profile", "lsc_general_info", "lsc_dump_qp", "lsc_solver_residuals", "lsc_solver_trace", "lsc_edt_from_bt", "lsc_free_host", "lsc_last_goals", "lsc_goal_storage", "lsc_set_goal_trace", "lsc_get_goal_trace",
    "lsc_last_bucket_max", "lsc_row_capacity", "lsc_comm_unique_id", "lsc_comm_init", "lsc_comm_info", "lsc_tick_device_sharded", "lsc_replan_tick_all",
    "lsc_row_iterations_total", "lsc_tick_device_fused_batch", "lsc_solver_stats", "lsc_working_set_peaks", "lsc_neighbour_counts", "lsc_neighbour_dump", "lsc_replan_tick_batch",
    "lsc_flight_weights", "lsc_flight_row_bytes", "lsc_flight_begin", "lsc_flight_reset", "lsc_flight_end", "lsc_fly_device", "lsc_flight_read",
    "lsc_set_obstacles", "lsc_set_obstacles_ex", "lsc_obstacle_states", "lsc_obstacle_states_device",
    "lsc_obstacle_motion", "lsc_obstacle_clock", "lsc_obstacle_clock_read", "lsc_obstacle_states_read", "lsc_flight_obstacles_read",
    "lsc_obstacle_positions_read", "lsc_flight_obstacle_positions_read", "lsc_obstacle_motion_ex", "lsc_obstacle_chaser_states_read",
    "lsc_mission_open", "lsc_mission_set_state", "lsc_mission_read", "lsc_mission_close", "lsc_set_goal_rule",
    "lsc_occupancy_from_bt", "lsc_set_occupancy", "lsc_map_update", "lsc_map_update_device", "lsc_map_read",
]

# the map from occupancy (LSC_MAP_* of the header)
MAP_BOXES_MAX = 64
MAP_REGROW_CORRIDORS = 1
MAP_DIMS, MAP_OCCUPANCY, MAP_EDT, MAP_INTEGRAL, MAP_GOAL_OCCUPANCY = 0, 1, 2, 3, 4
MAP_DIMS_INTS = 8

# planner states of a mission state and goal rules (LSC_MISSION_* / LSC_GOAL_RULE_* of the header)
MISSION_GOTO, MISSION_PATROL, MISSION_GOBACK = 0, 1, 2
GOAL_RULE_CONFIG, GOAL_RULE_RIGHT_HAND = 0, 1

OBSTACLES_MAX = 64           # LSC_OBSTACLES_MAX of the header
OBSTACLE_POINTS_MAX = 8      # LSC_OBSTACLE_POINTS_MAX
OBSTACLE_STRAIGHT, OBSTACLE_SPIN, OBSTACLE_PATROL = 0, 1, 2      # LSC_OBSTACLE_*
OBSTACLE_CHASING, OBSTACLE_GAUSSIAN = 3, 4


class LscObstacleModel(ctypes.Structure):    # lsc_obstacle_model: one obstacle's motion model (lsc_obstacle_motion)
    _fields_ = [("kind", ctypes.c_int), ("n_points", ctypes.c_int), ("speed", ctypes.c_double),
                ("points", (ctypes.c_double * 3) * OBSTACLE_POINTS_MAX)]

class LscObstacleChaser(ctypes.Structure):   # lsc_obstacle_chaser: one chasing obstacle's record (lsc_obstacle_motion_ex)
    _fields_ = [("obstacle", ctypes.c_int), ("target", ctypes.c_int), ("start", ctypes.c_double * 3), ("radius", ctypes.c_double),
                ("max_vel", ctypes.c_double), ("max_acc", ctypes.c_double), ("gamma_target", ctypes.c_double), ("gamma_obs", ctypes.c_double)]


class LscObstacleWalker(ctypes.Structure):   # lsc_obstacle_walker: one gaussian obstacle's record
    _fields_ = [("obstacle", ctypes.c_int), ("n_acc", ctypes.c_int), ("start", ctypes.c_double * 3), ("initial_vel", ctypes.c_double * 3),
                ("max_vel", ctypes.c_double), ("acc_update_cycle", ctypes.c_double), ("acc", ctypes.POINTER(ctypes.c_double))]


# what a flight log records per tick besides the summary (LSC_FLIGHT_* of the header)
FLIGHT_SAMPLES, FLIGHT_SAFETY, FLIGHT_AGENTS = 1, 2, 4
FLIGHT_MAX_TIMES = 64


class LscFlightConfig(ctypes.Structure):
    _fields_ = [("capacity_ticks", ctypes.c_int), ("n_times", ctypes.c_int), ("times", ctypes.c_double * 64), ("what", ctypes.c_int)]


class LscFlightTick(ctypes.Structure):       # 64 bytes: one summary row of the log
    _fields_ = [("planner_seq", ctypes.c_int), ("unmet", ctypes.c_int), ("end_unmet", ctypes.c_int), ("moved", ctypes.c_int),
                ("n_status", ctypes.c_int * 6), ("min_ratio", ctypes.c_double), ("pad", ctypes.c_int * 4)]


BUILT_SEGMENTS = (5, 4)      # csrc/Makefile builds these two; other M = recompile with -DLSC_SEGMENTS=k (3 <= k <= 5)


def lib_path(segments=5):
    """liblsc_hip.so (M = 5) / liblsc_hip_m4.so (M = 4) next to this file.  LSC_HIP_LIB overrides the M = 5 path and
    LSC_HIP_LIB_M4 the M = 4 one (A/B runs of two builds on the same GPU box; the LDS-poison builds of `make poison poison_m4`)."""
    if segments == 5:
        return os.environ.get("LSC_HIP_LIB") or os.path.join(_HERE, "liblsc_hip.so")
    if segments == 4:
        return os.environ.get("LSC_HIP_LIB_M4") or os.path.join(_HERE, "liblsc_hip_m4.so")
    return os.path.join(_HERE, f"liblsc_hip_m{segments}.so")


def load_library(segments=5):
    """Loads the library built for `segments` = horizon / dt (__graft_entry__.build() / csrc/Makefile).  Raises if absent."""
    if segments in _LIBS:
        return _LIBS[segments]
    p = lib_path(segments)
    if not os.path.exists(p):
        raise LscError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # PyTorch wheels bundle their own HIP/HSA runtime.  Two runtimes in one process do not coexist (the second one
    # finds "no HIP GPUs"), so when this harness runs next to torch, torch's runtime must be the one that is loaded
    # first; liblsc_hip.so then binds to it.  Stand-alone C++ users (lsc_sim) link /opt/rocm's runtime directly.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(p)
    vp, ip, dp, fp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    L.lsc_default_config.argtypes = [ctypes.POINTER(LscConfig)]
    L.lsc_default_config.restype = None
    L.lsc_create.argtypes = [ctypes.POINTER(LscConfig)]
    L.lsc_create.restype = vp
    L.lsc_destroy.argtypes = [vp]
    L.lsc_destroy.restype = None
    L.lsc_last_error.argtypes = [vp]
    L.lsc_last_error.restype = ctypes.c_char_p
    L.lsc_last_note.argtypes = [vp]
    L.lsc_last_note.restype = ctypes.c_char_p
    L.lsc_set_agents.argtypes = [vp, ctypes.c_int, dp, dp, dp, dp, dp]
    L.lsc_set_shard.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.lsc_set_obstacles.argtypes = [vp, ctypes.c_int, dp, dp]
    L.lsc_set_obstacles_ex.argtypes = [vp, ctypes.c_int, dp, dp, dp, ctypes.c_int, ctypes.c_double]
    L.lsc_obstacle_states.argtypes = [vp, fp]
    L.lsc_obstacle_states_device.argtypes = [vp, vp]
    L.lsc_obstacle_motion.argtypes = [vp, ctypes.c_int, ctypes.POINTER(LscObstacleModel)]
    L.lsc_obstacle_motion_ex.argtypes = [vp, ctypes.c_int, ctypes.POINTER(LscObstacleModel), ctypes.c_int, ctypes.POINTER(LscObstacleChaser),
                                         ctypes.c_int, ctypes.POINTER(LscObstacleWalker)]
    L.lsc_obstacle_chaser_states_read.argtypes = [vp, dp]
    L.lsc_obstacle_clock.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    L.lsc_obstacle_clock_read.argtypes = [vp, dp]
    L.lsc_obstacle_states_read.argtypes = [vp, fp]
    L.lsc_obstacle_positions_read.argtypes = [vp, dp]
    L.lsc_flight_obstacle_positions_read.argtypes = [vp, ctypes.c_int, ctypes.c_int, dp]
    L.lsc_flight_obstacles_read.argtypes = [vp, ctypes.c_int, ctypes.c_int, dp, ip, fp, dp, ip]
    L.lsc_set_distmap.argtypes = [vp, fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ip, ctypes.c_double]
    L.lsc_replan_tick.argtypes = [vp, fp, fp, fp, ctypes.c_int, fp, dp, ip, ip, fp, dp, fp]
    L.lsc_tick_device.argtypes = [vp, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp]
    L.lsc_tick_device_fused.argtypes = [vp, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    vpp = ctypes.POINTER(vp)
    L.lsc_tick_device_fused_batch.argtypes = [vpp, ctypes.c_int, vpp, vpp, vpp, ip, vpp, vpp, vpp, vpp, vpp, vp]
    L.lsc_replan_tick_batch.argtypes = [vpp, ctypes.c_int, vpp, vpp, vpp, ip, vpp, vpp, vpp, vpp]
    L.lsc_propagate_device.argtypes = [vp, vp, vp, vp]
    L.lsc_safety_ratio.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
    ubp = ctypes.POINTER(ctypes.c_ubyte)
    L.lsc_comm_unique_id.argtypes = [ubp]
    L.lsc_comm_init.argtypes = [vp, ctypes.c_int, ctypes.c_int, ubp]
    L.lsc_comm_info.argtypes = [vp, ip, ip, ip, ip]
    L.lsc_tick_device_sharded.argtypes = [vp, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp]
    L.lsc_replan_tick_all.argtypes = [vp, fp, fp, fp, ctypes.c_int, fp, dp, ip, ip, fp]
    L.lsc_sweep_device.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp]
    L.lsc_sweep_device_f32.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp]
    L.lsc_gjk_batch.argtypes = [vp, dp, ctypes.c_int, dp, dp]
    L.lsc_kernel_time_ms.argtypes = [vp, ctypes.c_int, dp, ctypes.POINTER(ctypes.c_long)]
    L.lsc_kernel_times_ms.argtypes = [vp, ctypes.c_int, dp, ctypes.c_long, ctypes.POINTER(ctypes.c_long)]
    L.lsc_set_timing.argtypes = [vp, ctypes.c_int]
    L.lsc_last_row_counts.argtypes = [vp, ip]
    L.lsc_neighbour_counts.argtypes = [vp, ip, ip]
    L.lsc_neighbour_dump.argtypes = [vp, ip, fp, fp, fp, fp, ip, ip, ip, ip, ip]
    L.lsc_last_bucket_max.argtypes = [vp, ip]
    L.lsc_row_capacity.argtypes = [vp, ip, ip]
    L.lsc_phase_profile.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
    L.lsc_goal_profile.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
    L.lsc_general_profile.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    L.lsc_general_info.argtypes = [vp, ip, ip]
    L.lsc_goal_key_table.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_int)]
    L.lsc_dump_qp.argtypes = [vp, ctypes.c_int, ctypes.c_char_p]
    L.lsc_solver_residuals.argtypes = [vp, dp]
    L.lsc_solver_trace.argtypes = [vp, ctypes.c_int, dp]
    L.lsc_edt_from_bt.argtypes = [ctypes.c_char_p, fp, fp, ctypes.c_double, ctypes.POINTER(fp), ip, ip, dp]
    L.lsc_last_goals.argtypes = [vp, fp]
    L.lsc_goal_storage.argtypes = [vp, ip]
    L.lsc_set_goal_trace.argtypes = [vp, ctypes.c_int]
    L.lsc_get_goal_trace.argtypes = [vp, ip, ip, ip, ip, ip, dp]
    L.lsc_free_host.argtypes = [vp]
    L.lsc_free_host.restype = None
    L.lsc_iterations_total.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    L.lsc_row_iterations_total.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    L.lsc_solver_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
    L.lsc_working_set_peaks.argtypes = [vp, ip]
    L.lsc_flight_weights.argtypes = [ctypes.c_double, dp, ctypes.c_int, dp, dp, dp, ip]
    L.lsc_flight_row_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.lsc_flight_row_bytes.restype = ctypes.c_size_t
    L.lsc_flight_begin.argtypes = [vp, ctypes.POINTER(LscFlightConfig)]
    L.lsc_flight_reset.argtypes = [vp]
    L.lsc_flight_end.argtypes = [vp]
    L.lsc_fly_device.argtypes = [vp, vpp, vp, vpp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    L.lsc_flight_read.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(LscFlightTick), fp, dp, ip, dp, ip, fp]
    L.lsc_mission_open.argtypes = [vp, fp, fp]
    L.lsc_mission_set_state.argtypes = [vp, ctypes.c_int]
    L.lsc_mission_read.argtypes = [vp, fp, fp, ip]
    L.lsc_mission_close.argtypes = [vp]
    L.lsc_set_goal_rule.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_double]
    L.lsc_occupancy_from_bt.argtypes = [ctypes.c_char_p, fp, fp, ctypes.POINTER(ubp), ip, ip, dp]
    L.lsc_set_occupancy.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ip, ctypes.c_double, ctypes.c_double]
    L.lsc_map_update.argtypes = [vp, ctypes.c_int, ip, ubp, ctypes.c_int, vp]
    L.lsc_map_update_device.argtypes = [vp, vp, ctypes.c_int, vp]
    L.lsc_map_read.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t]
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is ctypes.c_int or name not in ("lsc_default_config", "lsc_create", "lsc_destroy", "lsc_last_error", "lsc_last_note", "lsc_free_host",
                                                      "lsc_flight_row_bytes"):
            fn.restype = ctypes.c_int
    L.lsc_segments.argtypes = []
    if L.lsc_segments() != segments:
        raise LscError(f"{p} plans M = {L.lsc_segments()} segments, not {segments}")
    _LIBS[segments] = L
    return L
