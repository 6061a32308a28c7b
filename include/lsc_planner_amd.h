/*
 * lsc_planner_amd.h -- C ABI of the MI355X-native replanning path for qwerty35/lsc_planner.
 *
 * One call per replan tick for the WHOLE swarm replaces the reference's sequential
 *     for (qi...) agents[qi]->plan(sim_current_time);            src/multi_sync_simulator.cpp:320-328
 * i.e. for every agent: prediction shift -> LSC construction -> (SFC) -> QP solve
 *     TrajPlanner::planImpl / planLSC                            src/traj_planner.cpp:344-425
 *     TrajPlanner::generateLSC (GJK normals + margins)           src/traj_planner.cpp:1310-1407
 *     TrajPlanner::generateFeasibleSFC + CorridorConstructor     src/traj_planner.cpp:1451-1491,
 *                                                                include/corridor_constructor.hpp:18-245
 *     TrajOptimizer::solve / getTrajectory / getQPcost (CPLEX)   src/traj_optimizer.cpp:31-166
 * The inputs of all agents are frozen before any agent plans (multi_sync_simulator.cpp:249-304),
 * so one batched launch is semantically identical to the reference's loop.
 *
 * Conventions: plain C, caller owns every host buffer, the context owns device memory and the
 * per-agent persistent state (optimiser's last trajectory, SFC history).  Functions return 0 on
 * success or a negative LSC_E* code; nothing throws across the boundary.  A context is not
 * thread-safe (the reference's caller is single-threaded).  There is NO CPU fallback: every entry
 * point that computes fails with LSC_ENODEV when no gfx950 device is usable.
 *
 * Layouts
 *   traj   float  [N][3][M*(n+1)]   axis-major control points, index k*M*6 + m*6 + i  (n=5; M=5: k*30 + m*6 + i)
 *                                   == TrajOptimizer's variable order (src/traj_optimizer.cpp:277)
 *   state  float  [N][9]            position, velocity, acceleration (octomap::point3d = float32)
 *   goal   float  [N][3]            agent.current_goal_position (output of goal planning)
 */
#ifndef LSC_PLANNER_AMD_H
#define LSC_PLANNER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Segments of a plan: M = (int)((horizon + 1e-9) / dt), src/traj_optimizer.cpp:9.  A build parameter of the library: liblsc_hip.so
 * plans M = 5 (dt 0.2, horizon 1.0: launch/simulation.launch:60-61 and every other shipped launch file), liblsc_hip_m4.so -- the same
 * sources compiled with -DLSC_SEGMENTS=4 -- plans M = 4 (dt 0.5, horizon 2.0: the C++ defaults of src/param.cpp:66-67).  A caller
 * built against the M = 4 library defines LSC_SEGMENTS=4 before this header; lsc_segments() says what a loaded library plans, and
 * lsc_create refuses a configuration whose horizon / dt is another number. */
#ifndef LSC_SEGMENTS
#define LSC_SEGMENTS 5
#endif
#define LSC_M LSC_SEGMENTS
#define LSC_DEG 5        /* Bernstein degree n (only n=5, phi=3 exist: traj_optimizer.cpp:190-207) */
#define LSC_NC 6
#define LSC_SEGV (LSC_M * LSC_NC)
#define LSC_NV (3 * LSC_SEGV)

#define LSC_OK 0
#define LSC_EINVAL (-1)   /* bad argument                                              */
#define LSC_ENODEV (-2)   /* no usable HIP device / kernel image (no CPU fallback)     */
#define LSC_ENOMEM (-3)
#define LSC_EHIP (-4)     /* HIP runtime error, see lsc_last_error()                   */
#define LSC_ESTATE (-5)   /* call order (e.g. tick before set_agents)                  */
#define LSC_ECOMM (-6)    /* RCCL error / librccl.so not loadable, see lsc_last_error() */

/* per-agent status written by a tick (PlanningReport analogue, include/sp_const.hpp) */
#define LSC_STATUS_OK 0          /* QP solved, trajectory replaced                                       */
#define LSC_STATUS_INFEASIBLE 1  /* solver failed: optimiser's previous trajectory kept, like the reference
                                    (exception swallowed, src/traj_planner.cpp:1553-1584)                */
/* (3 was "more LSC rows than the LDS row capacity" in round 1: such agents are now solved by a second pass with their
 *  rows in HBM, so the code no longer reaches the caller)                                                  */
#define LSC_STATUS_SFC_BLOCKED 4 /* seed box of the corridor touches an obstacle (the reference throws
                                    std::invalid_argument, corridor_constructor.hpp:35-38): stale trajectory kept */
#define LSC_STATUS_GOAL_CAPACITY 5 /* the goal planner's search outgrew a capacity: an OPEN row under goal_row_cap, a path
                                    longer than the LDS search's path buffer, g beyond 32767 steps, or the ray stack.  A row
                                    that outgrows its LDS capacity otherwise restarts the search with its rows in HBM, and
                                    grids too large for LDS are searched in HBM from the start (lsc_goal_storage).  Nothing
                                    is guessed, the stale trajectory is kept                                           */

typedef struct lsc_ctx lsc_ctx;

/* Param fields that reach the hot path (src/param.cpp:4-144, launch/testall_empty.launch:36-101) */
typedef struct {
    double dt;                 /* traj/dt                     0.2  */
    double control_weight;     /* opt/control_input_weight    0.01 */
    double terminal_weight;    /* opt/terminal_weight         1.0  */
    float  world_min[3];       /* mission world box (Mission::world_min/max, float32) */
    float  world_max[3];
    int    use_octomap;        /* world/use_octomap: adds the SFC rows                 */
    double world_resolution;   /* world/resolution (0.1).  With use_octomap, max(|world_min[k]|, |world_max[k]|) + world_resolution
                                  must stay below 256 m on every axis: lsc_set_distmap returns LSC_EINVAL otherwise.  From 256 m
                                  on, the float 1e-5 by which the reference nudges each float32 lattice sample of its corridor test
                                  (corridor_constructor.hpp:102-112) is less than half a float32 step and is rounded away; its
                                  samples then skip cells, which the corridor kernel's contiguous cell ranges do not reproduce.
                                  Also limited: 3400 steps of world_resolution per axis of the world box (the ticks return LSC_EINVAL) */
    int    device;             /* HIP device ordinal                                   */
    int    max_rows_per_cp;    /* LDS row capacity per control point of the first pass; 0 = min(N-1, 64) (lowered further if
                                  the 160 KB LDS of a workgroup demands it).  Not a limit of the problem: an agent with more
                                  rows is re-planned by the second pass with all its 27(N-1) rows in HBM */
    int    max_iters;          /* interior-point iteration cap; 0 = 50                 */
    int    prune;              /* 1 (default via lsc_default_config): drop LSC rows that are provably redundant inside
                                  the box each control point can reach under the velocity AND acceleration rows;
                                  2: the same with the velocity rows only; 0: keep all 27(N-1) rows;
                                  3: like 1 without the spatial pre-cull of far obstacles that large swarms use
                                  (identical rows and plans by construction; the switch exists for the test of that claim) */
    int    goal_mode;          /* mode/goal: 0 static (the goal input IS current_goal_position), 1 prior_based: the goal
                                  input is the desired goal and TrajPlanner::goalPlanningWithPriority runs on the
                                  device: fused into the plan kernel on maps without a distance field (where the grid
                                  search has no observable effect), a separate launch with use_octomap (priority rule,
                                  GridBasedPlanner's A* with the reference's tie-breaking, line-of-sight goal) */
    double goal_threshold;     /* plan/goal_threshold          0.1 */
    double priority_dist_threshold; /* plan/priority_dist_threshold 0.4 */
    double goal_radius;        /* plan/goal_radius             2.0 */
    double warm_start_mu;      /* interior-point start: > 0 warm start from the shifted previous plan, every row
                                  centred on this complementarity value (default 0.03), with the cold (Mehrotra)
                                  start as fallback; 0 = always cold start */
    double grid_resolution;    /* grid/resolution 0.3: cell of the goal planner's search grid (goal_mode 1 + use_octomap) */
    double grid_margin;        /* grid/margin     0.2: a cell is occupied when EDT(centre) < radius + grid_margin        */
    double horizon;            /* traj/horizon 1.0: M = (int)((horizon + 1e-9) / dt) must be the library's lsc_segments() (5, or 4
                                  in liblsc_hip_m4.so); anything else is refused by lsc_create instead of silently planning
                                  a different horizon                                                                       */
    int    goal_row_cap;       /* 0 = as large as LDS allows; > 0 a hard, smaller OPEN-row capacity of the goal search: a row
                                  that outgrows it gives LSC_STATUS_GOAL_CAPACITY (tests)                                  */
    /* ---- alternate planner modes.  Any of them changes the shape of the QP; such agents are solved by a
     * general dense kernel (csrc/lsc_general.hip) instead of the banded fast path -- same results, several times slower. */
    int    planner_mode;       /* mode/planner: 0 lsc (default), 1 bvc -- Buffered Voronoi Cells: TrajPlanner::generateBVC
                                  (src/traj_planner.cpp:1409-1440), prediction / initial trajectory = current position, no
                                  stop-at-horizon rows; empty maps only (generateSFC throws in BVC mode)                    */
    int    slack_mode;         /* SlackMode: 0 none (default), 1 dynamical_limit, 2 collision_constraint
                                  (src/traj_optimizer.cpp:306-326, 375-390, 455-457, 476-510)                               */
    double slack_collision_weight; /* opt/slack_collision_weight, 100000 in every launch file                               */
    int    n_constraint_segments;  /* opt/N_constraint_segments; -1 = all M segments carry collision / corridor rows        */
    double reset_threshold;    /* multisim/reset_threshold (0.15 in the launch files).  > 0 switches the reference's disturbance
                                  checks on (obstaclePredictionCheck / initialTrajPlanningCheck, src/traj_planner.cpp:866-878,
                                  1047-1061): an agent found farther than this from where its plan puts it has its prediction
                                  reset to its position, and -- for the rest of the mission, the reference never clears
                                  obs_slack_indices -- every row against it carries a slack variable.  0 (default) = off:
                                  identical results as long as the caller's states follow the plans, and no extra launch on
                                  the device-resident ticks                                                                 */
    double gap_tolerance;      /* interior point: duality gap <= gap_tolerance (1 + |objective|) at the optimum; 0 = 1e-9
                                  (CPLEX's barrier default, CPX_PARAM_BAREPCOMP, is 1e-8)                                   */
    int    world_dimension;    /* world/dimension (src/param.cpp:12; 3).  2 = planar world: the goal planner's grid is the single
                                  layer z = world_z_2d (src/grid_based_planner.cpp:82-85, 127-133, 199-215) and the QP has the
                                  x and y variables only -- dim = param.world_dimension, src/traj_optimizer.cpp:8: 60 variables
                                  (:264-266), cost, equalities, velocity / acceleration rows over k < dim (:330, 394, 469), no z
                                  term in the terminal cost, the corridor rows (Box::convertToLSCs(dim): 4 half-spaces,
                                  src/collision_constraints.cpp:37-59) and the collision rows (:367, 423, 450) -- while every
                                  planned control point gets z = world_z_2d (:87-90).  The whole swarm must sit in that plane
                                  (states and previous plans at z = (float)world_z_2d, which is what the reference's simulator
                                  produces: src/mission.cpp:88-112, src/traj_planner.cpp:304-314); the host-buffer ticks return
                                  LSC_EINVAL otherwise.  An agent whose solve fails keeps the optimiser's previous trajectory, which
                                  starts as zeros in the reference (src/traj_optimizer.cpp:16-19) and has its own z overridden on the
                                  next state callback; here that stale plan's z block starts at world_z_2d, so a failed first solve
                                  leaves the swarm in the plane.  0 is read as 3                                              */
    double world_z_2d;         /* world/z_2d (src/param.cpp:15; 1.0)                                                        */
    int    goal_search;        /* goal planner's grid search: 0 (default) the register-resident search whenever the grid admits it
                                  (at most 128 rows, (j, z) of a cell in 17 bits), with 32-bit search keys when their table fits
                                  LDS (else the double itself as key); 1 always the general search with the row bookkeeping in
                                  LDS; 2 the register-resident search with 64-bit keys; 3 the HBM search on any grid (OPEN rows at
                                  full capacity in a per-agent HBM workspace, row bookkeeping in LDS).  Grids whose search state does
                                  not fit LDS (more than 131071 cells, or cells plus 16-entry rows beyond LDS) take the HBM search
                                  whatever this says; its limits (W * A <= 65535 cells per row, at most 65535 rows) are checked by
                                  lsc_set_distmap.  Same paths in every case (tests)                                          */
    int    solver;             /* QP solver of the LSC fast path (the reference: CPLEX with RootAlgorithm Dual, src/traj_optimizer.cpp:42-56).
                                  1 (default via lsc_default_config): a dual active-set solve first -- Goldfarb-Idnani on the 39-unknown
                                  reduced problem from the unconstrained optimum; measured: at most 9 of the ~2 000 rows are active at an
                                  optimum and the slowest agent of a tick needs ~8-13 changes of the working set -- and the interior point
                                  only when that gives up (more than 12 active rows, dependent rows, an infeasible QP: the interior point
                                  then decides the status as before).  0: the interior point alone (rounds 1-4).  Same optimum within the
                                  parity tolerances either way; the second pass (rows in HBM) keeps solver 0.  2: a test mode -- the
                                  active-set solve runs and then hands EVERY agent to the interior point (exercises the hand-over path,
                                  where everything only the interior point needs is set up); results = the interior point's           */
    int    goal_lds_row_cap;   /* 0 = as large as LDS allows; > 0 lowers the LDS OPEN-row capacity of the goal search, but a row that
                                  outgrows it restarts the search with its rows in HBM instead of giving status 5 (tests of the
                                  restart; goal_row_cap > 0 takes precedence)                                               */
} lsc_config;

void lsc_default_config(lsc_config *cfg);

/* TrajPlanner ctor x N + TrajOptimizer ctor (src/traj_planner.cpp:4-73, src/traj_optimizer.cpp:4-25) */
lsc_ctx *lsc_create(const lsc_config *cfg);
void     lsc_destroy(lsc_ctx *ctx);
const char *lsc_last_error(const lsc_ctx *ctx);
/* Informational remark of lsc_create, "" when there is none -- e.g. that a slack mode was configured with the LSC planner and
 * fixed to none like TrajPlanner::checkPlannerMode does (src/traj_planner.cpp:445-448).  Never an error. */
const char *lsc_last_note(const lsc_ctx *ctx);
/* Segments M this library was built for (see LSC_SEGMENTS above). */
int lsc_segments(void);

/* Mission::agents (src/mission.cpp:60-130): radius, downwash, max_vel[3], max_acc[3], nominal_velocity.
 * Doubles, as in struct Agent (include/sp_const.hpp:153-165); an agent seen as somebody else's
 * obstacle has its radius/downwash rounded through float32 (dynamic_msgs::Obstacle), which the
 * reference fixture log/QPmodel.lp pins.  Resets the per-agent persistent state. */
int lsc_set_agents(lsc_ctx *ctx, int N, const double *radius, const double *downwash,
                   const double *max_vel /*[N][3]*/, const double *max_acc /*[N][3]*/, const double *nominal_vel);

/* Shard of agents [first, first+count) planned by this context (agent-sharded multi-GPU); default all.
 * count may be 0 (a rank without agents: its ticks are no-ops). */
int lsc_set_shard(lsc_ctx *ctx, int first, int count);

/* ---- dynamic obstacles: the mission's non-cooperating moving spheres -----------------------------
 * TrajPlanner::setObstacles with ObstacleType::DYNAMICOBSTACLE.  Every agent's obstacle list is then the other N - 1 agents in index
 * order followed by the K obstacles; rows against them (src/traj_planner.cpp:1336-1406) come from a constant-velocity prediction at
 * EVERY planner_seq (:838-846), the pair's downwash (r_a + dw_o r_o) / (r_a + r_o) (:1342-1345) and the agents' margins (:1388-1394);
 * goal planning does not see them (:553).
 * lsc_set_obstacles: after lsc_set_agents, 0 <= K <= LSC_OBSTACLES_MAX; radius / downwash [K] are rounded through float32, a downwash
 * of 0 reads as 1 (src/mission.cpp:164-166).  Replaces the obstacles and every buffer sized by N - 1 + K; the agents' persistent state
 * survives.  K = 0 removes them: the context is then one that never had any.  lsc_set_agents drops them.
 * lsc_obstacle_states: host [K][6], position | velocity, uploaded by the next tick on its stream in front of its launches.  A
 * device-resident tick on a stream of the caller's waits on the host for that upload (and for what the stream held before it):
 * callers that must not synchronise use the device form.
 * lsc_obstacle_states_device: the ticks read the caller's device buffer [K][6]; the caller orders its writes on the tick's stream.
 * A tick of a context with K > 0 and no states returns LSC_ESTATE.
 * Served: lsc_replan_tick (dumps [count][N-1+K][M][..]), lsc_tick_device, lsc_tick_device_fused, lsc_replan_tick_all on a one-rank
 * communicator, lsc_safety_ratio (agents only); empty maps and distance fields, both goal modes, every solver, M = 5 and 4.
 * Not built, LSC_EINVAL with the cause in lsc_last_error (at lsc_set_obstacles where known then, else at the tick; nothing is
 * enqueued): several ranks or a shard that is not the whole swarm; more agents than CUs; planner_mode bvc, a slack mode,
 * reset_threshold > 0 (lsc_set_obstacles only: lsc_set_obstacles_ex serves it); world_dimension 2; the batch ticks; lsc_fly_device /
 * lsc_flight_begin without motion models (lsc_obstacle_motion, below); lsc_phase_profile with enable 1;
 * lsc_dump_qp; K out of range; a radius that is not positive and finite; a state that is not finite.
 *
 * lsc_set_obstacles_ex: lsc_set_obstacles plus what the disturbance reset needs; it accepts a context with reset_threshold > 0 (LSC mode).
 * Once an agent has been seen off its plan the whole swarm plans through the alternate-mode solver, whose obstacle list is then the
 * N - 1 agents and the K spheres as well.  A sphere is never off a plan of its own (:838-846), but an agent that is, or ever was, holds
 * every obstacle in its slack set (initialTrajPlanningCheck, :1047-1061): the rows against a sphere then carry slack variables
 * (src/traj_optimizer.cpp:317-326, 455-456) and their margin is the sphere's whole predicted size plus the agent's radius (:1395-1400).
 * The predicted size (obstacleSizePredictionWithConstAcc, :880-919): with size_prediction != 0, over the first
 * M_u = int((uncertainty_horizon + 1e-9) / dt) segments the radius plus the degree-5 control points of 0.5 max_acc (dt (m + t))^2, from
 * M_u on the radius plus 0.5 max_acc (M_u dt)^2; with size_prediction == 0 the radius.  The host forms the table [K][M][6] once.
 * max_acc [K]: the obstacles' acceleration bound (the mission file's max_acc).  LSC_EINVAL, naming the obstacle: a max_acc that is
 * negative or not finite; an uncertainty_horizon that is negative, not finite or gives M_u > M (the reference writes past its array);
 * everything lsc_set_obstacles refuses, reset_threshold > 0 apart.  A context set through it serves what one set through
 * lsc_set_obstacles serves, at any reset_threshold; lsc_general_info and the lsc_last_note remark go by N - 1 + K. */
#define LSC_OBSTACLES_MAX 64
int lsc_set_obstacles(lsc_ctx *ctx, int K, const double *radius, const double *downwash);
int lsc_set_obstacles_ex(lsc_ctx *ctx, int K, const double *radius, const double *downwash, const double *max_acc, int size_prediction,
                         double uncertainty_horizon);
int lsc_obstacle_states(lsc_ctx *ctx, const float *pos_vel /* host [K][6] */);
int lsc_obstacle_states_device(lsc_ctx *ctx, const float *d_pos_vel /* device [K][6] */);

/* TrajPlanner::setDistMap (src/traj_planner.cpp:168): dense EDT, metres, [nx][ny][nz], copied to HBM.
 * key_min = octomap key of cell (0,0,0).  Only used when use_octomap. */
int lsc_set_distmap(lsc_ctx *ctx, const float *edt, int nx, int ny, int nz, const int key_min[3], double res);

/* Map input formats: reads an octomap binary tree (.bt) and builds the distance field that
 * MultiSyncSimulator::setOctomap creates with DynamicEDTOctomap(maxdist, tree, world_min, world_max, false)
 * (src/multi_sync_simulator.cpp:153-167).  *edt is malloc'ed [dims0][dims1][dims2] float metres: release it with
 * lsc_free_host.  Pure host code (no GPU needed). */
int lsc_edt_from_bt(const char *path, const float world_min[3], const float world_max[3], double maxdist, float **edt,
                    int dims[3], int key_min[3], double *res);
void lsc_free_host(void *p);

/* The map from occupancy, built and changed on the device (csrc/lsc_map.hip).
 *
 * lsc_occupancy_from_bt: the first half of lsc_edt_from_bt -- the .bt file's occupied leaves on the grid of the world box.  *occ is
 *   malloc'ed [dims0][dims1][dims2] bytes, 1 occupied, 0 free: release it with lsc_free_host.  Pure host code.
 * lsc_set_occupancy: the context's map becomes the occupancy grid occ (host, [nx][ny][nz], non-zero: occupied), copied to HBM.  The
 *   distance field lsc_edt_from_bt(maxdist) would give, the corridor kernel's integral images and the goal planner's static occupancy are
 *   built from it ON THE DEVICE, to the same bytes as lsc_set_distmap builds them from that field on the host.  Refuses what
 *   lsc_set_distmap refuses, and LSC_EINVAL with the cause: a dimension below 1; maxdist not positive and finite;
 *   (int)(maxdist / res + 1) > 127.  Allocates everything an update needs; synchronises.
 *   lsc_set_agents afterwards keeps the map and rebuilds the per-radius products on the device.  lsc_set_distmap afterwards replaces
 *   the map and drops the occupancy.
 * lsc_map_update: n_boxes (0 .. LSC_MAP_BOXES_MAX) boxes of field cells, boxes[i] = {x0, y0, z0, x1, y1, z1}, lo inclusive, hi
 *   exclusive, are set to values[i] (0 free, 1 occupied) in call order -- where boxes overlap the later one wins -- and the whole map is
 *   rebuilt: the edit and the rebuild are enqueued on hip_stream (NULL: the context's own stream), nothing is allocated, no pointer a
 *   tick, a batch or a flight reads changes, and the host does not wait.  A tick enqueued behind it on that stream plans on the new map;
 *   the caller orders it against ticks on other streams.  The boxes are copied before the call returns.
 *   flags: LSC_MAP_REGROW_CORRIDORS -- every agent's next tick regrows all its corridor boxes from its current position (the reference's
 *   flag_initialize_sfc).  Without it boxes grown before the change stay as grown: the reference never re-checks a box either.
 *   LSC_EINVAL with the cause (nothing is enqueued): n_boxes out of range; a box outside the field or with lo >= hi; a value above 1; an
 *   unknown flag.  LSC_ESTATE: the context's map is not a device occupancy.
 * lsc_map_update_device: the same with a whole grid: d_occ (device, [nx][ny][nz] of the context's field) replaces the occupancy.
 * lsc_map_read: diagnostics; copies only, synchronises the device.  `which` and the exact size in bytes of `out`:
 *   LSC_MAP_DIMS            int[LSC_MAP_DIMS_INTS]: nx, ny, nz, n_radii, H, W, A (0 when the context plans no goals on the map), 1 when
 *                           the map is a device occupancy
 *   LSC_MAP_OCCUPANCY       unsigned char [nx][ny][nz]           (LSC_ESTATE on a map from lsc_set_distmap)
 *   LSC_MAP_EDT             float [nx][ny][nz]: the device buffer the goal planner's castRay reads; on a map from lsc_set_distmap whose
 *                           context plans no goals on it (no such buffer: the corridor kernel reads the images) the host's copy
 *   LSC_MAP_INTEGRAL        int [n_radii][nx+1][ny+1][nz+1]      (distinct radii in order of first appearance among the agents)
 *   LSC_MAP_GOAL_OCCUPANCY  unsigned char [n_radii][H W A], index H W k + W i + j
 *   It serves maps from lsc_set_distmap too. */
#define LSC_MAP_BOXES_MAX 64
#define LSC_MAP_REGROW_CORRIDORS 1
#define LSC_MAP_DIMS 0
#define LSC_MAP_OCCUPANCY 1
#define LSC_MAP_EDT 2
#define LSC_MAP_INTEGRAL 3
#define LSC_MAP_GOAL_OCCUPANCY 4
#define LSC_MAP_DIMS_INTS 8
int lsc_occupancy_from_bt(const char *path, const float world_min[3], const float world_max[3], unsigned char **occ, int dims[3],
                          int key_min[3], double *res);
int lsc_set_occupancy(lsc_ctx *ctx, const unsigned char *occ /* host */, int nx, int ny, int nz, const int key_min[3], double res,
                      double maxdist);
int lsc_map_update(lsc_ctx *ctx, int n_boxes, const int *boxes /* [n][6] */, const unsigned char *values /* [n] */, int flags,
                   void *hip_stream);
int lsc_map_update_device(lsc_ctx *ctx, const unsigned char *d_occ, int flags, void *hip_stream);
int lsc_map_read(lsc_ctx *ctx, int which, void *out, size_t bytes);

/* One replan tick, host buffers in and out (H2D + kernels + D2H inside).
 *   planner_seq : TrajPlanner::planner_seq AFTER its increment in plan() (1 on the first tick):
 *                 < 2 selects the current-velocity prediction (src/traj_planner.cpp:830-833, 998-1000)
 *   state/goal/prev_traj : all N agents (prev_traj = every agent's getTraj() of the previous tick)
 *   out_traj/out_cost/out_status/out_iters : the shard's agents only, [count]...
 *   out_lsc_normal [count][N-1][M][3] float, out_lsc_d [count][N-1][M][n+1] double, out_sfc [count][M][6]
 *                 : optional (NULL to skip) dense constraint dumps (CollisionConstraints::getLSC/getSFC). */
int lsc_replan_tick(lsc_ctx *ctx, const float *state, const float *goal, const float *prev_traj, int planner_seq,
                    float *out_traj, double *out_cost, int *out_status, int *out_iters,
                    float *out_lsc_normal, double *out_lsc_d, float *out_sfc);

/* ---- device-resident stepping (no host round trip inside a tick) -------------------------------
 * The caller (e.g. a torch tensor) owns device buffers and the stream; pointers are device pointers.
 *   d_state [N][9], d_goal [N][3], d_traj_prev [N][3][30] : read
 *   d_traj_next [N][3][30] : the shard's rows [first,first+count) are written (full table so that an
 *                            all-gather can run in place across ranks)
 *   d_cost [N] double, d_status [N] int, d_iters [N] int : shard's entries written                */
int lsc_tick_device(lsc_ctx *ctx, const float *d_state, const float *d_goal, const float *d_traj_prev,
                    int planner_seq, float *d_traj_next, double *d_cost, int *d_status, int *d_iters,
                    void *hip_stream);

/* Same tick with MultiSyncSimulator::update()'s ideal-state step fused into the launch: additionally writes
 * d_state_next [N][9] rows of the shard = the agent's state at t = dt on its new plan (what lsc_propagate_device
 * computes).  With one GPU a whole tick is then a single kernel launch; d_state and d_state_next must be different
 * buffers (every workgroup reads all current states). */
int lsc_tick_device_fused(lsc_ctx *ctx, const float *d_state, const float *d_goal, const float *d_traj_prev,
                          int planner_seq, float *d_traj_next, float *d_state_next, double *d_cost, int *d_status,
                          int *d_iters, void *hip_stream);

/* ---- several independent swarms on one GPU: the mission list as a batch axis ------------------------------
 * The reference's node flies a directory of missions back to back (src/multi_sync_simulator_node.cpp:43-70, src/param.cpp:106-122;
 * launch/testall_*.launch: 30 missions per swarm size).  A 64-agent swarm is 64 workgroups on a 256-CU chip, so up to LSC_BATCH_MAX
 * swarms -- one context each, all on one device -- are planned by ONE launch: lsc_tick_device_fused for every ctx[i] with its own
 * buffers and its own planner_seq[i], bit-identical results.  Every array argument has n entries (arrays of device pointers, held on
 * the host).  Maps with a distance field batch too (forest and office grids, octomap and empty-map swarms, static and grid goals in one
 * batch): the tick is then the goal-search batch (one launch per search instantiation among the contexts that plan goals), the corridor
 * batch, the plan batch.  The contexts must not be sharded, have at most one agent per CU each, all have or all lack the alternate-mode
 * hooks (reset_threshold > 0 / BVC / slack), be all planar or all 3-D, and have no goal trace or goal profiling on; a context with
 * use_octomap needs lsc_set_distmap.  LSC_EINVAL / LSC_ESTATE otherwise, with the reason in lsc_last_error(ctx[0]).  With lsc_set_timing
 * the launches are timed on ctx[0]: goal search under `which` 3, corridor update under 4, planning under 0. */
#define LSC_BATCH_MAX 8
int lsc_tick_device_fused_batch(lsc_ctx *const *ctx, int n, const float *const *d_state, const float *const *d_goal,
                                const float *const *d_traj_prev, const int *planner_seq, float *const *d_traj_next,
                                float *const *d_state_next, double *const *d_cost, int *const *d_status, int *const *d_iters,
                                void *hip_stream);

/* Host-buffer form of the same batched tick, what a simulator flying several missions in lockstep calls: for every ctx[i]
 * lsc_replan_tick's checks and host work on its own arrays (state[i], goal[i], prev_traj[i], planner_seq[i]), then one upload per
 * context, ONE batched tick, one download per context and one synchronisation, all on ctx[0]'s stream.  out_traj[i], out_cost[i],
 * out_status[i], out_iters[i] (out_iters may be NULL, or an entry of it) are bit-identical to lsc_replan_tick on ctx[i] alone;
 * lsc_last_goals(ctx[i]) is valid afterwards.  No constraint dumps in this form. */
int lsc_replan_tick_batch(lsc_ctx *const *ctx, int n, const float *const *state, const float *const *goal, const float *const *prev_traj,
                          const int *planner_seq, float *const *out_traj, double *const *out_cost, int *const *out_status,
                          int *const *out_iters);

/* ---- agent-sharded multi-GPU: one context (= one process, one GPU) per rank ---------------------
 * The reference's exchange point is MultiSyncSimulator::update (src/multi_sync_simulator.cpp:297-303), where every
 * agent receives every other agent's previous trajectory.  With the swarm partitioned over `world_size` ranks that
 * hand-over is ONE RCCL all-gather per tick, in place on the trajectory table (xGMI on a node).  The table is padded to
 * table_rows = shard_rows * world_size rows, shard_rows = ceil(N / world_size); rank r plans agents
 * [r*shard_rows, min((r+1)*shard_rows, N)) -- the trailing ranks of a ragged split own fewer (possibly zero) agents.
 *
 *   lsc_comm_unique_id : rank 0 creates the rendezvous token (ncclGetUniqueId) and ships it to the other ranks by any
 *                        means (a file, MPI, torch.distributed's store ...)
 *   lsc_comm_init      : collective over all ranks, between lsc_create and lsc_set_agents (which then sets the shard
 *                        and pads the context's tables); librccl.so is bound at run time (the copy already mapped into
 *                        the process, else the system's)
 *   lsc_comm_info      : world size, rank, shard_rows, table_rows                                                    */
#define LSC_COMM_ID_BYTES 128
int lsc_comm_unique_id(unsigned char id[LSC_COMM_ID_BYTES]);
int lsc_comm_init(lsc_ctx *ctx, int world_size, int rank, const unsigned char id[LSC_COMM_ID_BYTES]);
int lsc_comm_info(const lsc_ctx *ctx, int *world_size, int *rank, int *shard_rows, int *table_rows);

/* One tick of a sharded swarm, device-resident: lsc_tick_device for the rank's agents, the in-place all-gather of
 * d_traj_next (float [table_rows][90]: padded!), then the ideal next state of ALL N agents into d_state
 * (lsc_propagate_device) -- i.e. d_state is read by the tick and overwritten for the next one.  d_cost / d_status /
 * d_iters: the rank's entries only.  Everything is enqueued on hip_stream; no host synchronisation. */
int lsc_tick_device_sharded(lsc_ctx *ctx, float *d_state, const float *d_goal, const float *d_traj_prev, int planner_seq,
                            float *d_traj_next, double *d_cost, int *d_status, int *d_iters, void *hip_stream);

/* Multi-GPU form of lsc_replan_tick (host buffers): every rank passes the same inputs for all N agents, plans its
 * shard, and receives the outputs of ALL N agents (trajectories, costs, statuses, iterations and -- optional --
 * current_goal_position are all-gathered in one RCCL group).  What a replicated MultiSyncSimulator per rank calls. */
int lsc_replan_tick_all(lsc_ctx *ctx, const float *state, const float *goal, const float *prev_traj, int planner_seq,
                        float *out_traj /*[N][3][30]*/, double *out_cost /*[N]*/, int *out_status /*[N]*/,
                        int *out_iters /*[N] or NULL*/, float *out_goal /*[N][3] or NULL*/);

/* MultiSyncSimulator::update()'s ideal-state step on device: state[qi] = traj[qi] evaluated at t = dt
 * (getFutureStateMsg -> getStateFromControlPoints, include/polynomial.hpp:63-97).  All N agents. */
int lsc_propagate_device(lsc_ctx *ctx, const float *d_traj, float *d_state, void *hip_stream);

/* MultiSyncSimulator::savePlanningResult's agent-agent accounting (src/multi_sync_simulator.cpp:446-503) on the device, for
 * the plans of the last lsc_replan_tick / lsc_replan_tick_all.  times[n_times] (n_times <= 64): seconds into the plan at which
 * the swarm is sampled (the reference: 0, multisim_record_time_step, ... below multisim_time_step).  The context must hold the new
 * plans of ALL N agents: the last tick was lsc_replan_tick_all, or lsc_replan_tick of a context whose shard is the whole swarm
 * (LSC_ESTATE otherwise -- the partners' rows would be stale).  For every sample and
 * every agent of this context's shard, the downwash-scaled distance to every other agent over the sum of the two radii
 * (distBetweenAgents, include/util.hpp:225-229): out_ratio[n_times][count] = the minimum over the partners,
 * out_partner[n_times][count] = the first partner attaining it (what the reference's collision message names); either may be
 * NULL.  *out_min = the minimum over everything -- over ALL ranks when the context has a communicator (one ncclAllReduce(min);
 * collective: every rank must call it).  The reference walks all N^2 pairs on the host after every tick. */
int lsc_safety_ratio(lsc_ctx *ctx, const double *times, int n_times, double *out_ratio, int *out_partner, double *out_min);

/* ---- K closed-loop ticks per call on the device, with the mission's bookkeeping --------------------------------
 * lsc_fly_device enqueues n_ticks fused ticks on one stream with no host work between them; with a flight log open, one small record
 * launch behind every tick appends MultiSyncSimulator's per-tick accounting to the log (csrc/lsc_flight.hip, csrc/lsc_flight.hpp), and
 * the host reads the log once per batch (lsc_flight_read).  Plain stream order: no persistent kernel, no device-wide barrier, no graph.
 *
 * One log row per tick.  The summary is always written; the other parts are chosen by `what`:
 *   LSC_FLIGHT_SAMPLES  float [n_times][N][9]: position, velocity, acceleration of every agent on its NEW plan at every record time
 *                       (getStateFromControlPoints, include/polynomial.hpp:63-97: what the result CSV holds);
 *   LSC_FLIGHT_SAFETY   double ratio [n_times][N], int partner [n_times][N]: exactly lsc_safety_ratio's out_ratio / out_partner
 *                       (savePlanningResult, src/multi_sync_simulator.cpp:446-503); 1e300 / -1 for an agent without a partner;
 *   LSC_FLIGHT_AGENTS   double cost [N], int status [N], float end [N][3] (the new plan's last control point).
 *
 * Row j describes tick j's INPUT state and OUTPUT plan.  The reference's loop tests isFinished on the state the previous update() set
 * (src/multi_sync_simulator.cpp:358-380), so a mission is over BEFORE tick r + 1, where r is the first row with unmet == 0: the rows
 * beyond r were flown for nothing and the caller discards them. */
#define LSC_FLIGHT_SAMPLES 1
#define LSC_FLIGHT_SAFETY  2
#define LSC_FLIGHT_AGENTS  4
typedef struct {
    int capacity_ticks;        /* rows of the log */
    int n_times;               /* 1..64 record times per tick */
    double times[64];          /* seconds into the new plan, inside the horizon (t == M dt: last segment, local parameter 1) */
    int what;                  /* LSC_FLIGHT_* bits */
} lsc_flight_config;
typedef struct {
    int planner_seq;
    int unmet;                 /* agents whose INPUT position is farther than goal_threshold from the goal input (isFinished) */
    int end_unmet;             /* the same test on the new plan's end point (checkDeadlock) */
    int moved;                 /* agents whose end point is >= SP_EPSILON_FLOAT from the end point of the previous plan; every agent at
                                  planner_seq 1 (src/traj_planner.cpp:396-409) */
    int n_status[6];           /* agents per status code 0..5 */
    double min_ratio;          /* the swarm's minimum ratio over all record times; 1e300 without LSC_FLIGHT_SAFETY */
    int pad[4];
} lsc_flight_tick;             /* 64 bytes */

/* Host only (no device): Bernstein weights w5 [n_times][6], w4 [n_times][5], w3 [n_times][4] (degrees 5, 4, 3: position, velocity,
 * acceleration) and the segment seg [n_times] of each time, in the reference's own expression nChoosek * pow(t, i) * pow(1 - t, n - i)
 * at t = time / dt - seg -- the record kernel only repeats multiply-adds.  Any output may be NULL.  LSC_EINVAL: n_times outside 1..64,
 * a time below 0 or beyond the horizon (lsc_segments() * dt, which itself is the last segment at local parameter 1). */
int lsc_flight_weights(double dt, const double *times, int n_times, double *w5, double *w4, double *w3, int *seg);
/* Host only: bytes of one log row -- 64 (summary) + 8 n_times N + 4 n_times N (safety) + 36 n_times N (samples) + 24 N (agents),
 * each part only when its bit is set, rounded up to a multiple of 64.  0 for arguments out of range. */
size_t lsc_flight_row_bytes(int N, int n_times, int what);
/* Opens a log of cfg->capacity_ticks rows: allocates it, initialises the summaries, uploads the weights.  A log that was open is
 * replaced.  LSC_EINVAL (reason in lsc_last_error): a context with a communicator, a shard that is not the whole swarm, goal trace or goal
 * profiling on, n_times outside 1..64, a time outside the horizon, capacity below 1.  lsc_set_agents drops the log (it is then closed). */
int lsc_flight_begin(lsc_ctx *ctx, const lsc_flight_config *cfg);
/* The log is empty again: waits for what was flown, re-initialises the summaries on the context's stream and waits for that. */
int lsc_flight_reset(lsc_ctx *ctx);
int lsc_flight_end(lsc_ctx *ctx);
/* n_ticks closed-loop ticks: tick j (0-based) is exactly
 *   lsc_tick_device_fused(ctx, d_state[j & 1], d_goal, d_traj[j & 1], first_planner_seq + j, d_traj[(j + 1) & 1], d_state[(j + 1) & 1], ...)
 * -- goal search, corridor, neighbour lists, second pass and hand-over included -- followed, when a log is open, by one record launch
 * (timed under which = 6 of lsc_kernel_time_ms).  Nothing else is enqueued and the host does not wait.  d_cost / d_status / d_iters hold
 * the last tick's values afterwards.  With no log open it only flies.  n_ticks == 0 is LSC_OK and enqueues nothing.  Flying past the
 * log's capacity is refused before anything is enqueued (LSC_ESTATE): the log neither wraps nor overwrites rows.  LSC_EINVAL as for
 * lsc_flight_begin's context conditions. */
int lsc_fly_device(lsc_ctx *ctx, float *const d_state[2], const float *d_goal, float *const d_traj[2], int first_planner_seq,
                   int n_ticks, double *d_cost, int *d_status, int *d_iters, void *hip_stream);
/* Rows first_tick .. first_tick + n_ticks - 1 of the log (LSC_EINVAL when they were not all flown), after synchronising the stream last
 * flown on.  summary [n_ticks]; samples [n_ticks][n_times][N][9]; ratio, partner [n_ticks][n_times][N]; cost, status [n_ticks][N];
 * end [n_ticks][N][3].  NULL = skip; a part that is not recorded must be NULL (LSC_EINVAL). */
int lsc_flight_read(lsc_ctx *ctx, int first_tick, int n_ticks, lsc_flight_tick *summary, float *samples, double *ratio,
                    int *partner, double *cost, int *status, float *end);

/* ---- The goal stage: patrol missions and the right-hand goal rule on the device (csrc/lsc_mission.hip) ----
 * The first lines of TrajPlanner::goalPlanning (src/traj_planner.cpp:477-509), which sit in front of the goal mode: a PATROLLING agent
 * that is strictly closer than goal_threshold to its desired goal swaps desired goal and start (:479-485); in GOBACK every agent's
 * desired goal is the mission's start, on every tick (:486-490); with the right-hand rule a deadlocked agent (isDeadlock, :1733-1740:
 * planner_seq > seq_threshold, slower than velocity_threshold, farther than goal_threshold from its desired goal) plans towards
 * pos + (desired - pos) x (0, 0, 1) (:528-538).  All of it is one small launch in front of everything else a tick enqueues, reading
 * the tick's INPUT state; the neighbour lists, the goal search, the corridor and the plan kernel are handed its table in place of the
 * caller's goal pointer and are otherwise untouched.
 *
 * lsc_mission_open(ctx, start, goal): host float [N][3] each; opens (or replaces) the context's mission state -- desired = goal,
 *   start = start, legs = 0, planner state LSC_MISSION_GOTO.  lsc_set_agents drops it.
 * WHILE A MISSION STATE IS OPEN THE GOAL ARGUMENT OF EVERY TICK IS IGNORED (it may be NULL): the ticks plan towards the state's
 *   desired goals, and the record launch of lsc_fly_device tests unmet / end_unmet against the desired goals of that tick -- in GOBACK
 *   `unmet == 0` therefore means "all home" (isFinished, src/multi_sync_simulator.cpp:369-371).  The flight log's row format is unchanged.
 * lsc_mission_set_state(ctx, LSC_MISSION_*): startPatrolCallback / stopPatrolCallback (src/multi_sync_simulator.cpp:700-708), between
 *   ticks (host side only: the next tick's stage reads it).  In GOTO the stage changes nothing.
 * lsc_mission_read(ctx, desired, start, legs): float [N][3], float [N][3], int [N] (swaps made per agent since lsc_mission_open); any
 *   may be NULL.  Synchronises the device.
 * lsc_mission_close(ctx): the context is again what it was before lsc_mission_open, bit for bit.
 * lsc_set_goal_rule(ctx, rule, seq_threshold, velocity_threshold): LSC_GOAL_RULE_CONFIG (lsc_config.goal_mode alone decides; the
 *   thresholds are not read) or LSC_GOAL_RULE_RIGHT_HAND (mode/goal right_hand; src/param.cpp:79-80: 5 and 0.1).  The rule's goal is what
 *   the tick behind the stage plans towards as goal_mode 0, so the context must have been created with goal_mode 0; lsc_last_goals returns
 *   the rule's goals.  The desired goals are the mission state's when one is open, else the tick's goal argument.  A context setting
 *   that outlives lsc_set_agents.
 * Served: lsc_replan_tick, lsc_tick_device, lsc_tick_device_fused, lsc_fly_device; empty maps and distance fields, both solvers, planar
 *   worlds, BVC / slack contexts, contexts with dynamic obstacles.  Refused with LSC_EINVAL, the cause in lsc_last_error and nothing
 *   enqueued, while a mission state is open or the right-hand rule is set: a communicator of several ranks, a shard that is not the
 *   whole swarm, the batch ticks, goal trace / goal profiling.
 * A context that never opens a mission state or sets the rule enqueues exactly what it enqueued before these calls existed.
 * Known limit: under goal_mode 1 the reference's priority rule reads the OTHER agents' goals as the simulator's update() froze them
 *   (src/multi_sync_simulator.cpp:291), so on the tick an agent swaps, the others still see its old goal (src/traj_planner.cpp:554-562);
 *   here the swap is visible to every agent in the same tick -- what a host that rewrites the goal table between ticks gets.
 *   goal_mode 0 and the right-hand rule are exact. */
#define LSC_MISSION_GOTO   0
#define LSC_MISSION_PATROL 1
#define LSC_MISSION_GOBACK 2
#define LSC_GOAL_RULE_CONFIG     0
#define LSC_GOAL_RULE_RIGHT_HAND 1
int lsc_mission_open(lsc_ctx *ctx, const float *start, const float *goal);
int lsc_mission_set_state(lsc_ctx *ctx, int planner_state);
int lsc_mission_read(lsc_ctx *ctx, float *desired, float *start, int *legs);
int lsc_mission_close(lsc_ctx *ctx);
int lsc_set_goal_rule(lsc_ctx *ctx, int rule, int seq_threshold, double velocity_threshold);

/* ---- Motion models: the context moves its dynamic obstacles itself (csrc/lsc_obstacles.hip, csrc/lsc_obstacle_motion.hpp) ----
 * getObstacle(t) of include/obstacle.hpp for the three types whose motion is a closed form of the time -- straight (:123-173), spin
 * (:68-121), multisim_patrol (:175-231) -- as one launch of one workgroup in front of everything else a tick enqueues (in front of the
 * goal stage): it writes the [K][6] states the plan kernel reads.  The arithmetic is in doubles, rounded to float32 at the store.
 * Straight and patrol are the bits of the host's statements (+ - x / sqrt and comparisons only); spin goes through the device's double
 * sin / cos and may differ from the host by one float32 step of the rounded result.  OPT-IN: a context that never installs models
 * enqueues exactly what it enqueued before these calls existed, and every refusal of a context with obstacles stays.
 *
 * lsc_obstacle_motion(ctx, K, models): after lsc_set_obstacles, K equal to its K; K = 0 or models NULL removes the models (the context
 *   is then one that was only given lsc_set_obstacles; states fed before are forgotten).  points: straight { start, goal }; spin { axis
 *   position, axis orientation of any length, start }; multisim_patrol 2 to LSC_OBSTACLE_POINTS_MAX waypoints, walked round and round (a
 *   repeated waypoint is a leg of no length and is stepped over).  The per-leg constants are formed once, here.  Installing synchronises
 *   the device.  lsc_set_obstacles and lsc_set_agents drop the models.
 *   LSC_ESTATE: no obstacles are set.  LSC_EINVAL, naming the obstacle: K differs from lsc_set_obstacles'; an unknown kind; a wrong
 *   number of points; a point or speed that is not finite; a speed that is not positive; a spin whose start lies on its axis; a patrol
 *   whose waypoints span no distance.
 * lsc_obstacle_clock(ctx, start, now, step): the simulator's pair of statements.  Every tick that runs the stage evaluates the models at
 *   now - start (one double subtraction on the host) and then does now += step; a refused tick does not advance the clock.
 *   lsc_fly_device forms one time per enqueued tick the same way.  LSC_EINVAL: a value that is not finite.  Models without a clock:
 *   the tick returns LSC_ESTATE.  A tick so late that a patrol's walk would step over more than 65 536 legs (time / shortest positive
 *   leg time) returns LSC_EINVAL naming the obstacle, in front of everything it would enqueue.
 * lsc_obstacle_clock_read(ctx, now): LSC_ESTATE without a clock.
 * lsc_obstacle_states_read(ctx, pos_vel): host [K][6], the states the last tick read, whoever wrote them (the stage, lsc_obstacle_states,
 *   or the caller's device buffer).  Synchronises the device.  LSC_ESTATE: no obstacles, or no states yet.
 * lsc_obstacle_positions_read(ctx, pos): host double [K][3], the positions of the last tick's stage BEFORE the rounding to float32 (their
 *   float32 is what lsc_obstacle_states_read returns): for straight and patrol the host's doubles bit for bit, which is what a
 *   simulator that printed the host's doubles before needs to write the same file.  Synchronises.  LSC_ESTATE without models.
 * With models installed lsc_obstacle_states and lsc_obstacle_states_device return LSC_ESTATE (the context moves its obstacles itself:
 *   remove the models first).
 * The flight loop: a context WITH models may lsc_flight_begin / lsc_fly_device (without them the refusal of the obstacle block above
 *   stands, with its message).  lsc_flight_begin then allocates the obstacle track next to the log: capacity_ticks rows of
 *     double min_ratio | int below_one | int pad | float states [K][6] | double ratio [T][N] | int partner [T][N] | (to an 8 B boundary)
 *     double positions [K][3]                                                                                       (rounded up to 64 B)
 *   written by one more launch behind the record launch of every tick: ratio = the minimum over the obstacles of |sample position -
 *   obstacle position| (float32 difference and squared norm, double root) / (r_a + (double)(float) r_o), savePlanningResult's obstacle
 *   ratio (src/multi_sync_simulator.cpp:480-500: no downwash, the obstacle where the TICK put it at every record time); partner = the
 *   first obstacle attaining it; min_ratio their minimum (1e300 at reset), below_one how many are below 1.  The flight row, its `what`
 *   bits, lsc_flight_read and lsc_flight_row_bytes are unchanged; the track is released with the log (lsc_flight_end, lsc_set_agents)
 *   and reset with it (lsc_flight_reset).  lsc_fly_device with an open log whose track was sized for another K, or that was opened before
 *   the models were installed (or after they were removed), returns LSC_ESTATE and enqueues nothing.
 * lsc_flight_obstacles_read(ctx, first_tick, n_ticks, min_ratio [n], below_one [n], pos_vel [n][K][6], ratio [n][T][N], partner
 *   [n][T][N]): any may be NULL; synchronises the stream last flown on.  LSC_ESTATE: no log with a track is open.  LSC_EINVAL: rows that
 *   were not all flown.
 * lsc_flight_obstacle_positions_read(ctx, first_tick, n_ticks, pos [n][K][3]): the rows' positions in doubles (lsc_obstacle_positions_read
 *   of each tick); refusals as lsc_flight_obstacles_read.
 * Timing: the stage's and the track's launches belong to no timed group of lsc_set_timing (which = 6 stays the record launch alone).
 * Every other refusal of a context with dynamic obstacles stands: shards, communicators of several ranks, more agents than CUs, BVC,
 *   slack modes, reset_threshold > 0, planar worlds, the batch ticks, lsc_phase_profile, lsc_dump_qp.  A mission state and the right-hand
 *   rule are served together with moving obstacles; a tick's stages run in the order obstacles, mission, goal, corridor, plan. */
#define LSC_OBSTACLE_POINTS_MAX 8
#define LSC_OBSTACLE_STRAIGHT 0
#define LSC_OBSTACLE_SPIN     1
#define LSC_OBSTACLE_PATROL   2
typedef struct {
    int kind;                                        /* LSC_OBSTACLE_* */
    int n_points;
    double speed;
    double points[LSC_OBSTACLE_POINTS_MAX][3];
} lsc_obstacle_model;
int lsc_obstacle_motion(lsc_ctx *ctx, int K, const lsc_obstacle_model *models);
int lsc_obstacle_clock(lsc_ctx *ctx, double start, double now, double step);
int lsc_obstacle_clock_read(lsc_ctx *ctx, double *now);
int lsc_obstacle_states_read(lsc_ctx *ctx, float *pos_vel /* host [K][6] */);
int lsc_obstacle_positions_read(lsc_ctx *ctx, double *pos /* host [K][3] */);
int lsc_flight_obstacle_positions_read(lsc_ctx *ctx, int first_tick, int n_ticks, double *pos /* host [n][K][3] */);
int lsc_flight_obstacles_read(lsc_ctx *ctx, int first_tick, int n_ticks, double *min_ratio, int *below_one, float *pos_vel,
                              double *ratio, int *partner);

/* ---- Chasing and gaussian obstacles: motion models with state or history of their own (csrc/lsc_obstacle_motion.hpp) ----
 * chasing (include/obstacle.hpp:234-328, fed by updateObstacles of include/obstacle_generator.hpp:102-118): a potential-field pursuer.
 *   Every tick it accelerates towards its target AGENT's position in the tick's input state, is pushed away from the other obstacles
 *   where the PREVIOUS tick put them (before the first tick of an installation: positions 0 and radii 0, the generator's
 *   default-constructed obstacles), clamps acceleration (max_acc - 0.01) and velocity (max_vel) and integrates over dt = t - t_last.
 *   radius: the chaser's own radius as the mission file holds it (a double); the others' radii are lsc_set_obstacles' float32.
 * gaussian (:330-435): a random-acceleration walker; given its acceleration history, an INPUT here, a function of t that reads
 *   floor((t + 1e-5) / acc_update_cycle) + 1 history entries.
 * lsc_obstacle_motion_ex(ctx, K, models, n_chasers, chasers, n_walkers, walkers): lsc_obstacle_motion for kinds 0 to 2; models[o].kind
 *   LSC_OBSTACLE_CHASING / LSC_OBSTACLE_GAUSSIAN (n_points, speed and points are not read) says that obstacle o has a chaser / walker
 *   record.  Every such obstacle must be named by exactly one record of its kind, and no other obstacle by any.  Installing resets every
 *   chaser to start, velocity 0, t_last 0.  A context with at least one such model launches ONE stage that serves all five kinds, instead
 *   of the closed forms' stage (read - barrier - write: a chaser sees every other obstacle where the previous tick put it).
 *   LSC_EINVAL naming the obstacle: a value that is not finite; max_vel <= 0; a chaser's max_acc <= 0.01; a target outside 0 .. N - 1;
 *   a walker's acc_update_cycle <= 0, n_acc < 1 or n_acc > 4096; records that do not match the kinds.
 *   lsc_obstacle_motion given kind 3 or 4 returns LSC_EINVAL naming this call.
 * Ticks, refused in front of everything they would enqueue (LSC_EINVAL naming the obstacle; neither the clock nor any state advances):
 *   with a chaser, a clock time now - start below the chasers' last evaluated time; with a walker, a time that needs more than n_acc
 *   entries.  lsc_fly_device checks every one of its ticks first; its chasers read tick j's own state buffer.
 * lsc_obstacle_chaser_states_read(ctx, state): host double [K][7], position | velocity | t_last of every chaser as the last tick left
 *   it, NaN rows for obstacles that are no chasers.  Synchronises the device.  LSC_ESTATE without chasers.
 * The clock, the track, lsc_obstacle_states_read / lsc_obstacle_positions_read and every refusal above are as for kinds 0 to 2. */
#define LSC_OBSTACLE_CHASING  3
#define LSC_OBSTACLE_GAUSSIAN 4
typedef struct {
    int obstacle, target;                            /* index of the obstacle; index of the agent it chases */
    double start[3], radius, max_vel, max_acc, gamma_target, gamma_obs;
} lsc_obstacle_chaser;
typedef struct {
    int obstacle, n_acc;
    double start[3], initial_vel[3], max_vel, acc_update_cycle;
    const double *acc;                               /* host [n_acc][3], copied */
} lsc_obstacle_walker;
int lsc_obstacle_motion_ex(lsc_ctx *ctx, int K, const lsc_obstacle_model *models, int n_chasers, const lsc_obstacle_chaser *chasers,
                           int n_walkers, const lsc_obstacle_walker *walkers);
int lsc_obstacle_chaser_states_read(lsc_ctx *ctx, double *state /* host [K][7] */);

/* Dense LSC sweep only (TrajPlanner::generateLSC for every ordered pair), device buffers:
 *   d_normal [count][N-1][M][3] float, d_d [count][N-1][M][n+1] double. */
int lsc_sweep_device(lsc_ctx *ctx, const float *d_state, const float *d_traj_prev, int planner_seq,
                     float *d_normal, double *d_d, void *hip_stream);
/* The same sweep with the margins rounded to float32 (d_d32 [count][N-1][M][n+1] float): 180 B per ordered pair instead of
 * 300 -- the dump format for swarms whose table is large; the QP itself always reads the doubles. */
int lsc_sweep_device_f32(lsc_ctx *ctx, const float *d_state, const float *d_traj_prev, int planner_seq,
                         float *d_normal, float *d_d32, void *hip_stream);

/* GJK distance origin <-> conv(points) for `count` independent 6-point hulls (device kernel; test hook
 * for src/openGJK/openGJK.cpp:674-780).  pts [count][6][3] double (host), v [count][3], dist [count]. */
int lsc_gjk_batch(lsc_ctx *ctx, const double *pts, int count, double *v, double *dist);

/* Introspection used by bench.py: name / average device time (ms, HIP events) of the kernels timed since
 * the last reset.  which: 0 = plan kernel (all passes: LSC generation + QP), 1 = dense sweep kernel, 2 = the trajectory
 * all-gather of the sharded ticks, 3 = goal kernel (octomap worlds, mode/goal prior_based), 4 = corridor (SFC) kernel --
 * the per-phase columns of PlanningTimeStatistics (include/sp_const.hpp:89-128) that exist as separate launches; 5 = host
 * wall clock of lsc_replan_tick itself, entry to return (PCIe-inclusive: what the reference-side caller waits for); 6 = the record
 * launch of lsc_fly_device (one per tick while a flight log is open).
 * What a sample of which = 0 is: the kernels of the plan group stamp it themselves.  Thread 0 of every workgroup of the group's
 * first kernel reads the device's constant-rate clock at entry and folds it into the begin word of the sample's slot (atomic
 * minimum); thread 0 of every workgroup of its last kernel reads it on the way out and folds it into the end word (atomic
 * maximum).  The sample is end - begin at the clock's rate (hipDeviceAttributeWallClockRate): first workgroup's entry of the first
 * kernel to the last exit of a workgroup's first wave in the last kernel (no barrier is added for the stamp: a wave that
 * outlives the first wave of its workgroup is not in the sample).  The launches are plain launches -- a timed tick puts the packets of an
 * untimed tick into the queue -- and the two query functions synchronise ONE stream, that of the last stamped launch, read the
 * slots with one copy and convert: a context that is ticked on several streams between two queries must synchronise the others
 * itself before it asks.  The dispatch's own launch and the drain of its stores are NOT in such a sample (headline: 0.3 us below
 * an event pair's sample of the same launch).  A context has LSC_TIMING_SLOTS slots (default 4096, allocated and armed by
 * lsc_set_timing(ctx, 1), which synchronises that stream first).  Events time the plan group instead, in the same list and in
 * launch order, for: samples beyond the slots, a group with nothing to launch, a group of the throughput build (a shard of more
 * agents than CUs), a group whose plan launch has more than 256 workgroups, a profiled launch, and a context whose agents were
 * set with LSC_TIMING_EVENTS=1 in the environment.  which = LSC_TIME_STAMPED_COUNT of lsc_kernel_time_ms is no time:
 * *launches receives how many samples of which = 0 since lsc_set_timing(ctx, 1) came from stamps (*avg_ms 0).
 * What a sample of the other groups (and of an event-timed plan group) is: the events of a timed group ride on its launches
 * (hipExtLaunchKernel: start on the first kernel, stop on the last), so a sample is the dispatches' own time, begin of the first
 * kernel to end of the last -- the number rocprofv3 reports for the kernel -- and timing puts no packet of its own into the queue,
 * but a dispatch whose completion carries timestamps costs the tick about 4 us.  The way to the kernel (1-1.5 us per launch, which a
 * pair of recorded markers around the launch used to include) is not in it.  which = 2 is the exception: RCCL launches its own
 * kernels, so the exchange is clocked by a pair of recorded events around it. */
#define LSC_TIME_STAMPED_COUNT 100
int lsc_kernel_time_ms(lsc_ctx *ctx, int which, double *avg_ms, long *launches);
int lsc_set_timing(lsc_ctx *ctx, int enabled);
/* Per-launch device times (ms) of the launches timed since lsc_set_timing(ctx, 1): up to `capacity` values in launch
 * order; *launches receives how many were timed (bench.py's p99 per-tick solve time). */
int lsc_kernel_times_ms(lsc_ctx *ctx, int which, double *out_ms, long capacity, long *launches);

/* current_goal_position of every agent as used by the last tick, float [N][3] (goal_mode 1: planned on the device). */
int lsc_last_goals(lsc_ctx *ctx, float *goals);
/* Where the goal planner's grid search of the last tick kept its OPEN rows, for each of the context's agents (int [count], the
 * agents first .. first + count - 1): 0 LDS, 1 LDS and restarted in HBM after a row outgrew its LDS capacity, 2 HBM from the
 * start (grids too large for LDS, goal_search = 3).  goal_mode 1 + use_octomap with a distance field; LSC_ESTATE otherwise.
 * The HBM workspace's size is reported by lsc_last_note after lsc_set_distmap.  Synchronises. */
int lsc_goal_storage(lsc_ctx *ctx, int *where);

/* Goal-planner introspection (goal_mode 1 + use_octomap; parity tests): lsc_set_goal_trace(ctx, path_cap > 0) makes
 * the following ticks keep each agent's grid path; lsc_get_goal_trace returns, for the shard's agents, the path as
 * grid cells (i, j, k) int [count][path_cap][3], its length [count] (GridBasedPlanner::plan_result.grid_path,
 * src/grid_based_planner.cpp:66), flags [count] (bit 0 retreat rule fired, bit 1 the search without priorities was
 * used) and the number of nodes the search popped [count].  grid_dims / grid_min (optional) describe the grid of
 * GridBasedPlanner::updateGridInfo (src/grid_based_planner.cpp:72-93). */
int lsc_set_goal_trace(lsc_ctx *ctx, int path_cap);
int lsc_get_goal_trace(lsc_ctx *ctx, int *path_cells, int *path_len, int *flags, int *expansions, int grid_dims[3],
                       double grid_min[3]);

/* Active (non-redundant) LSC rows each agent's QP carried in the last tick, [N] (diagnostics). */
int lsc_last_row_counts(lsc_ctx *ctx, int *rows);
/* Neighbour lists of the last tick (diagnostics).  Swarms of 512 to 65 536 agents do not walk all N - 1 other agents per agent (the loops of
 * TrajPlanner::generateLSC, src/traj_planner.cpp:1335-1407, and goalPlanningWithPriority, :540-608): a uniform grid built in front of
 * the tick hands every agent of the shard
 *   units [N]               how many (obstacle, segment) units its LSC build looks at instead of all 5 (N - 1); -1: no list (capacity
 *                           overflow), the agent culled by itself;
 *   priority_candidates [N] (optional, may be NULL) how many agents lie within priority_dist_threshold of it -- all the priority rule can
 *                           act on; -1: no list, the agent scanned everybody; 0 when goals are not planned in the plan kernel.
 * Agents outside the shard keep what an earlier tick left.  Returns LSC_ESTATE when the context builds no lists (fewer than 512 or more
 * than 65 536 agents, prune != 1, LSC_NO_NEIGHBOUR_LISTS set when lsc_set_agents ran).  Results never depend on the lists. */
int lsc_neighbour_counts(lsc_ctx *ctx, int *units, int *priority_candidates);
/* Everything the two grid kernels (lsc_neigh.hip) wrote in the last tick, copied to the host (diagnostics; tests/test_gpu_neighbour_lists.py
 * holds it to a float64 reference).  Every output may be NULL and is then skipped:
 *   caps [2]                 capacity of an agent's unit list and of its priority list: the row lengths of units / priority below
 *                            (a first call with every other output NULL reads them);
 *   obs_bound [N][4]         centre and radius of the sphere around all predicted control points and the position of each agent;
 *   seg_bound [N][M][4]      the same around the six predicted control points of each segment;
 *   reach [N][M]             the bound B_m on how far a control point of segment m can end up from c_{0,2};
 *   query_radius             the swarm-wide obstacle-side radius G of the tick that sizes every query box (0 if no agent added to it);
 *   unit_count [N]           entries of each agent's unit list, -1: no list; as lsc_neighbour_counts reports them;
 *   units [N][caps[0]]       the units (obstacle * M + segment, obstacle = the other agent's index, minus one behind the own) as full 32-bit
 *                            values -- the lists of wide swarms ((N - 1) M > 65 535) hold 16 bits per entry and are decoded here exactly as
 *                            the plan kernel decodes them --, -1 behind the count;
 *   priority_count [N]       candidates of the priority rule, -1: no list; 0 when goals are not planned in the plan kernel;
 *   priority [N][caps[1]]    the candidates (agent indices, any order, possibly repeated), -1 behind the count;
 *   disturbed [N]            the swarm's disturbance bit as the agent is handed it (1: some agent is or was off its plan), -1 where
 *                            priority_count is -1.
 * spheres, reach and query_radius exist for all N agents, the lists for the agents of the shard (others keep what an earlier tick left).
 * Returns LSC_ESTATE, with the cause in lsc_last_error, when the context builds no lists (see lsc_neighbour_counts) or when the last tick
 * did not launch the grid kernels: lists that do not pay for the shard (without LSC_NEIGH_ALWAYS), ticks that dump constraints, traced
 * ticks, BVC / slack modes, ticks with dynamic obstacles, batched ticks; and before the first tick. */
int lsc_neighbour_dump(lsc_ctx *ctx, int caps[2], float *obs_bound, float *seg_bound, float *reach, float *query_radius, int *unit_count,
                       int *units, int *priority_count, int *priority, int *disturbed);
/* LSC rows one agent may carry in LDS before the second pass (rows in HBM) takes it over: *lds_rows for the 512-lane latency
 * build (shards of at most one agent per CU), *throughput_rows for the 256-lane build that larger shards use (two workgroups
 * per CU, half the LDS each; 0 = not available, e.g. when max_rows_per_cp was set explicitly). */
int lsc_row_capacity(const lsc_ctx *ctx, int *lds_rows, int *throughput_rows);
/* Rows of each agent's fullest control-point bucket in the last tick, [N]: what the first pass's LDS capacity
 * (max_rows_per_cp) has to hold for the agent not to take the second pass (diagnostics). */
int lsc_last_bucket_max(lsc_ctx *ctx, int *rows);

/* Sum over agents of interior-point iterations since the last reset (bench flop accounting). Synchronises. */
int lsc_iterations_total(lsc_ctx *ctx, long long *total, int reset);
/* Sum over agents of iterations x LSC rows carried (the rows that survived the redundancy pruning), since the last reset of
 * lsc_iterations_total: what the kernels executed, next to the 27 (N - 1) rows per iteration of the reference's model
 * (bench.py: roofline.frac_executed). */
int lsc_row_iterations_total(lsc_ctx *ctx, long long *total);

/* Counters of the active-set solve (lsc_config.solver 1) since the last reset of lsc_iterations_total: out[0] agent-replans it finished,
 * [1] agent-replans it handed to the interior point (working set beyond its capacity, dependent rows, no admissible step: the
 * interior point then decides, infeasible verdicts included), [2] changes of the working set, [3] interior-point iterations of the
 * handed-over agents.  Synchronises. */
int lsc_solver_stats(lsc_ctx *ctx, long long out[4]);
/* Largest working set of every agent's last active-set solve (diagnostics): peaks[N].  The first call after lsc_set_agents allocates the
 * per-agent array and reads zeros; from then on every plan kernel stores into it (before, it stores nothing).  0: the unconstrained
 * optimum violated no row, or the agent's last tick ran no active-set solve; 1 .. 12: rows the working set held at its largest;
 * 13: the solve needed a thirteenth row and handed the agent to the interior point.  Synchronises. */
int lsc_working_set_peaks(lsc_ctx *ctx, int *peaks);

/* Diagnostics.  lsc_phase_profile: enable=1 selects the instrumented plan kernel and clears its counters, 0 goes
 * back to the production kernel, -1 only reads; out (may be NULL) gets [N][16] counts (100 MHz wall clock)
 * per phase: setup, LSC build, IP init, residual pass, row reduction, Hessian assembly, Cholesky, triangular
 * solves, affine pass, corrector pass, step+update, output; then two parts of the row reduction (the LSC-bucket sums as wave 0
 * sees them, the axis-row gather as the last lane sees it) and two spare slots.  lsc_solver_residuals: [N][4] last duality gap,
 * primal residual, stationarity residual, objective. */
int lsc_phase_profile(lsc_ctx *ctx, int enable, long long *out);
/* The same for the goal planner's register-resident grid search: out gets [N][16] counters, shader cycles unless noted:
 * prologue (priority / retreat rule), grid set-up, search, path + line-of-sight goal; of the search: findMin, deleteMin,
 * neighbour screening, insertions; of those: cycles and count of the pops and of the insertions that took the general LDS
 * routines (rows beyond 64 entries, rehashes); the rest is reserved.  LDS searches only: enable = 1 is refused (LSC_ESTATE) on a
 * context whose grid is searched in HBM from the start, and an agent whose LDS search restarted in HBM records nothing. */
int lsc_goal_profile(lsc_ctx *ctx, int enable, long long *out);
/* Test hook, host only (no device needed): the 32-bit key table of the grid search for squared cell distances 0 .. words-1 --
 * out[d] = floor(sqrt d) << *rank_bits | rank of frac(sqrt d); a search key is (steps << rank_bits) + out[d2].  LSC_ESTATE when the
 * table's exactness conditions do not hold for that range (the search then keeps 64-bit keys). */
int lsc_goal_key_table(int words, unsigned int *out, int *rank_bits);
/* lsc_general_profile: sections of the alternate-mode kernel -- BVC / slack modes / disturbed agents -- collected while
 * lsc_phase_profile is enabled and cleared with it; out[N][16] shader cycles: set-up, start, residual pass, row reduction,
 * assembly, factorization, solves, affine pass, corrector right-hand side, its reduction and assembly, step; [12] the
 * iterations and [13] the solves of the agent. */
int lsc_general_profile(lsc_ctx *ctx, long long *out);
/* Read-only diagnostics of the alternate-mode solver (tests).  *lds_obstacles: the largest number of KEPT obstacles of one agent whose
 * row arrays all fit in LDS behind the solver's state, for this context's swarm size: an agent with at most that many is solved by the
 * build that addresses its rows as LDS, an agent with more by the generic-pointer build, whose last arrays lie in the HBM workspace
 * (lsc_last_row_counts gives 27 + M rows per kept obstacle).  *last_launch: how the context's last tick reached the solver -- 0 not at
 * all, 1 inside the plan kernel (the folded hand-over), 2 a launch of lsc_general_kernel behind it, 3 one of lsc_general_batch_kernel
 * (a batched tick).  Either pointer may be NULL. */
int lsc_general_info(const lsc_ctx *ctx, int *lds_obstacles, int *last_launch);
int lsc_solver_residuals(lsc_ctx *ctx, double *out);
/* QP failure forensics (TrajOptimizer::solve exports the model it could not solve: log/QPmodel.lp, src/traj_optimizer.cpp:99-153).
 * Writes the QP of `agent` as the LAST host-buffer tick (lsc_replan_tick / lsc_replan_tick_all) posed it, in CPLEX LP format with
 * the reference's variable names (x_m_i, y_m_i, z_m_i) and populatebyrow's row order (c1, c2, ...), so that it can be diffed against a
 * reference dump or fed to any LP/QP solver.  LSC mode, rows without slack variables. */
int lsc_dump_qp(lsc_ctx *ctx, int agent, const char *path);
/* Reads the [64][8] per-iteration trace recorded for the agent selected by the PREVIOUS call (out may be NULL),
 * then selects `agent` (-1: off): gap, |rp|, objective, affine step, sigma, step, |dx_aff|, mu.  Agents solved by the
 * alternate-mode kernel record the same eight values per iteration (the matrices behind the [64][8] block are the fast path's only). */
int lsc_solver_trace(lsc_ctx *ctx, int agent, double *out);

#ifdef __cplusplus
}
#endif
#endif
