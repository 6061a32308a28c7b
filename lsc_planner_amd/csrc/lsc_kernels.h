// lsc_kernels.h -- argument blocks shared by the kernels (lsc_kernels.hip) and the C ABI (lsc_abi.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include <stdint.h>

#include "lsc_model.hpp"

#define LSC_STATUS_OK_K 0
#define LSC_STATUS_INFEASIBLE_K 1
#define LSC_STATUS_CAPACITY_K 3
#define LSC_STATUS_SFC_K 4
#define LSC_STATUS_GOAL_K 5
#define LSC_STATUS_GENERAL_K 6   /* internal: the agent's QP has an alternate-mode shape -> lsc_general_kernel solves it */

namespace lsc {

struct PlanArgs;
struct NeighArgs;
struct ObsBlock;
struct NeighView;
// an argument block read where it lies, in the kernarg segment: constant address space => scalar loads, no private copy
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) PlanArgs KArgs;
#else
typedef const PlanArgs KArgs;
#endif

struct PlanArgs {
    const Model *model;
    const uint32_t *terms;     // packed Hessian assembly terms
    const uint32_t *entries;   // [n_entries+1][2] : (gi<<16|gj, first term)
    int N, first, count, planner_seq;
    int dim2;                  // world/dimension == 2: the launch takes the planar instantiation of the plan kernels (a compile-time switch)
    int cap;                   // LSC rows the LDS pass holds (total over the 27 control points; compact layout)
    int solver;                // 0 interior point; 1 dual active set first, interior point as fallback (lsc_config.solver)
    long long *solver_stats;   // optional [N][4] running counters of the active-set solve, per agent (lsc_solver_stats sums them)
    int *order;                // throughput build: launch order of the shard's agents (longest first), or null
    float *obs_bound;          // throughput build: [N][4] bounding sphere of every agent's predicted control points, or null
    int cap_tp;                // > 0: use the 256-lane throughput build with this row capacity and smem_tp bytes of LDS
    size_t smem_tp;
    NeighArgs *neigh;          // HOST pointer (never read on the device), or null: the context's neighbour-list buffers; run_plan (lsc_abi.cpp) launches
                               // the two kernels of lsc_neigh.hip in front of the tick of a large swarm and sets nv
    const NeighView *nv;       // device: the lists those kernels left for this tick, or null (every agent walks all the others, as small swarms do)
    const float *state;        // [N][9]
    const float *goal;         // [N][3] current goal (mode/goal static) or desired goal (prior_based)
    int goal_mode;             // 0 static, 1 prior_based: goalPlanningWithPriority runs in phase A of the plan kernel
    double goal_threshold, priority_dist_threshold, goal_radius;
    float *goal_out;           // [N][3] current_goal_position actually used (diagnostics / getCurrentGoalPosition)
    float *state_next;         // optional [N][9]: ideal state of the agent at t = dt on its NEW plan (fused propagation)
    float finv;                // (float)pow(dt, -1)
    const float *traj_prev;    // [N][90]
    const double *radius, *radius_obs, *downwash, *downwash_obs;  // [N]; *_obs = value rounded through float32
    const double *vmax, *amax; // [N][3]
    const double *vnom;        // [N]
    float *traj_next;          // [N][90]
    double *cost;              // [N]
    int *status, *iters, *nrows;
    int *bucket_max;           // optional [N]: rows of the fullest control-point bucket (diagnostics)
    long long *iters_acc;      // [N] running sum of interior-point iterations (bench accounting), may be null; entries [N, 2N) = running
                               // sum of iterations x LSC rows the agent carried (the row passes the kernel really executed)
    float *stale;              // [N][90] optimiser's last good trajectory (persistent)
    const float *sfc;          // [N][M][6] or null
    const int *sfc_err;        // [N] or null: seed box blocked -> status 4
    const int *goal_err;       // [N] or null: goal planner capacity overflow -> status 5
    float *out_normal;         // optional dense dump [count][N-1][M][3]
    double *out_d;             // optional dense dump [count][N-1][M][6]
    double *dbg;               // optional [N][4]: last (gap, |rp|, |rd|, objective) seen by the solver
    long long *prof;           // optional [N][PROF_PHASES] phase counters (selects the instrumented kernel)
    double *trace;             // optional [64][8] per-iteration trace of agent trace_agent (diagnostics)
    int trace_agent;
    unsigned char *spill_ws;   // second pass only: HBM row workspaces, one of spill_stride bytes per workgroup
    size_t spill_stride;
    // alternate planner modes (lsc_general.hip)
    const GModel *gmodel;
    int planner_mode;          // 0 LSC, 1 BVC
    int slack_mode;            // 0 none, 1 dynamical_limit, 2 collision_constraint
    int ncs;                   // opt/N_constraint_segments (-1 -> M)
    int general_all;           // every agent takes the general kernel (BVC or a slack mode is configured)
    double slack_w;            // opt/slack_collision_weight
    double reset_thr;          // multisim/reset_threshold; <= 0: no disturbance checks
    unsigned char *ever;       // [N] persistent: agent was seen off its plan at some tick (its rows keep slack variables)
    unsigned char *gen_ws;     // HBM workspaces of lsc_general_kernel, gen_stride bytes per workgroup (folded: per agent of the launch)
    size_t gen_stride;
    int fold;                  // lsc_plan_alt_kernel solves the agents it hands over itself (general_fold, lsc_general.hpp): no
                               // lsc_general_kernel launch follows.  Set by run_plan for one-round launches with room for count workspaces
    int generic_lsc_build;     // phase B never takes the one-wave-per-segment LSC build of small swarms (LSC_GENERIC_LSC_BUILD: tests, A/B runs)
    int step_all_slots;        // the active-set solve runs every change over all slots of the working set (LSC_STEP_ALL_SLOTS: tests, A/B runs);
                               // 0: over the slots of a size class, 4 / 8 / 12 by the largest working set the solve has held
    int plain_handover;        // the step of the active-set solve loads the chosen row's word, right-hand side and normal itself (the
                               // default); 0: the search hands them over as the row's record (LSC_SOLVE_ROW_RECORD: tests, A/B runs)
    int *ws_peak;              // optional [N]: largest working set of the agent's last active-set solve (lsc_working_set_peaks), or null
    const ObsBlock *obs;       // device: the mission's dynamic obstacles (lsc_set_obstacles), or null: none.  Non-null selects the OBS instantiations
    long long *t_begin, *t_end; // clock stamps of a timed launch group (LaunchEvents below: put_stamps fills them, nobody else), or null: where the
                               // group's first launch leaves its begin and its last launch its end (stamp_exit / stamp_end)
};
// The dynamic obstacles of a context (ObstacleType::DYNAMICOBSTACLE: non-cooperating moving spheres), one device-resident block: an agent's
// obstacle list is the other N - 1 agents in index order, then these K.  radius / downwash: rounded through float32, as dynamic_msgs::Obstacle
// holds them (PlanArgs::radius_obs does the same for agents).
constexpr int OBSTACLES_MAX = 64;
struct ObsBlock {
    int K, pad;
    const float *pos_vel;      // [K][6] position | velocity of this tick (the context's own buffer, or the caller's: lsc_obstacle_states_device)
    double radius[OBSTACLES_MAX], downwash[OBSTACLES_MAX];
    const double *size;        // [K][M][6] predicted sizes (rule_obstacle_size; lsc_set_obstacles_ex), or null: the context runs no disturbance
                               // checks.  Read only by general_agent<., true>, for the margins of a sphere in an agent's slack set
};
constexpr int PROF_PHASES = 16;
constexpr int LDS_MAX_BYTES = 160 * 1024;        // LDS of a CU: the largest dynamic request a kernel can opt into (allow_full_lds)

// the launch takes a build with the alternate-mode hooks: BVC or a slack mode is configured, or the disturbance checks are on
inline bool plan_alt_hooks(const PlanArgs &a) { return a.general_all || (a.reset_thr > 0.0 && a.ever); }

// One row of a kernel family's variant table: what selects the instantiation (a packed key, see plan_key / goal_key) and its address.
// The table is the ONE place an instantiation is written down: init_device_*() opts every row into the full LDS, the launchers look
// their kernel up in it, and a key without a row is a launch that is refused (hipErrorInvalidValue).
struct KernelVariant {
    int key;
    const void *fn;
};
template <class... A>
inline const void *kernel_address(void (*f)(A...)) { return reinterpret_cast<const void *>(f); }
template <size_t n>
inline const void *find_variant(const KernelVariant (&table)[n], int key)
{
    for (const KernelVariant &v : table)
        if (v.key == key) return v.fn;
    return nullptr;
}
template <size_t n>
inline hipError_t allow_full_lds(const KernelVariant (&table)[n])
{
    for (const KernelVariant &v : table) {
        const hipError_t e = hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX_BYTES);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// The timing of a launch group (lsc_set_timing, lsc_abi.cpp), in one of two forms.
//  * Clock stamps (t0 / t1; the plan group, which = 0): two words of device memory that the kernels write themselves.  Thread 0 of every
//    workgroup of the group's FIRST launch folds the device's constant-rate clock (wall_clock64: one counter for the whole card), as read
//    at the kernel's entry, into *t0 with an atomic minimum; thread 0 of every workgroup of its LAST launch folds it, as read on the way
//    out, into *t1 with an atomic maximum -- on every way out.  The launch itself is a plain hipLaunchKernel: a timed tick puts the
//    packets of an untimed tick into the queue and nothing else.  A sample is t1 - t0: first workgroup's entry of the first kernel to
//    the last exit of a workgroup's first wave in the last one (no barrier is added for the stamp: a wave that outlives wave 0 of its
//    workgroup is not in it).  The dispatch's own launch and the drain of its stores lie outside it.
//  * Events (start / stop; every other group, and the plan group where it has nothing to launch, takes the throughput or an
//    instrumented kernel -- they stamp nothing --, has more than 256 workgroups in its plan launch, finds no stamp slot of the context
//    left, or LSC_TIMING_EVENTS is set): hipExtLaunchKernel binds an event to the dispatch's own begin / end timestamp, so timing puts
//    no packet of its own into the queue (a recorded event is a barrier packet with a system-scope release, and the GPU pays for two
//    of them per tick); the dispatch's completion signal then carries timestamps, which costs the tick 4.3 us.
// A launcher takes the pair for ITS launches: first() goes to its first kernel and last() to its last, both to the only one.  All null:
// an untimed launch.
struct LaunchEvents {
    hipEvent_t start = nullptr, stop = nullptr;
    long long *t0 = nullptr, *t1 = nullptr;
    bool any() const { return start || stop; }
    bool stamps() const { return t0 || t1; }
    LaunchEvents first() const { return {start, nullptr, t0, nullptr}; }
    LaunchEvents last() const { return {nullptr, stop, nullptr, t1}; }
};
// a launcher with nothing to launch (an empty shard) still owes the stream its events: they are recorded instead.  (Stamps have nobody
// to write them: the host gives a group that may launch nothing events -- timing_begin, lsc_abi.cpp.)
inline hipError_t record_unlaunched(LaunchEvents ev, hipStream_t st)
{
    if (ev.start) { const hipError_t e = hipEventRecord(ev.start, st); if (e != hipSuccess) return e; }
    return ev.stop ? hipEventRecord(ev.stop, st) : hipSuccess;
}

// The device side of the stamps, called by the __global__ wrappers with their argument block where it lies in the kernarg segment (the
// pointer is a scalar load at the place of use, and nothing stays live across the kernel's body).  Atomics without a return value, as
// iters_acc and solver_stats are written: the wave does not wait for them.
template <class Args>
__device__ __forceinline__ const Args
#if defined(__HIP_DEVICE_COMPILE__)
    __attribute__((address_space(4)))
#endif
    *kernarg_block()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (const __attribute__((address_space(4))) Args *)__builtin_amdgcn_kernarg_segment_ptr();
#else
    return nullptr;                                                                  // (host pass of the single-source build)
#endif
}
// stamp_clock() is read at the kernel's entry, and BOTH words are written on the way out (stamp_exit; stamp_end in kernels that are never
// a group's first launch): on gfx9 an atomic without a return value counts in vmcnt like a load, so a begin stamp issued at entry stood
// in front of the wave's first wait for its own loads -- with every workgroup's stamp queued on one address, 17 ns each: 1 us of a
// 64-workgroup tick and 4.5 us of a 256-workgroup batch (profiles/timing_stamps_ab.log).  At the exit nothing waits.
__device__ __forceinline__ long long stamp_clock() { return (long long)wall_clock64(); }
template <class KA>
__device__ __forceinline__ void stamp_end(KA *ka)
{
    if (threadIdx.x != 0) return;
    if (long long *p = ka->t_end) (void)__hip_atomic_fetch_max(p, (long long)wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class KA>
__device__ __forceinline__ void stamp_exit(KA *ka, long long t_entry)
{
    if (threadIdx.x != 0) return;
    if (long long *p = ka->t_begin) (void)__hip_atomic_fetch_min(p, t_entry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (long long *p = ka->t_end) (void)__hip_atomic_fetch_max(p, (long long)wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Neighbour lists of a large swarm (lsc_neigh.hip): which (obstacle, segment) units can carry a row that survives the pruning of phase B,
// found through a uniform grid instead of a walk over all N - 1 obstacles per agent (the loop being replaced: `for oi < N_obs`,
// src/traj_planner.cpp:1335-1407).  Two launches in front of the tick: build (bounds of every agent + one grid insertion each), query
// (one workgroup per agent of the shard: the cells its reach overlaps -> sphere tests -> a sorted unit list in HBM).
constexpr int NEIGH_SLOTS = 12;                  // agents a grid bucket holds (one 32-byte sector: a tagged counter + 12 indices); the rest overflows
constexpr int NEIGH_MIN_AGENTS = 512;            // swarms below this keep the in-kernel cull
constexpr int NEIGH_PRIO_CAP = 64;               // candidates of the priority rule an agent's list holds
// Agent ids are 16-bit (grid buckets, the overflow list, the priority candidates): lists and the in-kernel cull serve up to 65 536 agents.
// A unit (obstacle * M + segment) needs more than 16 bits above 0x10000 / M agents; a list entry keeps its low 16 bits, and four
// per-agent starts (NeighView::blk) give the high part -- the lists are ascending -- so that the staged capacity of phase B stays 8 R.
constexpr int NEIGH_MAX_AGENTS = 65536;
constexpr int NEIGH_MAX_UNITS = (NEIGH_MAX_AGENTS - 1) * M;
static_assert(NEIGH_MAX_UNITS < 5 << 16, "four starts cover the high part of a unit");
// what phase A / B of plan_agent read of the lists (device memory, written once per lsc_set_agents: the pointers do not change)
struct NeighView {
    const unsigned short *list;                  // [N][cap] per agent: the units (obstacle * M + segment) phase B has to look at, ascending
    const int *cnt;                              // [N] entries of the agent's list; < 0: no list (capacity overflow), the agent culls by itself
    const unsigned short *plist;                 // [N][pcap] agents within priority_dist_threshold of the agent's position (goalPlanningWithPriority's candidates)
    const int *pcnt;                             // [N] -1: no information (the agent scans everybody); else entries of plist | (1 << 30 when ANY agent of the
                                                 // swarm is off its plan or was: the disturbance checks of phase A, made once by the build kernel)
    int cap, pcap;
    const unsigned long long *blk;               // [N] wide swarms ((N - 1) M > 0x10000): field k (16 bits) = the first entry of the agent's list whose unit
                                                 // is >= (k + 1) << 16, 0xffff = none; the entries hold the low 16 bits of each unit
};
struct NeighArgs {
    int N, first, count, planner_seq;
    float dtf;
    int dim2;
    double hv_scale, ha_scale, z2d;              // Model::hv_scale, ha_scale, z2d
    const float *state, *traj_prev;
    const double *radius, *radius_obs, *downwash, *downwash_obs, *vmax, *amax;
    int *order;                                  // launch order of the throughput build (longest agent first), or null
    const int *iters, *nrows;
    float *obs_bound;                            // [N][4] bounding sphere of all predicted control points (the in-kernel cull's, kept for agents without a list)
    float *seg_bound;                            // [N][M][4] bounding sphere of the predicted control points of each segment
    float *reach;                                // [N][M] per segment max_i(|c_{0,2} - p_{m,i}| + reach radius of c_{m,i}), rounded up
    unsigned long long *cells;                   // [hmask + 1][4] buckets: tag << 32 | count, then NEIGH_SLOTS agent indices (16 bit)
    unsigned long long *glob;                    // [16] tagged maxima: obstacle-side radius, overflow count, cell bounding box (6), somebody is off its plan
    unsigned short *ovf;                         // [ovf_cap] agents whose bucket was full
    int ovf_cap;
    unsigned tag, hmask;                         // tag of this tick (buckets of older ticks count as empty: nothing is ever cleared)
    double inv_cell, inv_cell_z;                 // 1 / cell size in x, y and in z (z cells are downwash times taller)
    double sc_max, zscale;                       // max(1, 1 / smallest downwash), max(1, largest downwash)
    unsigned short *list;                        // [N][list_cap] low 16 bits of each unit
    unsigned long long *blk;                     // [N] starts of the high parts (NeighView::blk), written by the wide query kernel
    int *cnt;                                    // [N]
    int list_cap;
    // phase A's walks over all agents (see NeighView)
    int goal_mode;                               // 1: goalPlanningWithPriority runs in phase A -> candidates by position
    double prio_thr;                             // priority_dist_threshold
    unsigned short *plist;                       // [N][plist_cap]
    int *pcnt;                                   // [N]
    int plist_cap;
    int checks;                                  // the plan kernel's disturbance checks are on (reset_threshold > 0, LSC mode, planner_seq >= 2)
    double reset_thr;
    unsigned char *ever;                         // [N] persistent "was seen off its plan" flags
    const NeighView *view;                       // device copy of the view over list / cnt / plist / pcnt
    long long *prof;                             // optional [count][8]: 100 MHz wall-clock stamps of the query kernel's stages (LSC_NEIGH_PROFILE)
    long long *t_begin, *t_end;                  // clock stamps of a timed launch group, as PlanArgs::t_begin / t_end (the build kernel stamps; the query
                                                 // kernel is never a group's first or last launch: the plan kernel follows it)
};
hipError_t launch_neigh(const NeighArgs &a, hipStream_t st, LaunchEvents ev = {});      // build + query: start rides on the build

// Several independent swarms -- one argument block each -- planned by ONE launch (blockIdx.y = swarm): the reference flies a list of
// missions back to back (src/multi_sync_simulator_node.cpp:43-70, src/param.cpp:106-122), and a 64-agent swarm is 64 workgroups on a
// 256-CU chip.  The blocks travel in the kernarg segment itself (no copy to the device; kernarg segments hold 4 KB).
constexpr int PLAN_BATCH_MAX = 8;
struct PlanBatch {
    PlanArgs a[PLAN_BATCH_MAX];
};
static_assert(sizeof(PlanBatch) <= 4096, "a batch of argument blocks must fit the kernarg segment");
// the n argument blocks of a batched launch -> the batch; the unused slots repeat the first block with count = 0 (their workgroups do
// not exist: blockIdx.y < n).  Returns the largest count, the launch's grid in x.
template <class Batch, class Args>
inline int fill_batch(Batch &b, const Args *a, int n)
{
    int most = 0;
    for (int i = 0; i < PLAN_BATCH_MAX; i++) {
        b.a[i] = a[i < n ? i : 0];
        if (i >= n) b.a[i].count = 0;
        else if (a[i].count > most) most = a[i].count;
    }
    return most;
}

// the stamp pointers of a timed launch -> its argument block(s); in a batch launch every swarm's workgroups stamp the same two words.
// Argument blocks of the groups that stay on events have no such fields.
inline void put_stamps(PlanArgs &a, const LaunchEvents &ev) { a.t_begin = ev.t0; a.t_end = ev.t1; }
inline void put_stamps(NeighArgs &a, const LaunchEvents &ev) { a.t_begin = ev.t0; a.t_end = ev.t1; }
inline void put_stamps(PlanBatch &b, const LaunchEvents &ev)
{
    for (PlanArgs &a : b.a) put_stamps(a, ev);
}
template <class Args>
inline void put_stamps(Args &, const LaunchEvents &) {}
// launch a kernel of one argument block through its address (hipLaunchKernelGGL ends in the same call); null: find_variant had no row
template <class Args>
inline hipError_t launch_variant(const void *fn, dim3 grid, dim3 block, size_t smem, hipStream_t st, const Args &args, LaunchEvents ev = {})
{
    if (!fn) return hipErrorInvalidValue;
    Args t = args;
    put_stamps(t, ev);                                 // (null for an untimed launch and for one timed by events, whatever the caller's block held)
    void *kargs[] = {&t};
    if (ev.any()) (void)hipExtLaunchKernel(fn, grid, block, kargs, smem, st, ev.start, ev.stop, 0);
    else (void)hipLaunchKernel(fn, grid, block, kargs, smem, st);
    return hipGetLastError();
}

struct SweepArgs {
    int N, first, count, planner_seq;
    float dtf;
    const float *state, *traj_prev;
    const double *radius, *radius_obs, *downwash, *downwash_obs;
    float *out_normal = nullptr;
    double *out_d = nullptr;
    float *out_d32 = nullptr;  // margins as float32 instead (out_d unused)
};

// Safe Flight Corridor update (TrajPlanner::generateFeasibleSFC), one lane per agent
struct SfcArgs {
    int N, first, count;
    const float *state, *goal, *traj_prev;
    const double *radius;
    const int *img_of_agent;    // [N] index of the blocked-cell integral image matching the agent's margin
    const int *integral;        // [n_img][(nx+1)(ny+1)(nz+1)] inclusive 3-D prefix sums of "EDT < r + res/2 - 1e-5"
    int nx, ny, nz;
    int key_min[3];
    double rf;                  // 1 / tree resolution (OcTreeBaseImpl::resolution_factor)
    double wres;                // world/resolution
    float world_min[3], world_max[3];
    float *sfc;                 // [N][M][6] persistent boxes (box_min, box_max as float)
    int *init_flag;             // [N] flag_initialize_sfc
    int *err;                   // [N] 1 when the seed box already touches an obstacle
    int table_len;              // entries per face table in LDS: steps a face can move inside the world + slack
    int planner_seq;
    double reset_thr;           // initialTrajPlanningCheck: an agent found off its plan re-initialises its corridor
};
hipError_t launch_sfc(const SfcArgs &a, hipStream_t st, LaunchEvents ev = {});

// Goal planning with a distance field (lsc_goal.hip): priority rule, grid A*, line-of-sight goal.  One wave per agent.
struct GoalArgs {
    int N, first, count, planner_seq;
    float dtf;
    const float *state, *goal, *traj_prev;     // goal = desired goals [N][3]
    const double *radius, *downwash, *radius_obs, *downwash_obs;
    double goal_threshold, priority_dist_threshold, goal_radius;
    // planning grid (GridBasedPlanner::updateGridInfo): dims, origin, resolution; cells addressed by key = H*W*z + W*i + j
    int H, W, A;
    int dim2;                                   // world/dimension == 2: start, goal and stamped agents sit in layer 0
    double gmin[3], gres;
    const unsigned char *occ_static;            // [n_img][H*W*A] by key: EDT(cell centre) < radius + grid_margin
    const int *img_of_agent;                    // [N]
    // distance field (DynamicEDTOctomap::getDistance)
    const float *edt;
    int nx, ny, nz, key_min[3];
    double rf, wres;
    // libstdc++ unordered_map bucket-count sequence (13, 29, 59, ...), read from the real container on the host
    int n_nb;
    int nb_seq[16];
    uint32_t nb_magic[16];                      // floor(2^32 / nb_seq[k])
    int row_cap;                                // LDS capacity of one OPEN row (entries)
    int variant, jbits;                         // search variant (see launch_goal: slots | 8 = Key32) and the bits of j in a register-search entry
    const uint32_t *fcode;                      // Key32 table [fcode_n]: floor(sqrt d2) << fcode_rb | rank of frac(sqrt d2), or null
    int fcode_n, fcode_rb;
    float *goal_out;                            // [N][3] current_goal_position
    int *err;                                   // [N] 0 ok, 1 capacity (row / path / g overflow), 2 ray stack overflow
    int *flags;                                 // optional [N]: bit 0 retreat rule, bit 1 search without priorities used
    int *expansions;                            // optional [N]: nodes popped
    int *path_out;                              // optional [count][path_cap] keys of the grid path (start -> goal)
    int path_cap;
    int *path_len;                              // optional [count]
    float *ray_stack;                           // [count][64][24][6] bisection stacks of castRay
    double reset_thr;                           // disturbance checks (multisim/reset_threshold; <= 0 off)
    const unsigned char *ever;                  // [N] persistent "was seen off its plan" flags
    long long *prof;                            // optional [N][8] section cycle counters (selects the instrumented kernel)
    int smem_bytes;                             // dynamic LDS of the launch (set by launch_goal; the poison build fills it)
    // HBM search state (large worlds): per agent, OPEN rows [H][W A] and the temp row [W A] as 32-bit entries, then (hbm = 2) the
    // cell bytes [C].  hbm = 0 with ws set: an LDS search whose row overflows restarts with its rows there (row_cap is then the LDS
    // capacity); hbm = 1 / 2: the HBM search from the start (row_cap = W A), cell bytes in LDS / in the workspace
    int hbm;
    unsigned char *ws;                          // [count][ws_stride] or null
    size_t ws_stride;
    int *storage;                               // optional [N]: 0 LDS search, 1 LDS search restarted in HBM, 2 HBM search
};
size_t goal_smem_bytes(int H, int W, int A, int cap, int key_words = 0);
size_t goal_hbm_smem_bytes(int H, int W, int A, bool cells_in_lds);     // LDS request of the HBM search (row bookkeeping [+ cell bytes])
size_t goal_hbm_ws_bytes(int H, int W, int A, bool cells_in_ws);        // its per-agent workspace (also the restart's, cells_in_ws = false)
int goal_fast_slots(int H, int W, int A, int *jbits);
hipError_t launch_goal(const GoalArgs &a, hipStream_t st, LaunchEvents ev = {});

// The goal search and the corridor update of several independent swarms, one launch each (blockIdx.y = swarm), like PlanBatch: a swarm
// on a map with a distance field runs both in front of its plan kernel, so a batched tick is goal batch -> SFC batch -> plan batch.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) GoalArgs KGoalArgs;
typedef const __attribute__((address_space(4))) SfcArgs KSfcArgs;
#else
typedef const GoalArgs KGoalArgs;
typedef const SfcArgs KSfcArgs;
#endif
struct GoalBatch {
    GoalArgs a[PLAN_BATCH_MAX];
};
struct SfcBatch {
    SfcArgs a[PLAN_BATCH_MAX];
};
static_assert(sizeof(GoalBatch) <= 4096 && sizeof(SfcBatch) <= 4096, "a batch of argument blocks must fit the kernarg segment");
// swarms of one search instantiation (launch_goal's variant: same slots, Key32 or not; no profiling) in one launch; LDS = the largest request
hipError_t launch_goal_batch(const GoalArgs *a, int n, hipStream_t st, LaunchEvents ev = {});
hipError_t launch_sfc_batch(const SfcArgs *a, int n, hipStream_t st, LaunchEvents ev = {});
int goal_batch_class(const GoalArgs &a);      // the key of the batch instantiation `a` takes (lsc_goal.hip: goal_key): two blocks may share a launch iff theirs are equal

size_t general_ws_bytes(int N);
size_t general_lds_bytes(int N);
int general_lds_obstacles(int N);
hipError_t init_device_general_kernel();
hipError_t launch_general(const PlanArgs &a, int slots, hipStream_t st, LaunchEvents ev = {}, int n_dyn = 0);   // n_dyn: the K of a.obs
size_t plan_smem_bytes(int n_terms, int n_entries, int rows, bool tables_in_lds = true);
size_t plan_spill_bytes(int n_obs);      // n_obs: obstacles per agent (N - 1 agents + the dynamic obstacles)
hipError_t init_device_kernels();
hipError_t init_device_goal_kernel();
hipError_t launch_plan(const PlanArgs &a, size_t smem, hipStream_t st, LaunchEvents ev = {});      // (start rides on lsc_prep_kernel where that runs in front)
bool plan_kernel_is_throughput(const PlanArgs &a);   // launch_plan takes the throughput build for `a`: its kernels carry no clock stamps
bool plan_kernel_folds(const PlanArgs &a);    // launch_plan takes lsc_plan_alt_kernel for `a`, the one kernel that can fold (a.fold itself is not read)
hipError_t launch_plan_batch(const PlanArgs *a, int n, size_t smem, hipStream_t st, LaunchEvents ev = {});
hipError_t launch_general_batch(const PlanArgs *a, int n, int slots, hipStream_t st, LaunchEvents ev = {});
hipError_t launch_plan_spill(const PlanArgs &a, int slots, size_t smem, hipStream_t st, LaunchEvents ev = {});
hipError_t launch_sweep(const SweepArgs &a, hipStream_t st, LaunchEvents ev = {});
hipError_t launch_propagate(const float *traj, float *state, int N, double dt, hipStream_t st);
hipError_t launch_safety(const float *traj, const double *weights, const int *seg, int n_times, int N, int first, int count,
                         const double *radius, const double *downwash, float *pos, double *out_ratio, int *out_partner, hipStream_t st);
hipError_t launch_gjk(const double *pts, int count, double *v, double *dist, hipStream_t st);

// The flight record of one tick (lsc_flight.hip): the simulator's per-tick accounting appended to the open log as one row, one launch
// behind the tick's last launch.  `row` is the tick's row (layout: lsc_flight.hpp, flight_layout), whose summary lsc_flight_begin /
// lsc_flight_reset initialised; w5 / w4 / w3 / seg are the host-built Bernstein weights and segments of the n_times record times.
struct FlightArgs {
    int N, n_times, what, planner_seq;
    int agents_per_block;      // agents one workgroup accounts for (flight_agents_per_block)
    float dt_inv;              // (float)pow(dt, -1)
    double goal_threshold;
    const float *state;        // [N][9] the tick's input state
    const float *goal;         // [N][3] the tick's goal input
    const float *traj_prev, *traj_next;   // [N][3][M*6]
    const double *cost;        // [N]
    const int *status;         // [N]
    const double *radius, *downwash;      // [N] (the doubles of lsc_set_agents)
    const double *w5, *w4, *w3;           // [n_times][6], [n_times][5], [n_times][4]
    const int *seg;            // [n_times]
    unsigned char *row;
};
int flight_agents_per_block(int N, int what);
hipError_t launch_flight(const FlightArgs &a, hipStream_t st, LaunchEvents ev = {});
// summaries of `rows` log rows of row_bytes each: zeros, min_ratio = 1e300
hipError_t launch_flight_init(unsigned char *rows, size_t row_bytes, int n_rows, hipStream_t st);

// The goal stage of a tick (lsc_mission.hip): the first lines of TrajPlanner::goalPlanning (src/traj_planner.cpp:477-509) for every agent,
// in front of everything else the tick launches.  With a mission state (desired != null) it applies the patrol swap or the GOBACK
// assignment to the context's tables from the tick's INPUT state; with the right-hand rule (rule_goal != null) it writes the goal the
// rest of the tick reads.  Without a mission state the desired goals are the caller's (goal_in).
constexpr int MISSION_GOTO = 0, MISSION_PATROL = 1, MISSION_GOBACK = 2;      // PlannerState (LSC_MISSION_* of the C ABI)
struct MissionArgs {
    int N, planner_state, planner_seq;
    int seq_threshold;                         // deadlock_seq_threshold of the right-hand rule
    double goal_threshold, velocity_threshold;
    const float *state;                        // [N][9] the tick's input state
    const float *goal_in;                      // [N][3] the caller's goals: read only when desired == null
    float *desired, *start;                    // [N][3] each: the leg every agent flies (null: no mission state)
    const float *mission_start, *mission_goal; // [N][3] each: the mission as it was opened
    int *legs;                                 // [N] swaps made since the mission state was opened
    float *rule_goal;                          // [N][3] right-hand rule: the tick's current goals (null: the rule is not set)
};
hipError_t launch_mission(const MissionArgs &a, hipStream_t st);

// The obstacle stage of a tick (lsc_obstacles.hip): a context with motion models (lsc_obstacle_motion) moves its dynamic obstacles itself,
// in front of everything else the tick launches.  t: the tick's time on the obstacles' clock, formed by the host; table: the host-built
// constants of the K models (lsc_obstacle_motion.hpp); pos_vel: the [K][6] buffer ObsBlock::pos_vel points to.
struct ObstacleEntry;
struct ObstacleStageArgs {
    int K, pad;
    double t;
    const ObstacleEntry *table;                // [K]
    float *pos_vel;                            // [K][6]
    double *pos_f64;                           // [K][3] the positions before the rounding to float32 (lsc_obstacle_positions_read)
};
hipError_t launch_obstacle_stage(const ObstacleStageArgs &a, hipStream_t st);

// The stage of a context with at least one chasing or gaussian model (lsc_obstacle_motion_ex), launched instead of the one above.  The
// parameter tables are indexed by the obstacle; `first`: no stage has run since the installation (the previous obstacles are zeros).
struct ObstacleChaser;
struct ObstacleWalker;
struct ObstacleStepArgs {
    int K, first;
    double t;
    const ObstacleEntry *table;                // [K] (kinds 3 and 4: the kind alone)
    const ObstacleChaser *chasers;             // [K]
    const ObstacleWalker *walkers;             // [K]
    const double *acc;                         // the walkers' acceleration histories, [.][3] (may be null without walkers)
    const ObsBlock *obs;                       // radius[K] rounded through float32
    const float *state;                        // [N][9] THIS tick's input state: a chaser's goal point is its target's position
    double *chaser_state;                      // [K][7] pos | vel | t_last
    float *pos_vel;                            // [K][6]
    double *pos_f64;                           // [K][3] in: the previous tick's positions; out: this tick's
};
hipError_t launch_obstacle_step(const ObstacleStepArgs &a, hipStream_t st);

// The obstacle track of one tick (lsc_obstacles.hip), one launch behind the tick's flight record: the agents' sample positions at the log's
// record times (w5 / seg: the log header's) against the obstacles where the tick's stage put them.  `row` is the tick's track row
// (obstacle_track_layout), whose summary lsc_flight_begin / lsc_flight_reset initialised.
struct ObstacleRecordArgs {
    int N, n_times, K, pad;
    const float *traj_next;                    // [N][3][M*6]
    const double *radius;                      // [N] (the doubles of lsc_set_agents)
    const double *w5;                          // [n_times][6]
    const int *seg;                            // [n_times]
    const ObsBlock *obs;                       // radius[K] rounded through float32
    const float *pos_vel;                      // [K][6] of this tick
    const double *pos_f64;                     // [K][3] of this tick: the stage's positions in doubles
    unsigned char *row;
};
hipError_t launch_obstacle_record(const ObstacleRecordArgs &a, hipStream_t st);
// summaries of `rows` track rows of row_bytes each: min_ratio = 1e300, below_one = 0
hipError_t launch_obstacle_track_init(unsigned char *rows, size_t row_bytes, int n_rows, hipStream_t st);

// The map's products from a device-resident occupancy grid (lsc_map.hip; the statements are lsc_map.hpp's): the distance field, then -- for
// a context with agents -- one integral image and one goal occupancy grid per distinct radius.  A chain of small launches on `st`: no
// allocation, no synchronise.  Everything the chain writes is written whole, so a rebuild needs nothing cleared.
struct MapArgs {
    int nx, ny, nz;                            // the field
    int md, trunc2;                            // truncation in cells and its square
    const unsigned char *occ;                  // [nx][ny][nz], non-zero: occupied
    unsigned short *pass_a, *pass_b;           // [nx][ny][nz] workspaces of the passes
    const float *table;                        // [trunc2 + 1] metres of a squared lattice distance
    float *edt;                                // [nx][ny][nz] out
    int n_radii;                               // 0: the distance field only
    const double *thr_blocked;                 // [n_radii] r + world_resolution / 2 - 1e-5
    const double *thr_goal;                    // [n_radii] r + grid_margin
    int *integral;                             // [n_radii][(nx+1)][(ny+1)][(nz+1)] out
    int H, W, A;                               // the goal planner's grid; goal_occ null: the context plans no goals on this map
    const int *cell_of;                        // [H + W + A] field cell of a grid index along x | y | z, -1: outside the field
    unsigned char *goal_occ;                   // [n_radii][H W A] out, index H W k + W i + j
};
hipError_t launch_map_build(const MapArgs &a, hipStream_t st);
struct MapBoxes;                               // lsc_map.hpp
// the edits of one update, applied to occ [nx][ny][nz] in front of a rebuild
hipError_t launch_map_edit(unsigned char *occ, int nx, int ny, int nz, const MapBoxes &boxes, hipStream_t st);

}  // namespace lsc
