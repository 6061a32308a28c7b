// lsc_abi.cpp -- C ABI (include/lsc_planner_amd.h) over the gfx950 kernels.  Host side only: builds the
// per-context constants once (what TrajOptimizer's constructor does per agent in the reference,
// src/traj_optimizer.cpp:4-25), owns HBM buffers and persistent per-agent state, launches kernels.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types and prototypes only: the library itself is bound at run time (see rccl_api())
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/lsc_planner_amd.h"
#include "lsc_kernels.h"
#include "lsc_rules.hpp"
#include "lsc_flight.hpp"
#include "lsc_obstacle_motion.hpp"
#include "lsc_map.hpp"
#include "lsc_device_mem.hpp"

using namespace lsc;

namespace {

int binom(int n, int k)
{
    if (k < 0 || k > n) return 0;
    long r = 1;
    for (int i = 1; i <= k; i++) r = r * (n - k + i) / i;
    return (int)r;
}

// Q_base = B Z B^T dt^(-2 phi + 1), phi = 3, phi_n = 1   (src/traj_optimizer.cpp:169-184; B from
// include/polynomial.hpp:415-426)
void build_qbase(double dt, double Q[NC * NC])
{
    const int n = DEG, phi = 3;
    double B[NC][NC], Z[NC][NC], T[NC][NC];
    for (int i = 0; i <= n; i++)
        for (int j = 0; j <= n; j++) B[i][j] = j >= i ? binom(n, i) * binom(n - i, n - j) * (((j - i) & 1) ? -1.0 : 1.0) : 0.0;
    auto fall = [](int a, int p) { if (a < p) return 0; int c = 1; for (int i = 0; i < p; i++) c *= a - i; return c; };
    for (int i = 0; i <= n; i++)
        for (int j = 0; j <= n; j++) {
            int den = i + j - 2 * phi + 1;
            Z[i][j] = den > 0 ? (double)fall(i, phi) * fall(j, phi) / den : 0.0;
        }
    for (int i = 0; i <= n; i++)
        for (int j = 0; j <= n; j++) { double s = 0; for (int l = 0; l <= n; l++) s += B[i][l] * Z[l][j]; T[i][j] = s; }
    const double sc = std::pow(dt, -2 * phi + 1);
    for (int i = 0; i <= n; i++)
        for (int j = 0; j <= n; j++) { double s = 0; for (int l = 0; l <= n; l++) s += T[i][l] * B[j][l]; Q[i * NC + j] = s * sc; }
}

struct HostModel {
    Model m;
    std::vector<uint32_t> terms;
    std::vector<uint32_t> entries;
};

void build_model(const lsc_config &cfg, HostModel &H)
{
    Model &m = H.m;
    std::memset(&m, 0, sizeof(m));
    m.dt = cfg.dt; m.w_c = cfg.control_weight; m.w_t = cfg.terminal_weight;
    m.hv_scale = cfg.dt / DEG;
    m.ha_scale = cfg.dt * cfg.dt / (DEG * (DEG - 1));
    double Q[NC * NC];
    build_qbase(cfg.dt, Q);
    for (int i = 0; i < NC * NC; i++) m.Qh[i] = 2.0 * cfg.control_weight * Q[i];

    // x_t as a combination of the 13 free variables of an axis (see lsc_model.hpp)
    double Zm[SEGV][NYA];
    std::memset(Zm, 0, sizeof(Zm));
    for (int mm = 0; mm < M; mm++)
        for (int i = 0; i < NC; i++) {
            const int t = mm * NC + i;
            if (mm == M - 1 && i >= 3) { Zm[t][NYL] = 1.0; continue; }       // stop at the horizon
            if (i >= 3) { Zm[t][3 * mm + (i - 3)] = 1.0; continue; }
            if (mm == 0) continue;                                         // fixed by the current state
            const int u3 = 3 * (mm - 1), u4 = u3 + 1, u5 = u3 + 2;          // c_{m-1,3..5}
            if (i == 0) Zm[t][u5] = 1.0;
            if (i == 1) { Zm[t][u5] = 2.0; Zm[t][u4] = -1.0; }
            if (i == 2) { Zm[t][u5] = 4.0; Zm[t][u4] = -4.0; Zm[t][u3] = 1.0; }
        }
    for (int t = 0; t < SEGV; t++) {
        int n = 0;
        for (int a = 0; a < NYA; a++)
            if (Zm[t][a] != 0.0) { m.x_i[t][n] = a; m.x_c[t][n] = Zm[t][a]; n++; }
        m.x_n[t] = n;
    }
    for (int a = 0; a < NYA; a++) {
        int n = 0;
        for (int t = 0; t < SEGV; t++)
            if (Zm[t][a] != 0.0) { m.t_t[a][n] = t; m.t_c[a][n] = Zm[t][a]; n++; }
        m.t_n[a] = n;
    }
    // Hc = Z^T blockdiag(Qh) Z
    for (int a = 0; a < NYA; a++)
        for (int b = 0; b < NYA; b++) {
            double s = 0;
            for (int mm = 0; mm < M; mm++)
                for (int i = 0; i < NC; i++)
                    for (int j = 0; j < NC; j++) s += Zm[mm * NC + i][a] * m.Qh[i * NC + j] * Zm[mm * NC + j][b];
            m.Hc[a * NYA + b] = s;
        }

    for (int t = 0; t < SEGV; t++)
        for (int a = 0; a < NYA; a++) m.gzt[t * NYA + a] = Zm[t][a];
    // inverse of the axis block of the reduced cost Hessian for T = 1 .. M terminal segments (Model::ginv): Gauss-Jordan with partial
    // pivoting in long double (the block is positive definite: a plan whose jerk cost vanishes is fixed by the initial state)
    for (int T = 1; T <= M; T++) {
        long double A[NYA][2 * NYA];
        for (int a = 0; a < NYA; a++) {
            for (int b = 0; b < NYA; b++) { A[a][b] = m.Hc[a * NYA + b]; A[a][NYA + b] = a == b ? 1.0L : 0.0L; }
            const int mterm = a == NYL ? M - 1 : ((a % 3) == 2 ? a / 3 : -1);       // y_a is c_{m,5} (or the last segment's end point)
            if (mterm >= M - T) A[a][a] += 2.0L * cfg.terminal_weight;
        }
        for (int c = 0; c < NYA; c++) {
            int piv = c;
            for (int r = c + 1; r < NYA; r++) if (fabsl(A[r][c]) > fabsl(A[piv][c])) piv = r;
            if (piv != c) for (int j = 0; j < 2 * NYA; j++) std::swap(A[c][j], A[piv][j]);
            const long double d = A[c][c];
            for (int j = 0; j < 2 * NYA; j++) A[c][j] /= d;
            for (int r = 0; r < NYA; r++) {
                if (r == c) continue;
                const long double f = A[r][c];
                if (f != 0.0L) for (int j = 0; j < 2 * NYA; j++) A[r][j] -= f * A[c][j];
            }
        }
        for (int a = 0; a < NYA; a++)
            for (int b = 0; b < NYA; b++) m.ginv[T - 1][a * NYA + b] = (double)(0.5L * (A[a][NYA + b] + A[b][NYA + a]));
        for (int t = 0; t < SEGV; t++)
            for (int a = 0; a < NYA; a++) {
                double acc = 0.0;
                for (int j = 0; j < m.x_n[t]; j++) acc += m.x_c[t][j] * m.ginv[T - 1][a * NYA + m.x_i[t][j]];
                m.ghz[T - 1][t * NYA + a] = acc;
            }
        // unconstrained optimum as a linear map of (s0, goal): gradient at y = 0 in x-space = Qh (segment 0) x0 - 2 w_t goal on the terminal points
        for (int j = 0; j < 4; j++) {
            long double gy[NYA];
            for (int b = 0; b < NYA; b++) {
                long double acc = 0.0L;
                if (j < 3) { for (int t = 0; t < NC; t++) acc += (long double)Zm[t][b] * (long double)m.Qh[t * NC + j]; }
                else { for (int mm = M - T; mm < M; mm++) acc += (long double)Zm[mm * NC + DEG][b] * (-2.0L * cfg.terminal_weight); }
                gy[b] = acc;
            }
            for (int a = 0; a < NYA; a++) {
                long double acc = 0.0L;
                for (int b = 0; b < NYA; b++) acc += (long double)m.ginv[T - 1][a * NYA + b] * gy[b];
                m.gy0[T - 1][a * 4 + j] = (double)(-acc);
            }
        }
    }

    // Hessian assembly terms: K[(k,a),(k',b)] += Z[t][a] Z[t'][b] * Wx[(k,t),(k',t')]
    auto scomp = [](int k, int kk) { if (k > kk) std::swap(k, kk); return k == 0 ? kk : (k == 1 ? 2 + kk : 5); };  // xx xy xz yy yz zz
    auto axis_of = [](int g) { return yaxis(g); };
    auto var_of = [](int g) { return yvar(g); };
    H.terms.clear(); H.entries.clear();
    int n_entries = 0;
    for (int gi = 0; gi < NY; gi++)
        for (int gj = 0; gj <= gi; gj++) {
            const int k = axis_of(gi), kk = axis_of(gj), a = var_of(gi), b = var_of(gj);
            std::map<int, int> acc;  // src -> integer coefficient
            for (int p = 0; p < m.t_n[a]; p++)
                for (int q = 0; q < m.t_n[b]; q++) {
                    const int t = m.t_t[a][p], tt = m.t_t[b][q];
                    const int c = (int)std::lround(m.t_c[a][p] * m.t_c[b][q]);
                    if (t == tt) {
                        acc[W_S + t * 6 + scomp(k, kk)] += c;
                        if (k == kk) acc[W_D + k * SEGV + t] += c;
                    } else if (k == kk && t / NC == tt / NC) {
                        const int lo = t < tt ? t : tt, df = t < tt ? tt - t : t - tt;
                        if (df == 1) acc[W_1 + k * SEGV + lo] += c;
                        if (df == 2) acc[W_2 + k * SEGV + lo] += c;
                    }
                }
            bool any = false;
            for (auto &kv : acc) if (kv.second != 0) any = true;
            const bool structural = any || (k == kk && m.Hc[a * NYA + b] != 0.0);
            if (gi - gj > BAND) {
                if (structural) { std::fprintf(stderr, "lsc: band violated (%d,%d)\n", gi, gj); std::abort(); }
                continue;
            }
            // every position of the band gets an entry, also the structurally zero ones: the Cholesky factor is
            // published in place and fills the band, so each assembly must rewrite all of it
            H.entries.push_back(((uint32_t)gi << 16) | (uint32_t)gj);
            H.entries.push_back((uint32_t)H.terms.size());
            for (auto &kv : acc) {
                if (kv.second == 0) continue;
                if (kv.second < -128 || kv.second > 127 || kv.first >= 1024) { std::fprintf(stderr, "lsc: term overflow\n"); std::abort(); }
                H.terms.push_back(((uint32_t)gi << 0) * 0u | ((uint32_t)kv.first << 8) | (uint32_t)(kv.second + 128));
            }
            n_entries++;
        }
    H.entries.push_back(0);
    H.entries.push_back((uint32_t)H.terms.size());
    m.n_entries = n_entries;
    m.n_terms = (int)H.terms.size();
    for (int k = 0; k < 3; k++) { m.world_min[k] = cfg.world_min[k]; m.world_max[k] = cfg.world_max[k]; }
    m.use_sfc = cfg.use_octomap;
    m.prune = cfg.prune;
    m.max_iters = cfg.max_iters > 0 ? cfg.max_iters : 50;
    m.dx_tol = 2e-8;
    m.gap_tol = cfg.gap_tolerance > 0.0 ? cfg.gap_tolerance : 1e-9;
    m.ws_mu0 = cfg.warm_start_mu >= 0.0 ? cfg.warm_start_mu : 0.03;
    m.dim2 = cfg.world_dimension == 2 ? 1 : 0;
    m.z2d = (double)(float)cfg.world_z_2d;
    int n = 0;
    for (int sl = 0; sl < AXROWS; sl++) {
        const int type = sl / NV, k = (sl % NV) / SEGV, t = (sl % NV) % SEGV, mm = t / NC, i = t % NC;
        const bool valid = type < 2 ? !(mm == 0 && i < 3) : (type < 4 ? (i <= 4 && !(mm == 0 && i < 2)) : (i <= 3 && !(mm == 0 && i == 0)));
        if (valid && !(m.dim2 && k == 2)) m.amap[n++] = (unsigned short)sl;      // planar world: `for (k < dim)`, src/traj_optimizer.cpp:274, 469
    }
    if (n != (m.dim2 ? AXVALID_2D : AXVALID_3D)) { std::fprintf(stderr, "lsc: axis row count %d\n", n); std::abort(); }
    m.n_ax = n;
    for (int i = 0; i < n; i++) {
        const uint32_t sl = m.amap[i], type = sl / NV, kt = sl % NV;
        m.amap32[i] = sl | (type << 10) | ((kt / SEGV) << 13) | ((kt % SEGV) << 15);
    }
    for (int v = 0; v < NV; v++) {
        const int k = v / SEGV, t = v % SEGV;
        m.xgp32[v] = (uint32_t)yglob(k, m.x_i[t][0]) | ((uint32_t)yglob(k, m.x_i[t][1]) << 8) | ((uint32_t)yglob(k, m.x_i[t][2]) << 16);
    }
    for (int t = 0; t < SEGV; t++)
        for (int j = 0; j < 3; j++) m.xtcm[t][j] = m.x_n[t] < j + 1 ? 0.0 : m.x_c[t][j];
    m.sigma_pow = 3;
    // (no environment overrides: everything that changes the solve is an lsc_config field)
}

// dense elimination tables of the alternate-mode kernel: axis-major y, with (LSC) or without (BVC) the stop rows
void build_gmodel(const lsc_config &cfg, const Model &m, GModel &g)
{
    std::memset(&g, 0, sizeof(g));
    const bool stop = cfg.planner_mode == 0;
    g.nya = stop ? NYA : GNYA;
    for (int mm = 0; mm < M; mm++)
        for (int i = 0; i < NC; i++) {
            const int t = mm * NC + i;
            if (mm == M - 1 && i >= 3) { g.Z[t][stop ? NYL : NYL + (i - 3)] = 1.0; continue; }
            if (i >= 3) { g.Z[t][3 * mm + (i - 3)] = 1.0; continue; }
            if (mm == 0) continue;
            const int u3 = 3 * (mm - 1), u4 = u3 + 1, u5 = u3 + 2;
            if (i == 0) g.Z[t][u5] = 1.0;
            if (i == 1) { g.Z[t][u5] = 2.0; g.Z[t][u4] = -1.0; }
            if (i == 2) { g.Z[t][u5] = 4.0; g.Z[t][u4] = -4.0; g.Z[t][u3] = 1.0; }
        }
    for (int a = 0; a < g.nya; a++)
        for (int b = 0; b < g.nya; b++) {
            double s = 0;
            for (int mm = 0; mm < M; mm++)
                for (int i = 0; i < NC; i++)
                    for (int j = 0; j < NC; j++) s += g.Z[mm * NC + i][a] * m.Qh[i * NC + j] * g.Z[mm * NC + j][b];
            g.Hc[a * GNYA + b] = s;
        }
}

}  // namespace

// Device memory of a context, grouped by lifetime.  Every group is replaced as a whole (assigning a fresh value frees what it owned)
// and its default value is "nothing allocated, nothing configured".  A new buffer is added to the group of its lifetime, nowhere else.

// context lifetime: released in lsc_destroy only
struct CtxMem {
    DevBuf<Model> d_model;
    DevBuf<GModel> d_gmodel;             // alternate planner modes (lsc_general.hip)
    DevBuf<uint32_t> d_terms, d_entries;
    DevBuf<double> d_trace;
    DevBuf<long long> d_stamps;          // [stamp_slots][2] clock stamps of the timed plan groups (lsc_ctx::stamp_slots), allocated by the first lsc_set_timing(1)
};

// map lifetime: the goal planner with a distance field (lsc_goal.hip); replaced by build_goal_grid
struct MapMem {
    DevBuf<float> d_edt, d_goal_planned, d_ray_stack;
    DevBuf<unsigned char> d_occ_static;
    DevBuf<int> d_goal_err, d_goal_flags, d_goal_exp;
    DevBuf<uint32_t> d_fcode;            // Key32 table of the goal search (lsc_ctx::h_fcode)
    DevBuf<unsigned char> d_goal_ws;     // the HBM search's workspace: lsc_ctx::goal_ws_bytes per agent, allocated for goal_ws_agents agents
    int goal_ws_agents = 0;
    DevBuf<int> d_goal_storage;
};

// occupancy lifetime: a map whose source is a device-resident occupancy grid (lsc_set_occupancy, lsc_map.hip).  Replaced by every
// lsc_set_occupancy, dropped by lsc_set_distmap; it outlives the swarm (lsc_set_agents keeps the map).  d_occ empty: the context's map,
// if it has one, came from lsc_set_distmap and nothing here is read.  The thresholds and index tables follow the swarm and the goal grid
// (build_integrals / build_goal_grid size them); lsc_map_update* allocate nothing.
struct OccMem {
    DevBuf<unsigned char> d_occ;         // [nx][ny][nz]
    DevBuf<unsigned short> d_pass_a, d_pass_b;
    DevBuf<float> d_table, d_edt;        // metres of a squared lattice distance [md^2 + 1]; the distance field (GoalArgs::edt reads it too)
    DevBuf<double> d_thr;                // [2][n_radii] blocked | goal thresholds
    DevBuf<int> d_cell_of;               // [H + W + A] MapArgs::cell_of
    int md = 0, n_radii = 0;
};

// obstacle lifetime: the mission's dynamic obstacles and everything sized by N - 1 + K; replaced by every lsc_set_obstacles (and dropped with
// the swarm).  K == 0: the context has none, and plans exactly as a context that never had any.
struct ObsMem {
    int K = 0;
    int cap = 0;                         // rows of the LDS pass with N - 1 + K obstacles per agent (lsc_ctx::cap while the obstacles are set)
    DevBuf<ObsBlock> d_block;            // what the kernels read (PlanArgs::obs)
    DevBuf<float> d_pos_vel;             // [K][6] the context's own copy of the states (lsc_obstacle_states)
    PinnedBuf<ObsBlock> h_block;         // host image of d_block, uploaded in front of the next tick when `block_dirty`
    PinnedBuf<float> h_pos_vel;          // [K][6] staged states, uploaded in front of the next tick when `states_pending`
    bool block_dirty = false, states_pending = false, have_states = false;
    hipStream_t upload_stream = nullptr; // an upload from the pinned images may still be in flight on this stream (obstacle_uploads_done)
    bool upload_in_flight = false;
    DevBuf<float> d_onormal;             // dense dumps [count][N-1+K][M][3] / [6], allocated by the first tick that asks for them
    DevBuf<double> d_od;
    DevBuf<unsigned char> d_spill;       // second pass: row workspaces for 27 (N - 1 + K) rows
    size_t spill_stride = 0;
    int spill_slots = 0;
    // lsc_set_obstacles_ex: the context may run the disturbance checks (reset_threshold > 0) with these obstacles
    bool reset_served = false;
    DevBuf<double> d_size;               // [K][M][6] predicted sizes (rule_obstacle_size), formed once on the host (ObsBlock::size)
    DevBuf<unsigned char> d_gen_ws;      // alternate-mode workspaces for N - 1 + K obstacles per agent (SwarmMem::gen_slots of them), when the
    size_t gen_stride = 0;               // context has any (SwarmMem::d_gen_ws)
    // motion models (lsc_obstacle_motion): the stage's table; empty: the caller feeds the states.  The clock is the simulator's pair of
    // statements: a tick that runs the stage evaluates at clock_now - clock_start, then clock_now += clock_step
    DevBuf<ObstacleEntry> d_models;
    DevBuf<double> d_pos_f64;            // [K][3] the stage's positions before the rounding to float32 (lsc_obstacle_positions_read, the track)
    std::vector<ObstacleEntry> h_models; // host image (the walk's bound is checked on the host in front of every tick)
    bool have_clock = false;
    double clock_start = 0.0, clock_now = 0.0, clock_step = 0.0;
    // chasing and gaussian models (lsc_obstacle_motion_ex): with at least one the ticks launch lsc_obstacle_step_kernel instead of
    // lsc_obstacle_kernel.  The parameter tables are indexed by the obstacle (rows of other kinds are zeros)
    int n_chasers = 0, n_walkers = 0;
    DevBuf<ObstacleChaser> d_chasers;    // [K]
    DevBuf<ObstacleWalker> d_walkers;    // [K]
    DevBuf<double> d_acc;                // the walkers' acceleration histories, one behind the other, [.][3]
    DevBuf<double> d_chaser_state;       // [K][7] pos | vel | t_last; start, 0, 0 at installation
    std::vector<ObstacleChaser> h_chasers;
    std::vector<ObstacleWalker> h_walkers;
    bool no_step_yet = true;             // no stage has run since the installation: a chaser's previous obstacles are zeros
    double chaser_t_last = 0.0;          // t_last of every chaser (each stage steps them all): a tick below it is refused
};

// mission lifetime: the goal stage's tables (lsc_mission.hip); replaced by every lsc_mission_open, emptied by lsc_mission_close (and
// dropped with the swarm).  Not open and no rule table: the ticks launch no stage.
struct MissionMem {
    bool open = false;
    int planner_state = LSC_MISSION_GOTO;
    DevBuf<float> d_tables;              // desired | start | mission start | mission goal, [N][3] each
    DevBuf<int> d_legs;                  // [N] swaps made
    DevBuf<float> d_rule_goal;           // [N][3] the right-hand rule's current goals, allocated by the first tick that flies the rule
};

// swarm lifetime: replaced by lsc_set_agents (free_agents)
struct SwarmMem {
    DevBuf<double> d_radius, d_radius_obs, d_downwash, d_downwash_obs, d_vmax, d_amax, d_vnom;
    DevBuf<float> d_stale, d_sfc, d_goal_cur;
    DevBuf<int> d_sfc_init, d_sfc_err, d_img_of_agent, d_integral;
    DevBuf<int> d_nrows, d_bmax, d_order;
    DevBuf<float> d_obs_bound;
    DevBuf<long long> d_iters_acc, d_prof;
    DevBuf<double> d_dbg;
    // host-pointer tick: inputs and outputs travel as ONE copy each, through pinned staging buffers.
    //   d_state | d_goal | d_prev  are consecutive in d_in (in_block_floats),
    //   d_cost | d_next | d_status | d_iters  in d_out (out_block_bytes)
    DevBuf<float> d_in;
    DevBuf<unsigned char> d_out;
    float *d_state = nullptr, *d_goal = nullptr, *d_prev = nullptr, *d_next = nullptr;
    double *d_cost = nullptr;
    int *d_status = nullptr, *d_iters = nullptr;
    PinnedBuf<float> h_in;
    PinnedBuf<unsigned char> h_out;
    DevBuf<float> d_onormal;             // dense constraint dumps, allocated by the first tick that asks for them
    DevBuf<double> d_od;
    DevBuf<unsigned char> d_spill;       // HBM row workspaces of the second pass (agents beyond the LDS row capacity)
    size_t spill_stride = 0;
    int spill_slots = 0;
    DevBuf<unsigned char> d_ever, d_gen_ws;      // alternate planner modes (lsc_general.hip)
    size_t gen_stride = 0;
    int gen_slots = 0;
    // neighbour lists of large swarms (lsc_neigh.hip): one allocation (base neigh.seg_bound ... see lsc_set_agents); neigh.cnt == nullptr: not in use
    DevBuf<unsigned char> d_neigh;
    DevBuf<long long> d_neigh_prof;      // (neigh.prof)
    NeighArgs neigh = {};
    DevBuf<unsigned char> d_safety;      // lsc_safety_ratio's buffers
    // the flight log (lsc_flight_begin): a header of FLIGHT_HEADER_BYTES -- the weights w5 | w4 | w3 and the segments of the record times, each
    // sized for FLIGHT_MAX_TIMES -- then flight_capacity rows of flight_row_bytes (lsc_flight.hpp: flight_layout).  Empty: no log is open
    DevBuf<unsigned char> d_flight;
    int flight_capacity = 0, flight_times = 0, flight_what = 0, flight_flown = 0;
    size_t flight_row_bytes = 0;
    hipStream_t flight_stream = nullptr; // the stream last flown on (lsc_flight_read synchronises it)
    // the obstacle track beside the log (lsc_flight_begin on a context with motion models): flight_capacity rows of track_row_bytes
    // (lsc_obstacle_motion.hpp: obstacle_track_layout), sized for track_K obstacles.  Empty: the log has no track
    DevBuf<unsigned char> d_track;
    size_t track_row_bytes = 0;
    int track_K = 0;
    DevBuf<long long> d_goal_prof;
    DevBuf<int> d_goal_path, d_goal_plen;
    DevBuf<int> d_ws_peak;               // [N] lsc_working_set_peaks (empty until asked for: the plan kernel then stores nothing)
    MapMem map;
    ObsMem obs;
    MissionMem mission;
};

// the two blocks of the host-pointer tick: floats of the input block of n agents, bytes of the output block of `rows` table rows
static constexpr size_t in_block_floats(size_t n) { return (9 + 3 + NV) * n; }
static constexpr size_t out_block_bytes(size_t rows) { return (sizeof(double) + sizeof(float) * NV + 2 * sizeof(int)) * rows; }
// header of the flight log: byte offsets of the weights and segments
static constexpr size_t FLIGHT_W5 = 0, FLIGHT_W4 = FLIGHT_W5 + 8 * 6 * FLIGHT_MAX_TIMES, FLIGHT_W3 = FLIGHT_W4 + 8 * 5 * FLIGHT_MAX_TIMES,
                        FLIGHT_SEG = FLIGHT_W3 + 8 * 4 * FLIGHT_MAX_TIMES, FLIGHT_HEADER_BYTES = 8192;
static_assert(FLIGHT_SEG + 4 * FLIGHT_MAX_TIMES <= FLIGHT_HEADER_BYTES, "the header holds the tables of 64 record times");
constexpr int TIMED_GROUPS = 7;          // `which` of lsc_kernel_time_ms: 0..4 and 6 are event pools (5 is the host's wall clock)

struct lsc_ctx {
    lsc_config cfg;
    HostModel hm;
    int N = 0, first = 0, count = 0, cap = 0, cap_tp = 0, n_cu = 256;
    int cap_agents = 0;                  // cap of the swarm alone (lsc_set_agents): what cap returns to when the obstacles go
    size_t smem_tp = 0;
    std::string err;
    std::string note;                    // informational remarks of lsc_create (not errors): lsc_last_note
    bool timing = false;
    CtxMem own;
    SwarmMem swarm;
    int last_host_seq = 0;               // planner_seq of the last host-buffer tick (lsc_dump_qp reads its inputs back)
    bool next_has_all_rows = false;      // d_next holds the new plan of ALL N agents (whole-swarm shard, or lsc_replan_tick_all's gather)
    bool h_ever_stale = false;           // device-resident ticks ran since h_ever was last in step with d_ever
    std::vector<unsigned char> h_ever;   // host mirror for the host-buffer ticks (they decide on the host whether anybody is off plan)
    std::vector<float> h_edt;   // host copy of the distance field (integral images are rebuilt when agents change)
    OccMem occ;                 // ... or the map's source is a device occupancy: h_edt is empty and the products are rebuilt on the device
    int edt_dims[3] = {0, 0, 0}, edt_kmin[3] = {0, 0, 0};
    double edt_res = 0.0;
    std::vector<double> h_radius;
    int goal_path_cap = 0;
    std::vector<uint32_t> h_fcode;       // Key32 table of the goal search (empty: Key64)
    int fcode_rb = 0;
    bool goal_profiling = false;
    int grid_dims[3] = {0, 0, 0}, grid_row_cap = 0;
    double grid_min[3] = {0, 0, 0};
    std::vector<int> nb_seq;
    // the HBM search of the goal planner: 0 none (the LDS search, restarted in HBM when goal_ws_bytes > 0), 1 / 2 the HBM search with
    // the cell bytes in LDS / in the workspace; goal_ws_bytes per agent
    int goal_hbm = 0;
    size_t goal_ws_bytes = 0;
    bool neigh_always = false;           // LSC_NEIGH_ALWAYS (measurements, tests): lists whenever the context has them, not only where they pay
    const char *neigh_skipped = "no tick has run since lsc_set_agents";      // why the last tick did not launch the kernels of lsc_neigh.hip;
                                         // null: it did, and their outputs are this tick's (lsc_neighbour_dump)
    bool general_handover = false;       // LSC_GENERAL_HANDOVER (tests, measurements): disturbed agents always go through a launch of
                                         // lsc_general_kernel, never through the plan kernel's own general_fold
    int last_general = 0;                // how the last tick reached the alternate-mode solver (lsc_general_info): 0 not at all, 1 folded into the
                                         // plan kernel, 2 a launch of lsc_general_kernel, 3 one of lsc_general_batch_kernel
    bool generic_lsc_build = false;      // LSC_GENERIC_LSC_BUILD (tests, measurements): phase B of the plan kernel never takes the one-wave-per-segment
                                         // build of small swarms (PlanArgs::generic_lsc_build)
    bool plain_handover = true;          // the step of the active-set solve loads the chosen row itself (PlanArgs::plain_handover); LSC_SOLVE_ROW_RECORD
                                         // (tests, measurements): it takes the record the search publishes instead
    bool step_all_slots = false;         // LSC_STEP_ALL_SLOTS (tests, measurements): the active-set solve runs every change over all slots of the
                                         // working set instead of a size class (PlanArgs::step_all_slots)
    int goal_rule = LSC_GOAL_RULE_CONFIG;    // lsc_set_goal_rule: a context setting (the rule's table belongs to the swarm: MissionMem)
    int deadlock_seq_threshold = 5;
    double deadlock_velocity_threshold = 0.1;
    int trace_agent = -1;
    bool profiling = false;
    hipStream_t stream = nullptr;
    // Kernel timing.  The plan group (which = 0) is timed by clock stamps that its kernels write into a slot of own.d_stamps (lsc_kernels.h:
    // LaunchEvents): slot i = {begin, end}, armed to {INT64_MAX, INT64_MIN} by lsc_set_timing(1) and never touched by the host between
    // ticks; the samples are read with one copy on query.  Every other group, and a plan group without a slot (nothing to launch, the slots
    // used up, LSC_TIMING_EVENTS), has one HIP event pair per launch, bound to its dispatches and read back on query.
    int stamp_slots = 4096;              // LSC_TIMING_SLOTS
    // Launch groups whose plan launch has more workgroups than this ride on events: every workgroup's two atomics go to ONE 16-byte slot
    // and workgroups leave in bursts.  Measured (profiles/timing_stamps_ab.log): 64 workgroups, a timed tick 0.3 us above an untimed one
    // (events: 4.4); 256 (four missions in one launch) 2.8 us above (events: 5.9).  256 is the largest group a gain was measured for;
    // beyond it only batches of more than four 64-agent missions get here (a shard of more than 256 agents takes the throughput kernels,
    // which stamp nothing), and nothing was measured there.
    int stamp_max_workgroups = 256;      // LSC_TIMING_STAMP_WORKGROUPS (tests, measurements)
    size_t stamp_used = 0;
    bool timing_events = false;          // LSC_TIMING_EVENTS: the plan group rides on events as the others do (the A/B arm of the stamps, and the fallback)
    std::vector<int> plan_samples;       // the plan group's samples in launch order: >= 0 a stamp slot, < 0: ~(index of its pair in ev_pool[0])
    hipStream_t stamp_stream = nullptr;  // the stream the last stamped group was launched on (whoever reads or re-arms the slots synchronises it)
    double clock_khz = 0.0;              // rate of the clock the kernels stamp with (hipDeviceAttributeWallClockRate)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool[TIMED_GROUPS];   // 0 plan kernel(s), 1 dense sweep, 2 trajectory exchange, 3 goal kernel, 4 corridor kernel, 6 flight record (5 unused)
    std::vector<double> host_tick_ms;    // which = 5: wall clock of every lsc_replan_tick since lsc_set_timing(1), entry to return
    size_t ev_used[TIMED_GROUPS] = {0, 0, 0, 0, 0, 0, 0};
    // agent-sharded multi-GPU: this context is rank `rank` of `world`; every rank owns a block of shard_rows agents of a
    // table padded to table_rows = shard_rows * world rows, so that the exchange is ONE in-place equal-sized all-gather
    int world = 1, rank = 0, shard_rows = 0, table_rows = 0;
    ncclComm_t comm = nullptr;
};

// RCCL is bound with dlopen instead of a link-time dependency: inside a PyTorch process the wheel's own librccl (and
// HIP runtime) is already mapped and must be the one that is used -- two RCCL copies in one process would each bring
// their own view of the devices; stand-alone C++ users (lsc_sim) get /opt/rocm's.
struct RcclApi {
    void *h = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};

static bool rccl_bind(RcclApi &api);
static const RcclApi *rccl_api()
{
    static RcclApi api;
    static std::once_flag once;                               // contexts may be created from several threads
    std::call_once(once, [] { (void)rccl_bind(api); });
    return api.h ? &api : nullptr;
}
static bool rccl_bind(RcclApi &api)
{
    const char *names[] = {"librccl.so.1", "librccl.so"};
    void *h = nullptr;
    for (const char *n : names) if (!h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);   // the copy the process already has
    for (const char *n : names) if (!h) h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return false;
    api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    api.AllGather = reinterpret_cast<decltype(api.AllGather)>(dlsym(h, "ncclAllGather"));
    api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(h, "ncclAllReduce"));
    api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(dlsym(h, "ncclGroupStart"));
    api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(dlsym(h, "ncclGroupEnd"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllGather || !api.AllReduce || !api.GroupStart || !api.GroupEnd ||
        !api.GetErrorString)
        return false;
    api.h = h;
    return true;
}

#define NCCLCHK(ctx, api, call)                                                               \
    do {                                                                                      \
        ncclResult_t r_ = (call);                                                             \
        if (r_ != ncclSuccess) {                                                              \
            (ctx)->err = std::string(#call) + ": " + (api)->GetErrorString(r_);               \
            return LSC_ECOMM;                                                                 \
        }                                                                                     \
    } while (0)

static const long long STAMP_ARMED[2] = {INT64_MAX, INT64_MIN};      // a slot nobody has stamped: any clock value is below / above

// slots [0, n) of the context's stamps back to "armed"; the caller has synchronised whatever may still write them
static hipError_t arm_stamps(lsc_ctx *c, size_t n)
{
    if (n == 0) return hipSuccess;
    std::vector<long long> h(2 * n);
    for (size_t i = 0; i < n; i++) { h[2 * i] = STAMP_ARMED[0]; h[2 * i + 1] = STAMP_ARMED[1]; }
    return hipMemcpy(c->own.d_stamps, h.data(), sizeof(long long) * h.size(), hipMemcpyHostToDevice);
}

// The timing of the next launch group `which`, on stream `st`.  Nothing is recorded or written here: the group hands first() to its first
// launch and last() to its last (LaunchEvents, lsc_kernels.h).  The plan group takes the next stamp slot when its plan launch has
// `workgroups` > 0 (the caller knows that its kernels will run: a group that launches nothing has nobody to stamp) and at most
// stamp_max_workgroups of them, the context has slots (lsc_set_timing allocates
// them, unless LSC_TIMING_EVENTS) and one is left; everybody else takes the next event pair of the pool, and the events take the
// dispatches' own timestamps.
static int timing_begin(lsc_ctx *c, int which, LaunchEvents *ev, hipStream_t st = nullptr, int workgroups = 0)
{
    const bool launches = workgroups > 0 && workgroups <= c->stamp_max_workgroups;
    if (which == 0 && launches && !c->timing_events && c->own.d_stamps && c->stamp_used < (size_t)c->stamp_slots) {
        long long *slot = c->own.d_stamps + 2 * c->stamp_used;
        c->plan_samples.push_back((int)c->stamp_used++);
        c->stamp_stream = st;
        ev->t0 = slot;
        ev->t1 = slot + 1;
        return LSC_OK;
    }
    if (c->ev_used[which] == c->ev_pool[which].size()) {
        // (no system-scope release of their own: the events are read for elapsed time only, after hipEventSynchronize; whoever reads the
        // tick's results synchronises the stream, as without timing)
        hipEvent_t a, b;
        if (hipEventCreateWithFlags(&a, hipEventDisableSystemFence) != hipSuccess || hipEventCreateWithFlags(&b, hipEventDisableSystemFence) != hipSuccess) return LSC_EHIP;
        c->ev_pool[which].push_back({a, b});
    }
    if (which == 0) c->plan_samples.push_back(~(int)c->ev_used[which]);      // (behind the pair's creation: a sample always has its source)
    auto &p = c->ev_pool[which][c->ev_used[which]++];
    ev->start = p.first;
    ev->stop = p.second;
    return LSC_OK;
}
// ... for a group whose kernels are not ours (which = 2, the RCCL all-gather): the pair is recorded around it, start here, *e1 behind it
static int timing_begin_recorded(lsc_ctx *c, int which, hipStream_t st, hipEvent_t *e1)
{
    LaunchEvents ev;
    if (timing_begin(c, which, &ev) != LSC_OK) return LSC_EHIP;
    *e1 = ev.stop;
    return hipEventRecord(ev.start, st) == hipSuccess ? LSC_OK : LSC_EHIP;
}

#define HIPCHK(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                   \
            return LSC_EHIP;                                                                  \
        }                                                                                     \
    } while (0)

static int build_integrals(lsc_ctx *c);
static int build_goal_grid(lsc_ctx *c, const std::vector<double> &radii);

extern "C" {

void lsc_default_config(lsc_config *cfg)
{
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->dt = 0.2; cfg->control_weight = 0.01; cfg->terminal_weight = 1.0;
    cfg->world_min[0] = -10; cfg->world_min[1] = -10; cfg->world_min[2] = 0;
    cfg->world_max[0] = 10; cfg->world_max[1] = 10; cfg->world_max[2] = 2.5f;
    cfg->use_octomap = 0; cfg->world_resolution = 0.1; cfg->device = 0;
    cfg->max_rows_per_cp = 0; cfg->max_iters = 50; cfg->prune = 1; cfg->warm_start_mu = 0.03;
    cfg->goal_mode = 0; cfg->goal_threshold = 0.1; cfg->priority_dist_threshold = 0.4; cfg->goal_radius = 2.0;
    cfg->grid_resolution = 0.3; cfg->grid_margin = 0.2;   // launch/testall_forest.launch:88-89
    cfg->horizon = 1.0; cfg->goal_row_cap = 0;
    cfg->planner_mode = 0; cfg->slack_mode = 0; cfg->slack_collision_weight = 100000.0; cfg->n_constraint_segments = -1;
    cfg->reset_threshold = 0.0;
    cfg->gap_tolerance = 1e-9;
    cfg->world_dimension = 3; cfg->world_z_2d = 1.0; cfg->goal_search = 0; cfg->solver = 1;
}

lsc_ctx *lsc_create(const lsc_config *cfg)
{
    if (!cfg || !(cfg->dt > 0)) return nullptr;
    // M = static_cast<int>((horizon + SP_EPSILON) / dt) (src/traj_optimizer.cpp:9, src/traj_planner.cpp:22).  The kernels are unrolled
    // for their segment count: this library plans M segments (liblsc_hip.so: 5, every shipped launch file; liblsc_hip_m4.so: 4, the
    // C++ defaults of src/param.cpp:66-67) and says so instead of silently planning another horizon.
    if ((int)((cfg->horizon + 1e-9) / cfg->dt) != M) {
        std::fprintf(stderr, "lsc_create: horizon %g / dt %g = %d segments, this library plans M = %d (lsc_segments(); the sibling build "
                             "liblsc_hip%s.so plans %d)\n", cfg->horizon, cfg->dt, (int)((cfg->horizon + 1e-9) / cfg->dt), M, M == 5 ? "_m4" : "", M == 5 ? 4 : 5);
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device >= ndev) {
        std::fprintf(stderr, "lsc_create: no usable HIP device (there is no CPU fallback)\n");
        return nullptr;
    }
    if (hipSetDevice(cfg->device) != hipSuccess) return nullptr;
    if (init_device_kernels() != hipSuccess) {
        std::fprintf(stderr, "lsc_create: device %d does not accept the gfx950 kernels' LDS request\n", cfg->device);
        return nullptr;
    }
    if (cfg->planner_mode < 0 || cfg->planner_mode > 1 || cfg->slack_mode < 0 || cfg->slack_mode > 2 ||
        (cfg->planner_mode == 1 && cfg->use_octomap)) {
        // BVC + octomap: the reference's generateSFC throws for every planner mode but LSC (src/traj_planner.cpp:1442-1449)
        std::fprintf(stderr, "lsc_create: unsupported planner_mode / slack_mode combination\n");
        return nullptr;
    }
    lsc_ctx *c = new lsc_ctx();
    c->cfg = *cfg;
    if (c->cfg.planner_mode == 0 && c->cfg.slack_mode != 0) {
        // TrajPlanner::checkPlannerMode (src/traj_planner.cpp:445-448): "LSC does not need slack variables, fix to none".  The
        // slack rows of LSC mode are the ones a disturbance reset leaves behind (obs_slack_indices), nothing else.
        c->cfg.slack_mode = 0;
        c->note = "planner_mode lsc with a slack mode: slack_mode fixed to none (src/traj_planner.cpp:445-448)";
    }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
    }
    build_model(*cfg, c->hm);
    GModel g;
    build_gmodel(*cfg, c->hm.m, g);
    CtxMem &o = c->own;
    const bool ok = hipStreamCreate(&c->stream) == hipSuccess &&
                    o.d_terms.alloc(c->hm.terms.size() + 2) == hipSuccess &&
                    hipMemcpy(o.d_terms, c->hm.terms.data(), sizeof(uint32_t) * c->hm.terms.size(), hipMemcpyHostToDevice) == hipSuccess &&
                    o.d_entries.upload(c->hm.entries.data(), c->hm.entries.size()) == hipSuccess &&
                    o.d_model.alloc(1) == hipSuccess &&       // (filled by lsc_set_agents)
                    o.d_gmodel.upload(&g, 1) == hipSuccess;
    if (!ok) { lsc_destroy(c); return nullptr; }
    return c;
}

// Row capacity of the LDS pass for n_obs obstacles per agent: 27 x max_rows_per_cp rows in total (default min(n_obs, 64) per control
// point), at most what the 160 KiB of a workgroup allow
static int lds_row_capacity(const lsc_ctx *c, int n_obs)
{
    int per_cp = c->cfg.max_rows_per_cp > 0 ? c->cfg.max_rows_per_cp : 64;
    if (per_cp > n_obs) per_cp = n_obs;
    if (per_cp < 1) per_cp = 1;
    constexpr int NBR = NCP - 3;              // control points that carry rows: 27 for M = 5
    int cap = NBR * per_cp;
    while (cap > NBR && plan_smem_bytes(c->hm.m.n_terms, c->hm.m.n_entries, cap) > LDS_MAX_BYTES) cap -= NBR;
    return cap;
}

static void free_agents(lsc_ctx *c)
{
    if (c->swarm.neigh.prof) {
        std::vector<long long> h(8 * (size_t)c->N);
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(h.data(), c->swarm.neigh.prof, sizeof(long long) * h.size(), hipMemcpyDeviceToHost) == hipSuccess) {
            double st[4] = {0, 0, 0, 0}, nq = 0, nc = 0, nu = 0, novf = 0;
            int n = 0;
            for (int q = 0; q < c->N; q++) {
                const long long *p = &h[8 * (size_t)q];
                if (p[4] == 0) continue;
                for (int k = 0; k < 4; k++) st[k] += (double)(p[k + 1] - p[k]) / 100.0;
                nq += (double)(p[5] & 0xffffffff); nc += (double)p[6]; nu += (double)p[7]; novf = (double)(p[5] >> 32); n++;
            }
            if (n) fprintf(stderr, "[lsc] query kernel of the neighbour lists, last tick, mean over %d agents: set-up %.2f us, cells -> candidates %.2f us, sphere tests %.2f us, "
                                   "sorted list %.2f us; %.0f cells, %.0f candidates (%.0f of them from the overflow list), %.0f units per agent\n", n, st[0] / n, st[1] / n, st[2] / n, st[3] / n, nc / n, nq / n, novf, nu / n);
        }
    }
    c->swarm = SwarmMem{};
}

void lsc_destroy(lsc_ctx *c)
{
    if (!c) return;
    if (c->comm) { if (const RcclApi *api = rccl_api()) (void)api->CommDestroy(c->comm); c->comm = nullptr; }
    free_agents(c);
    c->own = CtxMem{};
    for (int w = 0; w < TIMED_GROUPS; w++)
        for (auto &p : c->ev_pool[w]) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *lsc_last_error(const lsc_ctx *c) { return c ? c->err.c_str() : "null context"; }
const char *lsc_last_note(const lsc_ctx *c) { return c ? c->note.c_str() : ""; }
int lsc_segments(void) { return M; }

// Which LSC build phase B of the one-round plan kernel takes with n_obs obstacles per agent -- the other agents and the context's dynamic
// obstacles (lsc_kernels.hip, plan_agent: `placed`) --, as the note's "lsc build:" remark says it.
static const char *lsc_build_named(const lsc_ctx *c, int n_obs)
{
    return c->generic_lsc_build ? "generic pass (LSC_GENERIC_LSC_BUILD)" : (n_obs > 64 ? "generic pass (more than 64 obstacles)" : "one wave per segment");
}

// The "lsc build:" remark of lsc_set_agents speaks of the agents alone.  lsc_set_obstacles changes the number of obstacles per agent, and
// the kernel chooses its build by N - 1 + K: a remark of its own says which build the context takes with its K dynamic obstacles
// (K = 0: the remark goes).  It follows "lsc build: ...; step: ..." and goes with them at the next lsc_set_agents.
static void note_obstacles(lsc_ctx *c, int K)
{
    const std::string head = "; dynamic obstacles: ";
    const size_t at = c->note.find(head);
    if (at != std::string::npos) {
        const size_t to = c->note.find(';', at + head.size());
        c->note.erase(at, (to == std::string::npos ? c->note.size() : to) - at);
    }
    if (K > 0) c->note += head + "K = " + std::to_string(K) + ", " + std::to_string(c->N - 1 + K) + " per agent, " + lsc_build_named(c, c->N - 1 + K);
}

int lsc_set_agents(lsc_ctx *c, int N, const double *radius, const double *downwash, const double *max_vel,
                   const double *max_acc, const double *nominal_vel)
{
    if (!c || N < 1 || !radius || !downwash || !max_vel || !max_acc || !nominal_vel) return LSC_EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    free_agents(c);
    c->N = N;
    // rank's block of the (padded) table; world = 1 without lsc_comm_init: the whole swarm
    c->shard_rows = (N + c->world - 1) / c->world;
    c->table_rows = c->shard_rows * c->world;
    c->first = std::min(c->rank * c->shard_rows, N);
    c->count = std::min(c->shard_rows, N - c->first);
    const size_t Np = (size_t)c->table_rows;
    // Row capacity of the LDS pass: 27 x max_rows_per_cp rows in total (rows are stored compactly, so a control point may
    // hold more than its share), at most what the 160 KiB of a workgroup allow; never more than the 27 (N-1) that exist.
    constexpr int NBR = NCP - 3;              // control points that carry rows: 27 for M = 5
    const int cap = lds_row_capacity(c, N - 1);
    c->cap = c->cap_agents = cap;
    c->hm.m.cap = cap;
    // Throughput build (256 lanes, two workgroups per CU): used when the shard has more agents than the GPU has CUs; its
    // capacity is what fits half a CU's LDS.  (Pointless -- and slower per agent -- for a shard that fits the chip.)
    c->cap_tp = 0; c->smem_tp = 0;
    if (c->cfg.max_rows_per_cp == 0) {
        int ct = NBR;
        while (plan_smem_bytes(c->hm.m.n_terms, c->hm.m.n_entries, ct + NBR, false) <= 80 * 1024 - 512) ct += NBR;
        if (ct < cap && plan_smem_bytes(c->hm.m.n_terms, c->hm.m.n_entries, ct, false) <= 80 * 1024 - 512) {
            c->cap_tp = ct;
            c->smem_tp = plan_smem_bytes(c->hm.m.n_terms, c->hm.m.n_entries, ct, false);
        }
    }
    HIPCHK(c, hipMemcpy(c->own.d_model, &c->hm.m, sizeof(Model), hipMemcpyHostToDevice));
    std::vector<double> r_obs(N), dw_obs(N);
    for (int i = 0; i < N; i++) { r_obs[i] = (double)(float)radius[i]; dw_obs[i] = (double)(float)downwash[i]; }
    SwarmMem &s = c->swarm;
    const size_t n = (size_t)N;
    HIPCHK(c, s.d_radius.upload(radius, n));
    HIPCHK(c, s.d_radius_obs.upload(r_obs.data(), n));
    HIPCHK(c, s.d_downwash.upload(downwash, n));
    HIPCHK(c, s.d_downwash_obs.upload(dw_obs.data(), n));
    HIPCHK(c, s.d_vmax.upload(max_vel, 3 * n));
    HIPCHK(c, s.d_amax.upload(max_acc, 3 * n));
    HIPCHK(c, s.d_vnom.upload(nominal_vel, n));
    HIPCHK(c, s.d_stale.alloc_zero(NV * n));   // TrajOptimizer::trajectory starts at (0,0,0)
    if (c->cfg.world_dimension == 2) {
        // Planar world: an agent whose FIRST solve fails keeps this trajectory (src/traj_planner.cpp:1553-1584).  The reference
        // leaves its z at 0 and overrides the agent's own z with world/z_2d on the next state callback (src/traj_planner.cpp:304-314);
        // here the z block starts at z_2d, so that the stale plan -- and the state propagated from it -- stay in the plane the
        // kernels and the host-buffer ticks' input check rely on (an out-of-plane stale plan used to make every later
        // host-buffer tick of the whole swarm return LSC_EINVAL).
        std::vector<float> init((size_t)NV * N, 0.0f);
        const float z = (float)c->cfg.world_z_2d;
        for (int q = 0; q < N; q++)
            for (int j = 0; j < SEGV; j++) init[(size_t)q * NV + 2 * SEGV + j] = z;
        HIPCHK(c, hipMemcpy(s.d_stale, init.data(), sizeof(float) * init.size(), hipMemcpyHostToDevice));
    }
    HIPCHK(c, s.d_sfc.alloc_zero(M * 6 * n));
    HIPCHK(c, s.d_goal_cur.alloc_zero(3 * Np));
    HIPCHK(c, s.d_sfc_err.alloc_zero(n));
    {
        std::vector<int> ones(N, 1);                        // flag_initialize_sfc = true (src/traj_planner.cpp:48)
        HIPCHK(c, s.d_sfc_init.upload(ones.data(), n));
    }
    c->h_radius.assign(radius, radius + N);
    if (cap < NBR * (N - 1)) {
        // An agent can carry more rows than the LDS capacity holds: those agents are re-planned by a second pass with
        // their rows in HBM (the reference never drops a row, src/traj_optimizer.cpp:437-466).  One workspace per
        // persistent workgroup; 256 = one per CU.
        s.spill_stride = plan_spill_bytes(N - 1);
        s.spill_slots = std::min(N, 256);
        HIPCHK(c, s.d_spill.alloc(s.spill_stride * (size_t)s.spill_slots));
    }
    {
        // alternate modes: persistent "was seen off its plan" flags, and -- when such a QP can occur at all -- the HBM
        // workspaces of lsc_general_kernel (one per persistent workgroup; when the plan kernel folds the hand-over, one per agent of
        // its launch: run_plan folds only launches of at most gen_slots agents)
        HIPCHK(c, s.d_ever.alloc_zero(n));
        c->h_ever.assign(N, 0);
        const bool general_all = c->cfg.planner_mode == 1 || c->cfg.slack_mode != 0;
        if (general_all || c->cfg.reset_threshold > 0.0) {
            s.gen_stride = general_ws_bytes(N);
            s.gen_slots = std::min(N, 256);
            HIPCHK(c, s.d_gen_ws.alloc(s.gen_stride * (size_t)s.gen_slots));
        }
        c->general_handover = getenv("LSC_GENERAL_HANDOVER") != nullptr;
        // how the plan group is timed (lsc_set_timing): by events like the other groups, and how many stamp slots the context gets (tests);
        // the slots are sized when the context's first lsc_set_timing(1) allocates them
        const char *tev = getenv("LSC_TIMING_EVENTS");
        c->timing_events = tev && atoi(tev) != 0;
        if (const char *e = getenv("LSC_TIMING_STAMP_WORKGROUPS")) { const int v = atoi(e); if (v >= 1) c->stamp_max_workgroups = v; }
        if (const char *e = getenv("LSC_TIMING_SLOTS")) { const int v = atoi(e); if (v >= 1 && v <= (1 << 20) && !c->own.d_stamps) c->stamp_slots = v; }
    }
    {
        // which LSC build phase B of the one-round plan kernel takes (lsc_kernels.hip, plan_agent): said in the note, for tests and A/B runs
        c->generic_lsc_build = getenv("LSC_GENERIC_LSC_BUILD") != nullptr;
        const size_t prev = c->note.find("lsc build:");                // (a remark of an earlier lsc_set_agents goes)
        if (prev != std::string::npos) c->note.erase(prev >= 2 ? prev - 2 : prev);
        c->note += (c->note.empty() ? "" : "; ") + std::string("lsc build: ") + lsc_build_named(c, N - 1);
        // ... and how the active-set solve sizes its step (lsc_kernels.hip, gi_solve); the remark follows the one above and goes with it
        c->step_all_slots = getenv("LSC_STEP_ALL_SLOTS") != nullptr;
        c->note += std::string("; step: ") + (c->step_all_slots ? "all slots (LSC_STEP_ALL_SLOTS)" : "size classes");
        // ... and how the search hands the chosen row to the step (search_reduce)
        c->plain_handover = getenv("LSC_SOLVE_ROW_RECORD") == nullptr;
        c->note += std::string("; solve hand-over: ") + (c->plain_handover ? "plain" : "row record (LSC_SOLVE_ROW_RECORD)");
    }
    HIPCHK(c, s.d_nrows.alloc_zero(n));
    HIPCHK(c, s.d_bmax.alloc_zero(n));
    HIPCHK(c, s.d_order.alloc(n));
    HIPCHK(c, s.d_obs_bound.alloc(4 * n));
    c->neigh_skipped = "no tick has run since lsc_set_agents";
    if (N >= NEIGH_MIN_AGENTS && N <= NEIGH_MAX_AGENTS && c->cfg.prune == 1 && !getenv("LSC_NO_NEIGHBOUR_LISTS")) {
        // Neighbour lists (lsc_neigh.hip).  Cell size: what an agent at its velocity limit covers over the horizon + two diameters (1.6 m with
        // the shipped parameters: a query visits ~9 x 9 cells, one lane each, and a bucket's twelve slots hold a crowd four times as dense as
        // the 1024-agent benchmark's); any size is correct, the size only decides how many cells a query visits and how many agents share a
        // bucket.  LSC_NEIGH_CELL overrides it (measurements).
        NeighArgs &g = s.neigh;
        c->neigh_always = getenv("LSC_NEIGH_ALWAYS") != nullptr;
        double vm = 0.0, rm = 0.0, dmin = 1e300, dmax = 0.0;
        for (int i = 0; i < N; i++) {
            for (int k = 0; k < 3; k++) vm = std::max(vm, max_vel[3 * i + k]);
            rm = std::max(rm, radius[i]); dmin = std::min(dmin, dw_obs[i]); dmin = std::min(dmin, downwash[i]);
            dmax = std::max(dmax, dw_obs[i]); dmax = std::max(dmax, downwash[i]);
        }
        double cell = vm * M * c->cfg.dt + 4.0 * rm;
        if (const char *e = getenv("LSC_NEIGH_CELL")) { const double v = atof(e); if (v > 0.0) cell = v; }
        if (!(cell > 1e-3)) cell = 1e-3;
        g.sc_max = std::max(1.0, 1.0 / dmin); g.zscale = std::max(1.0, dmax);
        g.inv_cell = 1.0 / cell; g.inv_cell_z = 1.0 / (cell * g.zscale);
        unsigned H = 1024;
        while (H < 4u * (unsigned)N) H <<= 1;
        g.hmask = H - 1; g.ovf_cap = 4096; g.list_cap = 1024; g.plist_cap = NEIGH_PRIO_CAP; g.tag = 0;
        // (capacities the tests shrink to drive the overflow paths: an agent without a list culls by itself, results do not change)
        if (const char *e = getenv("LSC_NEIGH_OVF_CAP")) { const int v = atoi(e); if (v >= 1 && v <= 65536) g.ovf_cap = v; }
        if (const char *e = getenv("LSC_NEIGH_LIST_CAP")) { const int v = atoi(e); if (v >= 1 && v <= 65536) g.list_cap = v; }
        const size_t b_seg = sizeof(float) * 4 * M * (size_t)N, b_reach = sizeof(float) * M * (size_t)N, b_cells = 32 * (size_t)H, b_glob = 128,
                     b_ovf = sizeof(unsigned short) * (size_t)g.ovf_cap, b_list = sizeof(unsigned short) * (size_t)g.list_cap * N, b_cnt = sizeof(int) * (size_t)N,
                     b_plist = sizeof(unsigned short) * (size_t)g.plist_cap * N, b_view = sizeof(NeighView),
                     b_blk = (N - 1) * M > 0xffff ? sizeof(unsigned long long) * (size_t)N : 0;      // (the starts of the wide lists' high parts)
        auto al16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        const size_t total = al16(b_seg) + al16(b_reach) + al16(b_cells) + al16(b_glob) + al16(b_ovf) + al16(b_list) + 2 * al16(b_cnt) + al16(b_plist) + al16(b_blk) + al16(b_view);
        HIPCHK(c, s.d_neigh.alloc_zero(total));         // tag 0 everywhere: the first tick's tag is 1
        unsigned char *p = s.d_neigh;
        g.seg_bound = reinterpret_cast<float *>(p); p += al16(b_seg);
        g.reach = reinterpret_cast<float *>(p); p += al16(b_reach);
        g.cells = reinterpret_cast<unsigned long long *>(p); p += al16(b_cells);
        g.glob = reinterpret_cast<unsigned long long *>(p); p += al16(b_glob);
        g.ovf = reinterpret_cast<unsigned short *>(p); p += al16(b_ovf);
        g.list = reinterpret_cast<unsigned short *>(p); p += al16(b_list);
        g.cnt = reinterpret_cast<int *>(p); p += al16(b_cnt);
        g.pcnt = reinterpret_cast<int *>(p); p += al16(b_cnt);
        g.plist = reinterpret_cast<unsigned short *>(p); p += al16(b_plist);
        g.blk = b_blk ? reinterpret_cast<unsigned long long *>(p) : nullptr; p += al16(b_blk);
        NeighView v;
        v.list = g.list; v.cnt = g.cnt; v.plist = g.plist; v.pcnt = g.pcnt; v.cap = g.list_cap; v.pcap = g.plist_cap; v.blk = g.blk;
        HIPCHK(c, hipMemcpy(p, &v, sizeof(v), hipMemcpyHostToDevice));
        g.view = reinterpret_cast<const NeighView *>(p);
        g.prof = nullptr;
        if (getenv("LSC_NEIGH_PROFILE")) {        // stage stamps of the query kernel, printed by lsc_destroy (diagnostics)
            HIPCHK(c, s.d_neigh_prof.alloc_zero(8 * n));
            g.prof = s.d_neigh_prof;
        }
    }
    HIPCHK(c, s.d_iters_acc.alloc_zero(6 * n));       // [N] iterations, [N] iterations x LSC rows, [N][4] counters of the active-set solve (per agent: no workgroup shares an address)
    HIPCHK(c, s.d_prof.alloc_zero(2 * PROF_PHASES * n));          // [N] plan kernel, [N] general kernel
    HIPCHK(c, s.d_dbg.alloc_zero(4 * n));
    HIPCHK(c, s.d_in.alloc(in_block_floats(n)));
    s.d_state = s.d_in; s.d_goal = s.d_state + 9 * n; s.d_prev = s.d_state + 12 * n;
    // outputs: padded to table_rows so that the multi-GPU form gathers them in place
    HIPCHK(c, s.d_out.alloc_zero(out_block_bytes(Np)));
    unsigned char *out = s.d_out;
    s.d_cost = reinterpret_cast<double *>(out);
    s.d_next = reinterpret_cast<float *>(out + sizeof(double) * Np);
    s.d_status = reinterpret_cast<int *>(out + (sizeof(double) + sizeof(float) * NV) * Np);
    s.d_iters = s.d_status + Np;
    HIPCHK(c, s.h_in.alloc(in_block_floats(n)));
    HIPCHK(c, s.h_out.alloc(out_block_bytes(Np)));
    return build_integrals(c);
}

int lsc_set_shard(lsc_ctx *c, int first, int count)
{
    if (!c || c->N == 0) return LSC_ESTATE;
    if (first < 0 || count < 0 || first + count > c->N) return LSC_EINVAL;   // count 0: a rank without agents
    c->first = first; c->count = count;
    return LSC_OK;
}

// ---------------------------------------------------------------------------------------------------
// Dynamic obstacles (ObstacleType::DYNAMICOBSTACLE through TrajPlanner::setObstacles): non-cooperating moving spheres that follow the
// other agents in every agent's obstacle list.  Only the LSC build of the plan kernel sees them (lsc_kernels.hip: OBS).
// ---------------------------------------------------------------------------------------------------
// what a context must be to plan against dynamic obstacles: it plans the whole swarm alone, at most one agent per CU (the latency
// kernels), LSC mode without a slack mode, in a 3-D world -- and without disturbance checks unless the obstacles come with what those need
// reset_served: the obstacles came (or come) through lsc_set_obstacles_ex, which serves reset_threshold > 0
static int obstacles_context_ok(lsc_ctx *c, const char *fn, bool reset_served)
{
    const char *why = nullptr;
    if (c->world != 1) why = "the context is a rank of a sharded swarm (communicator of more than one rank)";
    else if (c->first != 0 || c->count != c->N) why = "the context's shard is not the whole swarm";
    else if (c->count > c->n_cu) why = "the swarm has more agents than the GPU has CUs (the throughput build is not built for them)";
    else if (c->cfg.slack_mode != 0) why = "a slack mode is configured";
    else if (c->cfg.planner_mode == 1) why = "planner_mode bvc";
    else if (c->cfg.reset_threshold > 0.0 && !reset_served) why = "reset_threshold > 0 (the disturbance checks); lsc_set_obstacles_ex serves them";
    else if (c->cfg.world_dimension == 2) why = "world_dimension 2 (planar world)";
    else if (c->profiling) why = "lsc_phase_profile is on (no instrumented kernel is built for them)";
    if (!why) return LSC_OK;
    c->err = std::string(fn) + ": dynamic obstacles are not built for this context: " + why;
    return LSC_EINVAL;
}

// in front of the next n_ticks ticks of a context with motion models: the clock is set, and no tick's time sends a patrol's walk (the one
// loop of the stage whose trip count depends on data) over more than OBSTACLE_WALK_MAX legs
static int obstacle_clock_ok(lsc_ctx *c, const char *fn, int n_ticks)
{
    const ObsMem &ob = c->swarm.obs;
    if (!ob.have_clock) { c->err = std::string(fn) + ": the context has motion models and no clock (lsc_obstacle_clock)"; return LSC_ESTATE; }
    double now = ob.clock_now, t_last = ob.chaser_t_last;
    for (int j = 0; j < n_ticks; j++, now += ob.clock_step) {
        const double t = now - ob.clock_start;
        // a chaser integrates over t - t_last: a time below its last evaluated one is refused; a walker reads floor((t + 1e-5) / cycle) + 1
        // entries of its history
        for (int o = 0; o < ob.K && (ob.n_chasers > 0 || ob.n_walkers > 0); o++) {
            if (ob.h_models[o].kind == OBSTACLE_CHASING && t < t_last) {
                c->err = std::string(fn) + ": at time " + std::to_string(t) + " the chaser obstacle " + std::to_string(o) + " would step backwards (its last evaluated time is " + std::to_string(t_last) + ")";
                return LSC_EINVAL;
            }
            if (ob.h_models[o].kind == OBSTACLE_GAUSSIAN && !(obstacle_walker_entries(ob.h_walkers[o], t) <= (double)ob.h_walkers[o].n_acc)) {
                c->err = std::string(fn) + ": at time " + std::to_string(t) + " the gaussian obstacle " + std::to_string(o) + " needs more than the " + std::to_string(ob.h_walkers[o].n_acc) + " entries of its acceleration history";
                return LSC_EINVAL;
            }
        }
        t_last = t;
        for (int o = 0; o < ob.K; o++)
            if (!obstacle_walk_ok(ob.h_models[o], t)) {
                c->err = std::string(fn) + ": at time " + std::to_string(t) + " the patrol walk of obstacle " + std::to_string(o) + " would step over more than 65536 legs (time / shortest leg time)";
                return LSC_EINVAL;
            }
    }
    return LSC_OK;
}

// in front of a tick: LSC_OK for a context without obstacles; with them, what lsc_set_obstacles checked (the shard may have changed
// since) and that their states were set
static int obstacles_tick_ok(lsc_ctx *c, const char *fn)
{
    const ObsMem &ob = c->swarm.obs;
    if (ob.K == 0) return LSC_OK;
    if (int rc = obstacles_context_ok(c, fn, ob.reset_served)) return rc;
    if (ob.d_models) return obstacle_clock_ok(c, fn, 1);     // (installed models count as "has states")
    if (!ob.have_states) { c->err = std::string(fn) + ": the context has dynamic obstacles and no states (lsc_obstacle_states / lsc_obstacle_states_device)"; return LSC_ESTATE; }
    return LSC_OK;
}

// the pinned images are free to be written: an upload queued by a device-resident tick may still read them
static int obstacle_uploads_done(lsc_ctx *c)
{
    ObsMem &ob = c->swarm.obs;
    if (ob.upload_in_flight) HIPCHK(c, hipStreamSynchronize(ob.upload_stream));
    ob.upload_in_flight = false;
    return LSC_OK;
}

// block and states, as far as they changed since the last tick, on the tick's stream in front of its launches
static int upload_obstacles(lsc_ctx *c, hipStream_t st)
{
    ObsMem &ob = c->swarm.obs;
    if (ob.K == 0 || (!ob.block_dirty && !ob.states_pending)) return LSC_OK;
    if (ob.upload_in_flight && ob.upload_stream != st) { if (int rc = obstacle_uploads_done(c)) return rc; }
    if (ob.block_dirty) HIPCHK(c, hipMemcpyAsync(ob.d_block.get(), ob.h_block.get(), sizeof(ObsBlock), hipMemcpyHostToDevice, st));
    if (ob.states_pending) HIPCHK(c, hipMemcpyAsync(ob.d_pos_vel.get(), ob.h_pos_vel.get(), sizeof(float) * 6 * (size_t)ob.K, hipMemcpyHostToDevice, st));
    ob.block_dirty = ob.states_pending = false;
    // The pinned images must not be rewritten while a copy reads them.  On the context's own stream the host-buffer tick synchronises
    // anyway; on a caller's stream (device-resident ticks fed host states) the wait is made HERE, while the handle is certainly alive --
    // no stream of the caller's is remembered
    if (st == c->stream) { ob.upload_stream = st; ob.upload_in_flight = true; }
    else HIPCHK(c, hipStreamSynchronize(st));
    return LSC_OK;
}

// lsc_set_obstacles (max_acc null) and lsc_set_obstacles_ex: the second is the first plus what the disturbance reset needs
static int set_obstacles(lsc_ctx *c, const char *fn, int K, const double *radius, const double *downwash, const double *max_acc,
                         int size_prediction, double uncertainty_horizon)
{
    if (!c) return LSC_EINVAL;
    const std::string f = fn;
    const bool ex = max_acc != nullptr;
    if (c->N == 0) { c->err = f + ": lsc_set_agents comes first"; return LSC_ESTATE; }
    if (K < 0 || K > LSC_OBSTACLES_MAX) { c->err = f + ": K = " + std::to_string(K) + " outside 0.." + std::to_string(LSC_OBSTACLES_MAX); return LSC_EINVAL; }
    if (K > 0 && (!radius || !downwash)) { c->err = f + ": null radius / downwash"; return LSC_EINVAL; }
    for (int o = 0; o < K; o++) {
        if (!(radius[o] > 0.0) || !std::isfinite(radius[o])) { c->err = f + ": radius of obstacle " + std::to_string(o) + " is not a positive finite number"; return LSC_EINVAL; }
        if (!(downwash[o] >= 0.0) || !std::isfinite(downwash[o])) { c->err = f + ": downwash of obstacle " + std::to_string(o) + " is negative or not finite"; return LSC_EINVAL; }
        if (ex && (!(max_acc[o] >= 0.0) || !std::isfinite(max_acc[o]))) { c->err = f + ": max_acc of obstacle " + std::to_string(o) + " is negative or not finite"; return LSC_EINVAL; }
    }
    int M_u = 0;
    if (ex && K > 0) {
        if (!(uncertainty_horizon >= 0.0) || !std::isfinite(uncertainty_horizon)) { c->err = f + ": uncertainty_horizon is negative or not finite (obstacle 0 and every other)"; return LSC_EINVAL; }
        // (compared as doubles: a horizon whose quotient does not fit an int must not reach the conversion)
        if ((uncertainty_horizon + 1e-9) / c->cfg.dt >= (double)(M + 1)) {
            c->err = f + ": uncertainty_horizon " + std::to_string(uncertainty_horizon) + " gives more than the M = " + std::to_string(M) + " segments of the horizon (obstacle 0 and every other: the reference writes past its size table)";
            return LSC_EINVAL;
        }
        M_u = rule_uncertainty_segments(uncertainty_horizon, c->cfg.dt);
    }
    if (K > 0) { if (int rc = obstacles_context_ok(c, fn, ex)) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());               // (ticks in flight read the buffers that go)
    c->swarm.obs = ObsMem{};
    c->cap = c->cap_agents;
    note_obstacles(c, 0);
    if (K == 0) return LSC_OK;
    static_assert(LSC_OBSTACLES_MAX == OBSTACLES_MAX, "the header's bound is the block's");
    ObsMem &ob = c->swarm.obs;
    const int N = c->N, n_obs = N - 1 + K;
    constexpr int NBR = NCP - 3;
    ob.cap = lds_row_capacity(c, n_obs);
    HIPCHK(c, ob.d_block.alloc(1));
    HIPCHK(c, ob.d_pos_vel.alloc_zero(6 * (size_t)K));
    HIPCHK(c, ob.h_block.alloc(1));
    HIPCHK(c, ob.h_pos_vel.alloc(6 * (size_t)K));
    ObsBlock &b = *ob.h_block.get();
    std::memset(&b, 0, sizeof(b));
    b.K = K; b.pos_vel = ob.d_pos_vel;
    for (int o = 0; o < K; o++) {
        // as dynamic_msgs::Obstacle holds them (float32); a downwash of 0 is "not given" = 1 (mission.cpp:164-166)
        b.radius[o] = (double)(float)radius[o];
        b.downwash[o] = downwash[o] == 0.0 ? 1.0 : (double)(float)downwash[o];
    }
    if (ob.cap < NBR * n_obs) {
        ob.spill_stride = plan_spill_bytes(n_obs);
        ob.spill_slots = std::min(N, 256);
        HIPCHK(c, ob.d_spill.alloc(ob.spill_stride * (size_t)ob.spill_slots));
    }
    if (ex) {
        // the predicted sizes, once, in doubles (rule_obstacle_size on the float32 radius the rows use); the alternate-mode workspaces of a
        // context that can hand agents over (lsc_set_agents allocated its own by N - 1) by N - 1 + K
        std::vector<double> size((size_t)K * M * NC);
        for (int o = 0; o < K; o++)
            for (int m = 0; m < M; m++)
                for (int i = 0; i < NC; i++)
                    size[((size_t)o * M + m) * NC + i] = rule_obstacle_size(b.radius[o], max_acc[o], c->cfg.dt, M_u, size_prediction != 0, m, i);
        HIPCHK(c, ob.d_size.upload(size.data(), size.size()));
        b.size = ob.d_size;
        if (c->swarm.d_gen_ws) {
            ob.gen_stride = general_ws_bytes(N + K);
            HIPCHK(c, ob.d_gen_ws.alloc(ob.gen_stride * (size_t)c->swarm.gen_slots));
        }
        ob.reset_served = true;
    }
    ob.block_dirty = true;
    ob.K = K;
    c->cap = ob.cap;
    note_obstacles(c, K);
    return LSC_OK;
}

int lsc_set_obstacles(lsc_ctx *c, int K, const double *radius, const double *downwash)
{
    return set_obstacles(c, "lsc_set_obstacles", K, radius, downwash, nullptr, 0, 0.0);
}

int lsc_set_obstacles_ex(lsc_ctx *c, int K, const double *radius, const double *downwash, const double *max_acc, int size_prediction,
                         double uncertainty_horizon)
{
    if (c && K > 0 && !max_acc) { c->err = "lsc_set_obstacles_ex: null max_acc"; return LSC_EINVAL; }
    static const double none = 0.0;
    return set_obstacles(c, "lsc_set_obstacles_ex", K, radius, downwash, max_acc ? max_acc : &none, size_prediction, uncertainty_horizon);
}

int lsc_obstacle_states(lsc_ctx *c, const float *pos_vel)
{
    if (!c || !pos_vel) return LSC_EINVAL;
    ObsMem &ob = c->swarm.obs;
    if (ob.K == 0) { c->err = "lsc_obstacle_states: the context has no dynamic obstacles (lsc_set_obstacles)"; return LSC_ESTATE; }
    if (ob.d_models) { c->err = "lsc_obstacle_states: the context moves its obstacles itself (motion models are installed: lsc_obstacle_motion with K = 0 removes them)"; return LSC_ESTATE; }
    for (int i = 0; i < 6 * ob.K; i++)
        if (!std::isfinite(pos_vel[i])) { c->err = "lsc_obstacle_states: state of obstacle " + std::to_string(i / 6) + " is not finite"; return LSC_EINVAL; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = obstacle_uploads_done(c)) return rc;
    std::memcpy(ob.h_pos_vel.get(), pos_vel, sizeof(float) * 6 * (size_t)ob.K);
    if (ob.h_block.get()->pos_vel != ob.d_pos_vel.get()) { ob.h_block.get()->pos_vel = ob.d_pos_vel; ob.block_dirty = true; }
    ob.states_pending = true; ob.have_states = true;
    return LSC_OK;
}

int lsc_obstacle_states_device(lsc_ctx *c, const float *d_pos_vel)
{
    if (!c || !d_pos_vel) return LSC_EINVAL;
    ObsMem &ob = c->swarm.obs;
    if (ob.K == 0) { c->err = "lsc_obstacle_states_device: the context has no dynamic obstacles (lsc_set_obstacles)"; return LSC_ESTATE; }
    if (ob.d_models) { c->err = "lsc_obstacle_states_device: the context moves its obstacles itself (motion models are installed: lsc_obstacle_motion with K = 0 removes them)"; return LSC_ESTATE; }
    if (ob.h_block.get()->pos_vel != d_pos_vel) {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        if (int rc = obstacle_uploads_done(c)) return rc;
        ob.h_block.get()->pos_vel = d_pos_vel; ob.block_dirty = true;
    }
    ob.states_pending = false; ob.have_states = true;
    return LSC_OK;
}

// lsc_obstacle_motion (ex false: kinds 0 to 2 alone) and lsc_obstacle_motion_ex
static int obstacle_motion_install(lsc_ctx *c, const char *fn, bool ex, int K, const lsc_obstacle_model *models, int n_chasers, const lsc_obstacle_chaser *chasers,
                                   int n_walkers, const lsc_obstacle_walker *walkers)
{
    static_assert(LSC_OBSTACLE_CHASING == OBSTACLE_CHASING && LSC_OBSTACLE_GAUSSIAN == OBSTACLE_GAUSSIAN && sizeof(ObstacleChaserState) == 7 * sizeof(double),
                  "the header's constants are the table's");
    static_assert(LSC_OBSTACLE_POINTS_MAX == OBSTACLE_POINTS_MAX && LSC_OBSTACLE_STRAIGHT == OBSTACLE_STRAIGHT && LSC_OBSTACLE_SPIN == OBSTACLE_SPIN &&
                  LSC_OBSTACLE_PATROL == OBSTACLE_PATROL, "the header's constants are the table's");
    if (!c) return LSC_EINVAL;
    ObsMem &ob = c->swarm.obs;
    const std::string f(fn);
    if (ob.K == 0) { c->err = f + ": the context has no dynamic obstacles (lsc_set_obstacles comes first)"; return LSC_ESTATE; }
    const bool remove = K == 0 || !models;
    if (!remove && K != ob.K) { c->err = f + ": " + std::to_string(K) + " models for the " + std::to_string(ob.K) + " obstacles of lsc_set_obstacles"; return LSC_EINVAL; }
    if (!remove && (n_chasers < 0 || n_walkers < 0 || (n_chasers > 0 && !chasers) || (n_walkers > 0 && !walkers))) { c->err = f + ": a negative count, or records that are null"; return LSC_EINVAL; }
    std::vector<ObstacleEntry> table(remove ? 0 : (size_t)K);
    std::vector<ObstacleChaser> ch(table.size());
    std::vector<ObstacleWalker> wk(table.size());
    std::vector<ObstacleChaserState> st(table.size());
    std::vector<double> acc;
    int have_chasers = 0, have_walkers = 0;
    for (size_t o = 0; o < table.size(); o++) {
        const int kind = models[o].kind;
        if (kind == OBSTACLE_CHASING || kind == OBSTACLE_GAUSSIAN) {
            if (!ex) {
                c->err = f + ": obstacle " + std::to_string(o) + ": kind " + std::to_string(kind) + " (chasing 3, gaussian 4) is installed through lsc_obstacle_motion_ex";
                return LSC_EINVAL;
            }
            table[o] = ObstacleEntry{};
            table[o].kind = kind;
            continue;
        }
        if (const int why = obstacle_entry_build(kind, models[o].n_points, models[o].speed, models[o].points, table[o])) {
            c->err = f + ": obstacle " + std::to_string(o) + ": " + obstacle_refusal(why);
            return LSC_EINVAL;
        }
    }
    const double nan = std::nan("");
    for (auto &s0 : st) s0 = ObstacleChaserState{{nan, nan, nan}, {nan, nan, nan}, nan};       // (rows of obstacles that are no chasers: lsc_obstacle_chaser_states_read)
    std::vector<int> named(table.size(), 0);
    for (int i = 0; !remove && i < n_chasers + n_walkers; i++) {
        const bool is_chaser = i < n_chasers;
        const int o = is_chaser ? chasers[i].obstacle : walkers[i - n_chasers].obstacle;
        const char *what = is_chaser ? "chaser" : "walker";
        if (o < 0 || o >= K) { c->err = f + ": " + what + " record " + std::to_string(is_chaser ? i : i - n_chasers) + " names obstacle " + std::to_string(o) + " outside 0.." + std::to_string(K - 1); return LSC_EINVAL; }
        if (table[o].kind != (is_chaser ? OBSTACLE_CHASING : OBSTACLE_GAUSSIAN)) {
            c->err = f + ": a " + what + " record names obstacle " + std::to_string(o) + ", whose model is of kind " + std::to_string(table[o].kind);
            return LSC_EINVAL;
        }
        if (named[o]++) { c->err = f + ": obstacle " + std::to_string(o) + " is named by more than one " + what + " record"; return LSC_EINVAL; }
        int why;
        if (is_chaser) {
            const lsc_obstacle_chaser &r = chasers[i];
            why = obstacle_chaser_build(r.target, c->N, r.start, r.radius, r.max_vel, r.max_acc, r.gamma_target, r.gamma_obs, ch[o]);
            st[o] = ObstacleChaserState{{r.start[0], r.start[1], r.start[2]}, {0.0, 0.0, 0.0}, 0.0};
            have_chasers++;
        } else {
            const lsc_obstacle_walker &r = walkers[i - n_chasers];
            why = obstacle_walker_build(r.start, r.initial_vel, r.max_vel, r.acc_update_cycle, r.n_acc, r.acc, (int)(acc.size() / 3), wk[o]);
            if (!why) acc.insert(acc.end(), r.acc, r.acc + 3 * (size_t)r.n_acc);
            have_walkers++;
        }
        if (why) { c->err = f + ": obstacle " + std::to_string(o) + " (" + what + "): " + obstacle_refusal_ex(why); return LSC_EINVAL; }
    }
    for (size_t o = 0; o < table.size(); o++)
        if ((table[o].kind == OBSTACLE_CHASING || table[o].kind == OBSTACLE_GAUSSIAN) && !named[o]) {
            c->err = f + ": obstacle " + std::to_string(o) + " is of kind " + std::to_string(table[o].kind) + " and no " + (table[o].kind == OBSTACLE_CHASING ? "chaser" : "walker") + " record names it";
            return LSC_EINVAL;
        }
    if (remove && !ob.d_models) return LSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());               // (ticks in flight read the table and the states that change hands)
    ob.upload_in_flight = false;
    ob.d_models.reset();
    ob.d_pos_f64.reset();
    ob.h_models.clear();
    ob.have_clock = false;
    ob.d_chasers.reset(); ob.d_walkers.reset(); ob.d_acc.reset(); ob.d_chaser_state.reset();
    ob.h_chasers.clear(); ob.h_walkers.clear();
    ob.n_chasers = ob.n_walkers = 0;
    ob.no_step_yet = true;
    ob.chaser_t_last = 0.0;
    // the states are the context's own buffer from here on, and nobody has fed them: with models the stage writes them in front of
    // every tick, without them the context is one that was only given lsc_set_obstacles
    ob.states_pending = ob.have_states = false;
    if (ob.h_block.get()->pos_vel != ob.d_pos_vel.get()) { ob.h_block.get()->pos_vel = ob.d_pos_vel; ob.block_dirty = true; }
    if (remove) return LSC_OK;
    HIPCHK(c, ob.d_pos_f64.alloc_zero(3 * table.size()));
    HIPCHK(c, ob.d_models.upload(table.data(), table.size()));
    ob.h_models = std::move(table);
    if (have_chasers + have_walkers > 0) {
        HIPCHK(c, ob.d_chasers.upload(ch.data(), ch.size()));
        HIPCHK(c, ob.d_walkers.upload(wk.data(), wk.size()));
        if (!acc.empty()) HIPCHK(c, ob.d_acc.upload(acc.data(), acc.size()));
        HIPCHK(c, ob.d_chaser_state.upload(reinterpret_cast<const double *>(st.data()), 7 * st.size()));
        ob.h_chasers = std::move(ch); ob.h_walkers = std::move(wk);
        ob.n_chasers = have_chasers; ob.n_walkers = have_walkers;
    }
    return LSC_OK;
}

int lsc_obstacle_motion(lsc_ctx *c, int K, const lsc_obstacle_model *models)
{
    return obstacle_motion_install(c, "lsc_obstacle_motion", false, K, models, 0, nullptr, 0, nullptr);
}

int lsc_obstacle_motion_ex(lsc_ctx *c, int K, const lsc_obstacle_model *models, int n_chasers, const lsc_obstacle_chaser *chasers, int n_walkers,
                           const lsc_obstacle_walker *walkers)
{
    return obstacle_motion_install(c, "lsc_obstacle_motion_ex", true, K, models, n_chasers, chasers, n_walkers, walkers);
}

int lsc_obstacle_chaser_states_read(lsc_ctx *c, double *state)
{
    if (!c || !state) return LSC_EINVAL;
    const ObsMem &ob = c->swarm.obs;
    if (ob.n_chasers == 0) { c->err = "lsc_obstacle_chaser_states_read: the context has no chasing obstacles (lsc_obstacle_motion_ex)"; return LSC_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(state, ob.d_chaser_state.get(), sizeof(double) * 7 * (size_t)ob.K, hipMemcpyDeviceToHost));
    return LSC_OK;
}

int lsc_obstacle_clock(lsc_ctx *c, double start, double now, double step)
{
    if (!c) return LSC_EINVAL;
    if (!std::isfinite(start) || !std::isfinite(now) || !std::isfinite(step)) { c->err = "lsc_obstacle_clock: a value that is not finite"; return LSC_EINVAL; }
    ObsMem &ob = c->swarm.obs;
    if (!ob.d_models) { c->err = "lsc_obstacle_clock: the context has no motion models (lsc_obstacle_motion)"; return LSC_ESTATE; }
    ob.clock_start = start; ob.clock_now = now; ob.clock_step = step; ob.have_clock = true;
    return LSC_OK;
}

int lsc_obstacle_clock_read(lsc_ctx *c, double *now)
{
    if (!c || !now) return LSC_EINVAL;
    const ObsMem &ob = c->swarm.obs;
    if (!ob.have_clock) { c->err = "lsc_obstacle_clock_read: no clock is set (lsc_obstacle_clock)"; return LSC_ESTATE; }
    *now = ob.clock_now;
    return LSC_OK;
}

int lsc_obstacle_states_read(lsc_ctx *c, float *pos_vel)
{
    if (!c || !pos_vel) return LSC_EINVAL;
    const ObsMem &ob = c->swarm.obs;
    if (ob.K == 0) { c->err = "lsc_obstacle_states_read: the context has no dynamic obstacles (lsc_set_obstacles)"; return LSC_ESTATE; }
    if (!ob.d_models && !ob.have_states) { c->err = "lsc_obstacle_states_read: the obstacles have no states yet"; return LSC_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(pos_vel, ob.h_block.get()->pos_vel, sizeof(float) * 6 * (size_t)ob.K, hipMemcpyDeviceToHost));
    return LSC_OK;
}

// Key32 table of the goal search: word d = floor(sqrt d) << rb | rank of frac(sqrt d) among the distinct fractional parts of
// sqrt(0 .. words - 1).  Returns false (table empty) when the ranks need more than 16 bits or the smallest gap between two distinct
// fractional parts -- the wrap-around gap 1 - max included -- is not orders of magnitude above the rounding of the reference's F.
// (The argument why such keys order and tie exactly like the reference's doubles is spelled out in build_goal_grid.)
static bool goal_key_table(int words, std::vector<uint32_t> &table, int &rank_bits)
{
    table.clear();
    rank_bits = 0;
    if (words < 1 || words > (1 << 16)) return false;
    std::vector<std::pair<long double, int>> fr(words);
    std::vector<uint32_t> q(words);
    for (int d = 0; d < words; d++) {
        uint32_t r = (uint32_t)std::sqrt((double)d);
        while ((long long)r * r > d) r--;
        while ((long long)(r + 1) * (r + 1) <= d) r++;
        q[d] = r;
        fr[d] = {(long long)r * r == d ? 0.0L : sqrtl((long double)d) - (long double)r, d};     // exact 0 for perfect squares
    }
    std::sort(fr.begin(), fr.end());
    std::vector<uint32_t> rank(words);
    long double min_gap = 1.0L - fr.back().first;
    uint32_t rk = 0;
    for (int i = 0; i < words; i++) {
        if (i > 0 && fr[i].first != fr[i - 1].first) { rk++; min_gap = std::min(min_gap, fr[i].first - fr[i - 1].first); }
        rank[fr[i].second] = rk;
    }
    int rb = 1;
    while ((1u << rb) <= rk) rb++;
    // gaps are ~1 / D^2 (>= 1e-10 for D < 65536); long double resolves 1e-16 here; the reference's F carries < 1e-9 of rounding
    // at most (ulp(2^19) = 6e-11, three roundings) against 10 x gap
    const bool safe = min_gap > 1e-12L && 10.0L * min_gap > 50.0L * 6e-11L && rb <= 16;
    // (with rb <= 16 and steps <= G_MAX = 32767, (steps + q) << rb stays below 2^32 - 1 = NONE)
    if (!safe) return false;
    table.resize(words);
    for (int d = 0; d < words; d++) table[d] = (q[d] << rb) | rank[d];
    rank_bits = rb;
    return true;
}

// test hook (host only, no device needed): the key table for squared distances 0 .. words - 1
int lsc_goal_key_table(int words, unsigned int *out, int *rank_bits)
{
    if (!out || !rank_bits) return LSC_EINVAL;
    std::vector<uint32_t> t;
    int rb = 0;
    if (!goal_key_table(words, t, rb)) return LSC_ESTATE;
    std::memcpy(out, t.data(), sizeof(uint32_t) * t.size());
    *rank_bits = rb;
    return LSC_OK;
}

// the HBM search's workspace for the context's agents (c->count of them; again when a shard grows)
static int alloc_goal_ws(lsc_ctx *c)
{
    if (!c->goal_ws_bytes || c->swarm.map.goal_ws_agents >= c->count) return LSC_OK;
    c->swarm.map.goal_ws_agents = 0;
    const size_t bytes = c->goal_ws_bytes * (size_t)c->count;
    if (c->swarm.map.d_goal_ws.alloc(bytes) != hipSuccess) {
        (void)hipGetLastError();
        c->err = "goal planner: cannot allocate " + std::to_string(bytes >> 20) + " MiB of HBM workspace for the search (" +
                 std::to_string(c->goal_ws_bytes) + " bytes per agent)";
        return LSC_ENOMEM;
    }
    c->swarm.map.goal_ws_agents = c->count;
    return LSC_OK;
}

// Goal planner inputs derived from the map (GridBasedPlanner::updateGridInfo / updateGridMap, distmap part,
// src/grid_based_planner.cpp:72-130): grid geometry, one static occupancy grid per distinct radius (indexed by the
// search key H*W*z + W*i + j), the distance field itself for castRay, and the bucket-count sequence of the
// std::unordered_map this build's libstdc++ provides (the reference's OPEN rows are such maps; see lsc_goal.hip).
static int build_goal_grid(lsc_ctx *c, const std::vector<double> &radii)
{
    if (c->cfg.goal_mode != 1 || !c->cfg.use_octomap) return LSC_OK;
    const double res = c->cfg.grid_resolution;
    if (!(res > 0)) { c->err = "grid_resolution must be positive"; return LSC_EINVAL; }
    int dim[3];
    for (int a = 0; a < 3; a++) {
        c->grid_min[a] = -std::floor((-(double)c->cfg.world_min[a] + 1e-9) / res) * res;
        const double gmax = std::floor(((double)c->cfg.world_max[a] + 1e-9) / res) * res;
        if (a == 2 && c->cfg.world_dimension == 2) {          // planar world: one layer at z = world/z_2d (:82-85)
            c->grid_min[a] = c->cfg.world_z_2d;
            dim[a] = 1;
        } else {
            dim[a] = (int)std::round((gmax - c->grid_min[a]) / res) + 1;
        }
        c->grid_dims[a] = dim[a];
    }
    const int H = dim[0], W = dim[1], A = dim[2];
    const size_t C = (size_t)H * W * A;
    const long long WA = (long long)W * A;
    // OPEN row capacity: what fits the 160 KiB of LDS next to the per-cell state
    int cap = (int)std::min<long long>(WA, 1 << 30);
    bool lds_fits = C <= 131071;
    if (lds_fits) {
        while (cap > 16 && goal_smem_bytes(H, W, A, cap) > 158 * 1024) cap--;
        lds_fits = goal_smem_bytes(H, W, A, cap) <= 158 * 1024;
    }
    // The HBM search (lsc_goal.hip): grids whose search state does not fit LDS (more than 131071 cells -- the 17 bits of a cell key -- or
    // cells plus 16-entry rows beyond LDS), and goal_search = 3.  Rows at full capacity W A in a per-agent HBM workspace; an entry
    // holds the row-local key W z + j.  Its own limits are checked here: a refused grid is an error at load, never a different goal.
    c->goal_hbm = 0;
    c->goal_ws_bytes = 0;
    auto hbm_rows_ok = [&](std::string &why) {
        if (WA > 65535) { why = "a grid row (W * A cells) has more than 65535 cells (an OPEN entry keeps its row position in 16 bits)"; return false; }
        if (H > 65535) { why = "the grid has more than 65535 rows (findMin keeps the row index in 16 bits)"; return false; }
        return true;
    };
    if (!lds_fits || c->cfg.goal_search == 3) {
        std::string why;
        if (!hbm_rows_ok(why)) { c->err = "goal planner: search grid too large for the HBM search: " + why; return LSC_EINVAL; }
        if (goal_hbm_smem_bytes(H, W, A, false) > 158 * 1024) { c->err = "goal planner: the row bookkeeping of the HBM search does not fit LDS"; return LSC_EINVAL; }
        c->goal_hbm = goal_hbm_smem_bytes(H, W, A, true) <= 150 * 1024 ? 1 : 2;     // cell bytes in LDS while they fit
        cap = (int)WA;
        c->goal_ws_bytes = goal_hbm_ws_bytes(H, W, A, c->goal_hbm == 2);
    }
    // ---- Key32: the search key as one 32-bit word (lsc_goal.hip).  The A* key is F = 10 (g + sqrt(d2)), g = steps, d2 = squared cell
    // distance to the goal: integers.  The search only ever ORDERS keys and tests them for EQUALITY, so any map of (g, d2) that
    // preserves both is as good as the double the reference computes.  Write sqrt(d2) = q + f, q = floor.  Then
    //     key = ((g + q) << rb) | rank(f),      rank = position of f among the distinct fractional parts of sqrt(0 .. D)
    // orders like g + sqrt(d2): integer parts first (f < 1), fractional parts by rank; and key equality <=> (g + q, f) equal <=>
    // the reals are equal.  The reference's doubles order the same way: equal reals mean equal d2 (same double) or two perfect
    // squares (every operation exact), and distinct reals differ by at least the smallest gap between distinct fractional parts,
    // which is CHECKED below to exceed the rounding error of the reference's three roundings (a few ulp of F < 2^19) by orders
    // of magnitude.  If the check fails, or the table does not fit next to a useful row capacity, Key64 (the double itself) is used.
    c->h_fcode.clear();
    c->fcode_rb = 0;
    {
        const long long D = (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1) + (long long)(A - 1) * (A - 1);
        int cap32 = W * A;
        const int words = D < (1 << 16) ? (int)D + 1 : 0;
        if (words > 0) {
            while (cap32 > 16 && goal_smem_bytes(H, W, A, cap32, words) > 158 * 1024) cap32--;
            if (goal_smem_bytes(H, W, A, cap32, words) > 158 * 1024 || cap32 < std::min(W * A, 192)) cap32 = 0;
        }
        int jb_unused = 0;
        const bool fast = c->cfg.goal_search != 1 && goal_fast_slots(H, W, A, &jb_unused) != 0;     // else the table would be dead weight in LDS
        if (words > 0 && cap32 > 0 && c->cfg.goal_search != 2 && fast && !c->goal_hbm) {
            int rb = 0;
            if (goal_key_table(words, c->h_fcode, rb)) { c->fcode_rb = rb; cap = cap32; }
        }
    }
    if (!c->goal_hbm) {
        if (c->cfg.goal_row_cap > 0) cap = std::max(4, std::min(cap, c->cfg.goal_row_cap));   // explicit smaller capacity (tests force the overflow path)
        else if (c->cfg.goal_lds_row_cap > 0) cap = std::max(4, std::min(cap, c->cfg.goal_lds_row_cap));   // smaller LDS capacity, restart in HBM
        // a row that can outgrow its LDS capacity restarts the search in HBM -- unless goal_row_cap asks for the hard capacity (status 5)
        std::string why;
        if (cap < WA && c->cfg.goal_row_cap <= 0 && hbm_rows_ok(why)) c->goal_ws_bytes = goal_hbm_ws_bytes(H, W, A, false);
    }
    c->grid_row_cap = cap;
    // bucket counts of a growing std::unordered_map<uint_least32_t, T> (identity hash), from the container itself; as far as the
    // longest row can grow (W A entries where the HBM search or the restart can run)
    {
        const long long rows_max = c->goal_ws_bytes ? WA : cap;
        std::unordered_map<uint_least32_t, int> probe;
        c->nb_seq.clear();
        size_t last = probe.bucket_count();
        for (uint_least32_t k = 0; k < (uint_least32_t)rows_max + 1 && c->nb_seq.size() < 16; k++) {
            probe[k] = 0;
            if (probe.bucket_count() != last) { last = probe.bucket_count(); c->nb_seq.push_back((int)last); }
        }
        if (c->goal_ws_bytes && (c->nb_seq.empty() || c->nb_seq.back() < rows_max)) {
            c->err = "goal planner: 16 bucket counts of std::unordered_map do not cover a grid row of " + std::to_string(rows_max) + " cells";
            return LSC_EINVAL;
        }
    }
    const int nx = c->edt_dims[0], ny = c->edt_dims[1], nz = c->edt_dims[2];
    const double rf = 1.0 / c->edt_res;
    auto edt_at = [&](const float p[3]) -> float {
        int cc[3];
        const int dims[3] = {nx, ny, nz};
        for (int a = 0; a < 3; a++) {
            cc[a] = (int)std::floor(rf * (double)p[a]) + 32768 - c->edt_kmin[a];
            if (cc[a] < 0 || cc[a] >= dims[a]) return -1.0f;
        }
        return c->h_edt[((size_t)cc[0] * ny + cc[1]) * nz + cc[2]];
    };
    // a map from a device occupancy (lsc_set_occupancy): the grids are filled by lsc_map.hip's chain from the index tables below
    const bool on_device = (bool)c->occ.d_occ;
    if (on_device) {
        std::vector<int> cell_of;
        const int dims[3] = {nx, ny, nz};
        for (int a = 0; a < 3; a++)
            for (int i = 0; i < dim[a]; i++) cell_of.push_back(map_goal_cell(c->grid_min[a], i, res, rf, c->edt_kmin[a], dims[a]));
        HIPCHK(c, c->occ.d_cell_of.upload(cell_of.data(), cell_of.size()));
    }
    std::vector<unsigned char> occ(on_device ? 0 : C * radii.size(), 0);
    const float margin = (float)c->cfg.grid_margin;
    for (size_t r = 0; r < radii.size() && !on_device; r++)
        for (int i = 0; i < H; i++)
            for (int j = 0; j < W; j++)
                for (int k = 0; k < A; k++) {
                    const float p[3] = {(float)(c->grid_min[0] + i * res), (float)(c->grid_min[1] + j * res),
                                        (float)(c->grid_min[2] + k * res)};
                    if ((double)edt_at(p) < radii[r] + (double)margin) occ[r * C + (size_t)H * W * k + (size_t)W * i + j] = 1;
                }
    c->swarm.map = MapMem{};
    MapMem &m = c->swarm.map;
    if (!c->h_fcode.empty()) HIPCHK(c, m.d_fcode.upload(c->h_fcode.data(), c->h_fcode.size()));
    if (on_device) {
        HIPCHK(c, m.d_occ_static.alloc(C * radii.size()));           // (the field is OccMem::d_edt)
    } else {
        HIPCHK(c, m.d_edt.upload(c->h_edt.data(), c->h_edt.size()));
        HIPCHK(c, m.d_occ_static.upload(occ.data(), occ.size()));
    }
    const size_t N = (size_t)c->N;
    HIPCHK(c, m.d_goal_planned.alloc(3 * N));
    HIPCHK(c, m.d_goal_err.alloc_zero(N));
    HIPCHK(c, m.d_goal_flags.alloc(N));
    HIPCHK(c, m.d_goal_exp.alloc(N));
    HIPCHK(c, m.d_ray_stack.alloc(N * 64 * 24 * 6));
    HIPCHK(c, m.d_goal_storage.alloc_zero(N));
    if (int rc = alloc_goal_ws(c)) return rc;
    if (c->goal_ws_bytes) {
        char buf[256];
        std::snprintf(buf, sizeof buf, "goal planner: %s, %d x %d x %d grid: %.2f MB of HBM workspace per agent (%.1f MB for %d agents)",
                      c->goal_hbm ? (c->goal_hbm == 1 ? "HBM search (cell bytes in LDS)" : "HBM search (cell bytes in HBM)")
                                  : "LDS search, restarted in HBM when a row outgrows its LDS capacity",
                      H, W, A, c->goal_ws_bytes / 1e6, c->goal_ws_bytes * (double)c->swarm.map.goal_ws_agents / 1e6, c->swarm.map.goal_ws_agents);
        const size_t prev = c->note.find("goal planner:");             // (a remark of an earlier map goes)
        if (prev != std::string::npos) c->note.erase(prev >= 2 ? prev - 2 : prev);
        c->note += (c->note.empty() ? "" : "; ") + std::string(buf);
    }
    return LSC_OK;
}

// The whole rebuild of a map whose source is the device occupancy, enqueued on `st`: the distance field and -- for a context with
// agents -- the integral images and goal grids, into the buffers the ticks read.  No allocation, no synchronise.
static int map_enqueue_build(lsc_ctx *c, hipStream_t st)
{
    const OccMem &o = c->occ;
    MapArgs a = {};
    a.nx = c->edt_dims[0]; a.ny = c->edt_dims[1]; a.nz = c->edt_dims[2];
    a.md = o.md; a.trunc2 = o.md * o.md;
    a.occ = o.d_occ; a.pass_a = o.d_pass_a; a.pass_b = o.d_pass_b; a.table = o.d_table; a.edt = o.d_edt;
    if (o.n_radii > 0 && c->swarm.d_integral) {
        a.n_radii = o.n_radii;
        a.thr_blocked = o.d_thr; a.thr_goal = o.d_thr + o.n_radii;
        a.integral = c->swarm.d_integral;
        if (c->swarm.map.d_occ_static) {
            a.H = c->grid_dims[0]; a.W = c->grid_dims[1]; a.A = c->grid_dims[2];
            a.cell_of = o.d_cell_of; a.goal_occ = c->swarm.map.d_occ_static;
        }
    }
    HIPCHK(c, launch_map_build(a, st));
    return LSC_OK;
}

// what lsc_set_distmap and lsc_set_occupancy refuse alike
static int map_refusals(lsc_ctx *c, const char *who, double res)
{
    // The corridor kernel visits the reference's lattice samples (spacing world/resolution) as contiguous cell ranges of
    // the distance field: that is only the same set when both resolutions agree (they do in every shipped launch file)
    if (std::fabs(res - c->cfg.world_resolution) > 1e-9 * res) {
        c->err = std::string(who) + ": map resolution differs from world_resolution";
        return LSC_EINVAL;
    }
    // ... and only while the float 1e-5 by which the reference nudges every lattice sample survives the float32 addition: from 256 m on
    // a float32 step is 3.05e-5 m, `x + 1e-5f` rounds back to x, the reference's samples skip cells and its boxes are no longer those of
    // contiguous ranges (rule_sfc_axis_cells, lsc_rules.hpp).  A sample lies at most one step outside the world box.  (The world box is
    // fixed at lsc_create, so this is the one place it meets a distance field.)
    if (c->cfg.use_octomap) {
        double reach = 0.0;
        for (int k = 0; k < 3; k++) reach = std::max(reach, std::max(std::fabs((double)c->cfg.world_min[k]), std::fabs((double)c->cfg.world_max[k])));
        if (!(reach + c->cfg.world_resolution < SFC_WORLD_REACH_MAX)) {
            char buf[320];
            std::snprintf(buf, sizeof buf, "%s: use_octomap needs max(|world_min|, |world_max|) + world_resolution < %g m on every axis (this world: "
                          "%g m): beyond it the float32 lattice samples of the reference's corridor test no longer feel their 1e-5 nudge and "
                          "skip cells, which the corridor kernel's contiguous cell ranges do not reproduce", who, SFC_WORLD_REACH_MAX, reach + c->cfg.world_resolution);
            c->err = buf;
            return LSC_EINVAL;
        }
    }
    return LSC_OK;
}

// blocked-cell integral images, one per distinct agent radius:  blocked = EDT < r + res/2 - 1e-5
// (include/corridor_constructor.hpp:114)
static int build_integrals(lsc_ctx *c)
{
    if ((c->h_edt.empty() && !c->occ.d_occ) || c->N == 0) return LSC_OK;
    const int nx = c->edt_dims[0], ny = c->edt_dims[1], nz = c->edt_dims[2];
    std::vector<double> radii;
    std::vector<int> img(c->N);
    for (int q = 0; q < c->N; q++) {
        auto it = std::find(radii.begin(), radii.end(), c->h_radius[q]);
        if (it == radii.end()) { radii.push_back(c->h_radius[q]); img[q] = (int)radii.size() - 1; }
        else img[q] = (int)(it - radii.begin());
    }
    const size_t isz = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
    if (c->occ.d_occ) {
        // the map's source is a device occupancy: the same thresholds, in the host's doubles; the images and grids are the chain's
        // (lsc_map.hip), which writes every entry of both
        std::vector<double> thr(2 * radii.size());
        for (size_t r = 0; r < radii.size(); r++) {
            thr[r] = radii[r] + 0.5 * c->cfg.world_resolution - 1e-5;
            thr[radii.size() + r] = radii[r] + (double)(float)c->cfg.grid_margin;
        }
        c->occ.n_radii = 0;                              // (until everything below stands: an update in between builds the field only)
        HIPCHK(c, c->occ.d_thr.upload(thr.data(), thr.size()));
        HIPCHK(c, c->swarm.d_integral.alloc(isz * radii.size()));
        HIPCHK(c, c->swarm.d_img_of_agent.upload(img.data(), img.size()));
        if (int rc = build_goal_grid(c, radii)) return rc;
        c->occ.n_radii = (int)radii.size();
        if (int rc = map_enqueue_build(c, c->stream)) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return LSC_OK;
    }
    std::vector<int> I(isz * radii.size(), 0);
    for (size_t r = 0; r < radii.size(); r++) {
        const double thr = radii[r] + 0.5 * c->cfg.world_resolution - 1e-5;
        int *J = I.data() + r * isz;
        auto at = [&](int x, int y, int z) -> int & { return J[((size_t)x * (ny + 1) + y) * (nz + 1) + z]; };
        for (int x = 1; x <= nx; x++)
            for (int y = 1; y <= ny; y++)
                for (int z = 1; z <= nz; z++) {
                    const int b = (double)c->h_edt[((size_t)(x - 1) * ny + (y - 1)) * nz + (z - 1)] < thr ? 1 : 0;
                    at(x, y, z) = b + at(x - 1, y, z) + at(x, y - 1, z) + at(x, y, z - 1) - at(x - 1, y - 1, z) - at(x - 1, y, z - 1) -
                                  at(x, y - 1, z - 1) + at(x - 1, y - 1, z - 1);
                }
    }
    HIPCHK(c, c->swarm.d_integral.upload(I.data(), I.size()));
    HIPCHK(c, c->swarm.d_img_of_agent.upload(img.data(), img.size()));
    return build_goal_grid(c, radii);
}

int lsc_set_distmap(lsc_ctx *c, const float *edt, int nx, int ny, int nz, const int key_min[3], double res)
{
    if (!c || !edt || nx < 1 || ny < 1 || nz < 1 || !key_min || !(res > 0)) return LSC_EINVAL;
    if (int rc = map_refusals(c, "lsc_set_distmap", res)) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->occ.d_occ) {                              // the map is replaced: a device occupancy goes with it
        HIPCHK(c, hipDeviceSynchronize());
        c->occ = OccMem{};
    }
    c->h_edt.assign(edt, edt + (size_t)nx * ny * nz);
    c->edt_dims[0] = nx; c->edt_dims[1] = ny; c->edt_dims[2] = nz;
    for (int k = 0; k < 3; k++) c->edt_kmin[k] = key_min[k];
    c->edt_res = res;
    return build_integrals(c);
}

// The map from an occupancy grid: the field and everything derived from it are built on the device (lsc_map.hip) and rebuilt there by
// lsc_map_update*.  Allocates everything an update needs.
int lsc_set_occupancy(lsc_ctx *c, const unsigned char *occ, int nx, int ny, int nz, const int key_min[3], double res, double maxdist)
{
    if (!c) return LSC_EINVAL;
    if (!occ || !key_min) { c->err = "lsc_set_occupancy: null argument"; return LSC_EINVAL; }
    if (nx < 1 || ny < 1 || nz < 1) { c->err = "lsc_set_occupancy: every dimension of the grid must be at least 1"; return LSC_EINVAL; }
    if (!(res > 0)) { c->err = "lsc_set_occupancy: the resolution must be positive"; return LSC_EINVAL; }
    if (!(maxdist > 0) || !std::isfinite(maxdist)) { c->err = "lsc_set_occupancy: maxdist must be positive and finite"; return LSC_EINVAL; }
    if (!(maxdist / res + 1 < (double)(MAP_MD_MAX + 1))) {           // (int)(maxdist / res + 1) > MAP_MD_MAX
        char buf[200];
        std::snprintf(buf, sizeof buf, "lsc_set_occupancy: maxdist / res + 1 = %g cells, more than the %d the 16-bit passes of the distance field hold",
                      maxdist / res + 1, MAP_MD_MAX);
        c->err = buf;
        return LSC_EINVAL;
    }
    if (int rc = map_refusals(c, "lsc_set_occupancy", res)) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());               // (a tick may still read the buffers this call replaces)
    const size_t cells = (size_t)nx * ny * nz;
    OccMem o;
    o.md = map_truncation_cells(maxdist, res);
    std::vector<float> table((size_t)o.md * o.md + 1);
    for (size_t d2 = 0; d2 < table.size(); d2++) table[d2] = map_edt_table_entry((int)d2, res);
    HIPCHK(c, o.d_occ.upload(occ, cells));
    HIPCHK(c, o.d_pass_a.alloc(cells));
    HIPCHK(c, o.d_pass_b.alloc(cells));
    HIPCHK(c, o.d_edt.alloc(cells));
    HIPCHK(c, o.d_table.upload(table.data(), table.size()));
    c->occ = std::move(o);
    c->h_edt.clear();
    c->edt_dims[0] = nx; c->edt_dims[1] = ny; c->edt_dims[2] = nz;
    for (int k = 0; k < 3; k++) c->edt_kmin[k] = key_min[k];
    c->edt_res = res;
    if (c->N == 0) {                                 // no agents yet: the field alone; lsc_set_agents builds the rest
        if (int rc = map_enqueue_build(c, c->stream)) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return LSC_OK;
    }
    return build_integrals(c);
}

// what lsc_map_update and lsc_map_update_device share: the rebuild behind the edit, and the flag
static int map_rebuild(lsc_ctx *c, int flags, hipStream_t st)
{
    if (int rc = map_enqueue_build(c, st)) return rc;
    if ((flags & LSC_MAP_REGROW_CORRIDORS) && c->swarm.d_sfc_init)
        HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->swarm.d_sfc_init.get(), 1, (size_t)c->N, st));     // flag_initialize_sfc of every agent
    return LSC_OK;
}

int lsc_map_update(lsc_ctx *c, int n_boxes, const int *boxes, const unsigned char *values, int flags, void *hip_stream)
{
    if (!c) return LSC_EINVAL;
    if (!c->occ.d_occ) { c->err = "lsc_map_update: the context's map is not a device occupancy (lsc_set_occupancy was not called, or lsc_set_distmap replaced it)"; return LSC_ESTATE; }
    if (n_boxes < 0 || n_boxes > MAP_BOXES_MAX) { c->err = "lsc_map_update: n_boxes must be 0 .. " + std::to_string(MAP_BOXES_MAX); return LSC_EINVAL; }
    if (n_boxes > 0 && (!boxes || !values)) { c->err = "lsc_map_update: null boxes or values"; return LSC_EINVAL; }
    if (flags & ~LSC_MAP_REGROW_CORRIDORS) { c->err = "lsc_map_update: unknown flag"; return LSC_EINVAL; }
    // the boxes travel in the edit kernel's argument block: nothing of the caller's or the context's is read after this call returns
    MapBoxes b = {};
    b.n = n_boxes;
    for (int i = 0; i < n_boxes; i++) {
        for (int k = 0; k < 3; k++) {
            const int lo = boxes[6 * i + k], hi = boxes[6 * i + 3 + k];
            if (lo < 0 || hi > c->edt_dims[k] || lo >= hi) {
                char buf[200];
                std::snprintf(buf, sizeof buf, "lsc_map_update: box %d, axis %d: [%d, %d) is empty or outside the field's 0 .. %d", i, k, lo, hi, c->edt_dims[k]);
                c->err = buf;
                return LSC_EINVAL;
            }
            b.box[i][k] = lo; b.box[i][3 + k] = hi;
        }
        if (values[i] > 1) { c->err = "lsc_map_update: box " + std::to_string(i) + ": value must be 0 (free) or 1 (occupied)"; return LSC_EINVAL; }
        b.value[i] = values[i];
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(c, launch_map_edit(c->occ.d_occ, c->edt_dims[0], c->edt_dims[1], c->edt_dims[2], b, st));
    return map_rebuild(c, flags, st);
}

int lsc_map_update_device(lsc_ctx *c, const unsigned char *d_occ, int flags, void *hip_stream)
{
    if (!c) return LSC_EINVAL;
    if (!c->occ.d_occ) { c->err = "lsc_map_update_device: the context's map is not a device occupancy (lsc_set_occupancy was not called, or lsc_set_distmap replaced it)"; return LSC_ESTATE; }
    if (!d_occ) { c->err = "lsc_map_update_device: null grid"; return LSC_EINVAL; }
    if (flags & ~LSC_MAP_REGROW_CORRIDORS) { c->err = "lsc_map_update_device: unknown flag"; return LSC_EINVAL; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(c, hipMemcpyAsync(c->occ.d_occ, d_occ, c->occ.d_occ.size(), hipMemcpyDeviceToDevice, st));
    return map_rebuild(c, flags, st);
}

// Diagnostics (copies only, synchronises the device): the map as the kernels read it, whichever entry point it came from.
int lsc_map_read(lsc_ctx *c, int which, void *out, size_t bytes)
{
    if (!c || !out) return LSC_EINVAL;
    const bool dev = (bool)c->occ.d_occ;
    if (!dev && c->h_edt.empty()) { c->err = "lsc_map_read: the context has no map"; return LSC_ESTATE; }
    const size_t cells = (size_t)c->edt_dims[0] * c->edt_dims[1] * c->edt_dims[2];
    const size_t C = c->swarm.map.d_occ_static ? (size_t)c->grid_dims[0] * c->grid_dims[1] * c->grid_dims[2] : 0;
    const size_t isz = (size_t)(c->edt_dims[0] + 1) * (c->edt_dims[1] + 1) * (c->edt_dims[2] + 1);
    const size_t n_radii = c->swarm.d_integral ? c->swarm.d_integral.size() / isz : 0;
    const void *src = nullptr;
    size_t want = 0;
    bool host = false;
    int dims[LSC_MAP_DIMS_INTS] = {c->edt_dims[0], c->edt_dims[1], c->edt_dims[2], (int)n_radii, C ? c->grid_dims[0] : 0, C ? c->grid_dims[1] : 0,
                                   C ? c->grid_dims[2] : 0, dev ? 1 : 0};
    switch (which) {
    case LSC_MAP_DIMS: src = dims; want = sizeof dims; host = true; break;
    case LSC_MAP_OCCUPANCY:
        if (!dev) { c->err = "lsc_map_read: the context's map is not a device occupancy"; return LSC_ESTATE; }
        src = c->occ.d_occ.get(); want = cells; break;
    case LSC_MAP_EDT:
        // the buffer castRay reads where the context has one (the uploaded field of lsc_set_distmap included); a context that plans no
        // goals on the map keeps the host's field only (the corridor kernel reads the integral images)
        if (dev) src = c->occ.d_edt.get();
        else if (c->swarm.map.d_edt) src = c->swarm.map.d_edt.get();
        else { src = c->h_edt.data(); host = true; }
        want = sizeof(float) * cells; break;
    case LSC_MAP_INTEGRAL: src = c->swarm.d_integral.get(); want = sizeof(int) * isz * n_radii; break;
    case LSC_MAP_GOAL_OCCUPANCY: src = c->swarm.map.d_occ_static.get(); want = C * n_radii; break;
    default: c->err = "lsc_map_read: unknown product"; return LSC_EINVAL;
    }
    if (bytes != want) { c->err = "lsc_map_read: the product has " + std::to_string(want) + " bytes, the buffer " + std::to_string(bytes); return LSC_EINVAL; }
    if (want == 0) return LSC_OK;
    if (host) { std::memcpy(out, src, want); return LSC_OK; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, src, want, hipMemcpyDeviceToHost));
    return LSC_OK;
}

// goalPlanning(): fused into phase A of the plan kernel on maps without a distance field; with one it is a launch of
// its own (lsc_goal.hip) whose output replaces the goal input of the SFC and plan kernels
static bool plans_goals(const lsc_ctx *c) { return c->cfg.goal_mode == 1 && c->cfg.use_octomap; }

static int fill_goal_args(lsc_ctx *c, GoalArgs &g, const float *d_state, const float *d_goal, const float *d_prev, int seq)
{
    if (!c->swarm.map.d_occ_static) { c->err = "goal_mode prior_based with use_octomap: lsc_set_distmap was not called"; return LSC_ESTATE; }
    g.N = c->N; g.first = c->first; g.count = c->count; g.planner_seq = seq; g.dtf = (float)c->cfg.dt;
    g.state = d_state; g.goal = d_goal; g.traj_prev = d_prev;
    g.radius = c->swarm.d_radius; g.downwash = c->swarm.d_downwash; g.radius_obs = c->swarm.d_radius_obs; g.downwash_obs = c->swarm.d_downwash_obs;
    g.goal_threshold = c->cfg.goal_threshold; g.priority_dist_threshold = c->cfg.priority_dist_threshold;
    g.goal_radius = c->cfg.goal_radius;
    g.H = c->grid_dims[0]; g.W = c->grid_dims[1]; g.A = c->grid_dims[2]; g.dim2 = c->cfg.world_dimension == 2 ? 1 : 0;
    for (int k = 0; k < 3; k++) { g.gmin[k] = c->grid_min[k]; g.key_min[k] = c->edt_kmin[k]; }
    g.gres = c->cfg.grid_resolution;
    g.occ_static = c->swarm.map.d_occ_static; g.img_of_agent = c->swarm.d_img_of_agent;
    g.edt = c->occ.d_edt ? c->occ.d_edt.get() : c->swarm.map.d_edt.get(); g.nx = c->edt_dims[0]; g.ny = c->edt_dims[1]; g.nz = c->edt_dims[2];
    g.rf = 1.0 / c->edt_res; g.wres = c->cfg.world_resolution;
    g.n_nb = (int)c->nb_seq.size();
    for (int k = 0; k < 16; k++) {
        g.nb_seq[k] = k < g.n_nb ? c->nb_seq[k] : 0;
        g.nb_magic[k] = k < g.n_nb ? (uint32_t)(0x100000000ull / (uint32_t)c->nb_seq[k]) : 0u;
    }
    g.row_cap = c->grid_row_cap;
    g.variant = c->cfg.goal_search == 1 ? 0 : goal_fast_slots(g.H, g.W, g.A, &g.jbits);
    if (g.variant == 0) g.jbits = 0;
    g.fcode = nullptr; g.fcode_n = 0; g.fcode_rb = 0;
    if (g.variant != 0 && c->swarm.map.d_fcode) { g.variant |= 8; g.fcode = c->swarm.map.d_fcode; g.fcode_n = (int)c->h_fcode.size(); g.fcode_rb = c->fcode_rb; }
    g.goal_out = c->swarm.map.d_goal_planned; g.err = c->swarm.map.d_goal_err; g.flags = c->swarm.map.d_goal_flags; g.expansions = c->swarm.map.d_goal_exp;
    g.path_out = c->swarm.d_goal_path; g.path_cap = c->goal_path_cap; g.path_len = c->swarm.d_goal_plen;
    g.ray_stack = c->swarm.map.d_ray_stack;
    g.reset_thr = c->cfg.planner_mode == 0 ? c->cfg.reset_threshold : 0.0; g.ever = c->swarm.d_ever;
    g.prof = c->goal_profiling ? c->swarm.d_goal_prof.get() : nullptr;
    g.smem_bytes = 0;                                  // (set by the launch)
    if (int rc = alloc_goal_ws(c)) return rc;
    g.hbm = c->goal_hbm;
    g.ws = c->goal_ws_bytes ? c->swarm.map.d_goal_ws.get() : nullptr;
    g.ws_stride = c->goal_ws_bytes;
    g.storage = c->swarm.map.d_goal_storage;
    if (c->goal_hbm) { g.variant = 0; g.jbits = 0; }  // (the HBM search is the general search)
    if (c->goal_hbm && g.prof) {
        c->err = "lsc_goal_profile: this context's grid is searched in HBM; the profile covers the LDS searches only";
        return LSC_ESTATE;
    }
    return LSC_OK;
}

static int run_goal(lsc_ctx *c, const float *d_state, const float *&d_goal, const float *d_prev, int seq, hipStream_t st)
{
    if (!plans_goals(c)) return LSC_OK;
    GoalArgs g;
    if (int rc = fill_goal_args(c, g, d_state, d_goal, d_prev, seq)) return rc;
    LaunchEvents ev;
    if (c->timing && timing_begin(c, 3, &ev) != LSC_OK) return LSC_EHIP;
    HIPCHK(c, launch_goal(g, st, ev));
    d_goal = c->swarm.map.d_goal_planned;
    return LSC_OK;
}

static int fill_sfc_args(lsc_ctx *c, SfcArgs &s, const float *d_state, const float *d_goal, const float *d_prev, int seq)
{
    if (!c->swarm.d_integral) { c->err = "use_octomap is set but lsc_set_distmap was not called"; return LSC_ESTATE; }
    s.N = c->N; s.first = c->first; s.count = c->count;
    s.state = d_state; s.goal = d_goal; s.traj_prev = d_prev;
    s.radius = c->swarm.d_radius; s.img_of_agent = c->swarm.d_img_of_agent; s.integral = c->swarm.d_integral;
    s.nx = c->edt_dims[0]; s.ny = c->edt_dims[1]; s.nz = c->edt_dims[2];
    for (int k = 0; k < 3; k++) { s.key_min[k] = c->edt_kmin[k]; s.world_min[k] = c->cfg.world_min[k]; s.world_max[k] = c->cfg.world_max[k]; }
    s.rf = 1.0 / c->edt_res; s.wres = c->cfg.world_resolution;
    s.sfc = c->swarm.d_sfc; s.init_flag = c->swarm.d_sfc_init; s.err = c->swarm.d_sfc_err;
    double ext = 0.0;
    for (int k = 0; k < 3; k++) ext = std::max(ext, (double)c->cfg.world_max[k] - (double)c->cfg.world_min[k]);
    s.table_len = (int)std::ceil(ext / c->cfg.world_resolution) + 8;
    s.planner_seq = seq; s.reset_thr = c->cfg.planner_mode == 0 ? c->cfg.reset_threshold : 0.0;
    if (sizeof(double) * 6 * (size_t)s.table_len > LDS_MAX_BYTES) {
        c->err = "world extent / world_resolution too large for the SFC face tables (limit 3400 steps per axis)";
        return LSC_EINVAL;
    }
    return LSC_OK;
}

static int run_sfc(lsc_ctx *c, const float *d_state, const float *d_goal, const float *d_prev, int seq, hipStream_t st)
{
    if (!c->cfg.use_octomap) return LSC_OK;
    SfcArgs s;
    if (int rc = fill_sfc_args(c, s, d_state, d_goal, d_prev, seq)) return rc;
    LaunchEvents ev;
    if (c->timing && timing_begin(c, 4, &ev) != LSC_OK) return LSC_EHIP;
    HIPCHK(c, launch_sfc(s, st, ev));
    return LSC_OK;
}

static int fill_plan_args(lsc_ctx *c, PlanArgs &a, const float *d_state, const float *d_goal, const float *d_prev, int seq,
                          float *d_next, double *d_cost, int *d_status, int *d_iters)
{
    if (c->N == 0) return LSC_ESTATE;
    a.model = c->own.d_model; a.terms = c->own.d_terms; a.entries = c->own.d_entries;
    a.N = c->N; a.first = c->first; a.count = c->count; a.planner_seq = seq; a.cap = c->cap;
    a.dim2 = c->cfg.world_dimension == 2 ? 1 : 0;
    a.solver = c->cfg.solver;
    a.solver_stats = c->swarm.d_iters_acc ? c->swarm.d_iters_acc + 2 * (size_t)c->N : nullptr;      // ([N][4] counters behind the two per-agent blocks)
    a.cap_tp = (c->count > c->n_cu) ? c->cap_tp : 0; a.smem_tp = c->smem_tp;
    a.order = (c->count > 2 * c->n_cu) ? c->swarm.d_order.get() : nullptr;   // more than one round of throughput workgroups
    a.obs_bound = c->swarm.d_obs_bound;                                // obstacle-level pre-cull (throughput build; latency build of large swarms: launch_plan decides)
    a.neigh = c->swarm.neigh.cnt ? &c->swarm.neigh : nullptr;                // neighbour lists of a large swarm: run_plan launches their kernels and sets the three fields below
    a.nv = nullptr;
    c->neigh_skipped = "only single ticks (run_plan) build them, not batched ticks or dense sweeps";      // (run_plan overwrites this)
    a.state = d_state; a.goal = d_goal; a.traj_prev = d_prev;
    a.radius = c->swarm.d_radius; a.radius_obs = c->swarm.d_radius_obs; a.downwash = c->swarm.d_downwash; a.downwash_obs = c->swarm.d_downwash_obs;
    a.vmax = c->swarm.d_vmax; a.amax = c->swarm.d_amax; a.vnom = c->swarm.d_vnom;
    a.traj_next = d_next; a.cost = d_cost; a.status = d_status; a.iters = d_iters; a.nrows = c->swarm.d_nrows; a.bucket_max = c->swarm.d_bmax; a.iters_acc = c->swarm.d_iters_acc;
    a.stale = c->swarm.d_stale; a.sfc = c->cfg.use_octomap ? c->swarm.d_sfc.get() : nullptr;
    a.sfc_err = c->cfg.use_octomap ? c->swarm.d_sfc_err.get() : nullptr;
    const bool planned = c->cfg.goal_mode == 1 && c->cfg.use_octomap;   // goals come from lsc_goal_kernel
    a.goal_err = planned ? c->swarm.map.d_goal_err.get() : nullptr;
    a.out_normal = nullptr; a.out_d = nullptr;
    a.goal_mode = planned ? 0 : c->cfg.goal_mode; a.goal_threshold = c->cfg.goal_threshold;
    a.priority_dist_threshold = c->cfg.priority_dist_threshold; a.goal_radius = c->cfg.goal_radius;
    a.goal_out = c->swarm.d_goal_cur; a.state_next = nullptr; a.finv = (float)std::pow(c->cfg.dt, -1);
    a.dbg = c->swarm.d_dbg; a.prof = c->profiling ? c->swarm.d_prof.get() : nullptr;
    a.trace = c->trace_agent >= 0 ? c->own.d_trace.get() : nullptr; a.trace_agent = c->trace_agent;
    a.spill_ws = c->swarm.d_spill; a.spill_stride = c->swarm.spill_stride;
    a.gmodel = c->own.d_gmodel; a.planner_mode = c->cfg.planner_mode; a.slack_mode = c->cfg.slack_mode;
    a.ncs = c->cfg.n_constraint_segments; a.general_all = (c->cfg.planner_mode == 1 || c->cfg.slack_mode != 0) ? 1 : 0;
    a.slack_w = c->cfg.slack_collision_weight; a.reset_thr = c->cfg.planner_mode == 0 ? c->cfg.reset_threshold : 0.0;
    a.ever = c->swarm.d_ever; a.gen_ws = c->swarm.d_gen_ws; a.gen_stride = c->swarm.gen_stride;
    a.fold = 0;                          // (run_plan decides)
    a.t_begin = nullptr; a.t_end = nullptr;      // (a timed launch's stamps: launch_variant puts them in)
    a.generic_lsc_build = c->generic_lsc_build ? 1 : 0;
    a.step_all_slots = c->step_all_slots ? 1 : 0;
    a.plain_handover = c->plain_handover ? 1 : 0;
    a.ws_peak = c->swarm.d_ws_peak;
    // dynamic obstacles: their block selects the OBS instantiations; the second pass then holds 27 (N - 1 + K) rows
    const ObsMem &ob = c->swarm.obs;
    a.obs = ob.K > 0 ? ob.d_block.get() : nullptr;
    if (ob.K > 0) { a.spill_ws = ob.d_spill; a.spill_stride = ob.spill_stride; }
    // ... and the alternate-mode solver's rows of N - 1 + K obstacles (lsc_set_obstacles_ex)
    if (ob.K > 0 && ob.d_gen_ws) { a.gen_ws = ob.d_gen_ws; a.gen_stride = ob.gen_stride; }
    return LSC_OK;
}

// Whether lsc_general_kernel has to run in this tick.  The alternate-mode kernel follows the plan kernel when a
// configured mode sends every agent there (BVC, slack modes).  With the disturbance checks on, a host-buffer tick knows
// the answer exactly (same float32 test on the host copy of the inputs, general_hint 0 / 1); a device-resident tick does
// not see the states (hint -1) and launches the kernel, whose workgroups leave at once when nobody was flagged -- unless the plan
// kernel folds the hand-over (run_plan: PlanArgs::fold), in which case no launch follows at all.
static bool want_general(const lsc_ctx *c, int general_hint)
{
    if (!c->swarm.d_gen_ws) return false;
    if (c->cfg.planner_mode == 1 || c->cfg.slack_mode != 0) return true;
    return general_hint != 0;
}

// the disturbance checks on host copies (rule_off_plan, the host compile of what the kernels call); keeps the
// host mirror of the persistent flags in step with the device's
static int host_disturbance_hint(lsc_ctx *c, const float *state, const float *prev_traj, int planner_seq)
{
    if (!(c->cfg.reset_threshold > 0.0) || c->cfg.planner_mode != 0) return 0;
    if (c->h_ever_stale) {
        // device-resident ticks have run since the mirror was last in step: they flag agents on the device only
        if (c->swarm.d_ever && !c->h_ever.empty() &&
            (hipDeviceSynchronize() != hipSuccess ||
             hipMemcpy(c->h_ever.data(), c->swarm.d_ever, c->h_ever.size(), hipMemcpyDeviceToHost) != hipSuccess)) return 1;   // when in doubt, launch
        c->h_ever_stale = false;
    }
    int any = 0;
    for (int q = 0; q < c->N; q++) {
        if (planner_seq >= 2) {
            const float *t = prev_traj + (size_t)q * NV + NC;
            const float t1[3] = {t[0], t[SEGV], t[2 * SEGV]};
            if (rule_off_plan(t1, state + 9 * q, c->cfg.reset_threshold)) c->h_ever[q] = 1;
        }
        any |= c->h_ever[q];
    }
    return any;
}

// Planar worlds (world/dimension == 2).  The reference reads the planning agent's own position at z = world/z_2d whatever it is told
// (TrajPlanner::currentStateCallback, src/traj_planner.cpp:304-314), stores z = z_2d in every control point it plans
// (src/traj_optimizer.cpp:87-90) and drops the z term of every collision row (:450) -- which is only meaningful when the whole swarm
// sits in that plane, as it does in the reference's simulator (starts at z_2d, src/mission.cpp:88-93; ideal states evaluated from
// planar plans).  The kernels rely on exactly that, so the host-buffer ticks check it instead of planning something else silently.
static int planar_inputs_ok(lsc_ctx *c, const float *state, const float *prev_traj, int planner_seq)
{
    if (c->cfg.world_dimension != 2) return LSC_OK;
    const float z = (float)c->cfg.world_z_2d;
    for (int q = 0; q < c->N; q++) {
        bool ok = state[9 * (size_t)q + 2] == z;
        if (planner_seq >= 2) {
            const float *t = prev_traj + (size_t)q * NV + 2 * SEGV;
            for (int j = 0; j < SEGV; j++) ok = ok && t[j] == z;
        }
        if (!ok) {
            c->err = "planar world (world_dimension 2): agent " + std::to_string(q) + " is not at z = world_z_2d (state / previous plan)";
            return LSC_EINVAL;
        }
    }
    return LSC_OK;
}

static int run_plan(lsc_ctx *c, const PlanArgs &a_in, hipStream_t st, int general_hint = -1)
{
    const size_t smem = plan_smem_bytes(c->hm.m.n_terms, c->hm.m.n_entries, c->cap);
    LaunchEvents ev;
    // (events for an empty shard, which launches nothing and records them, and for a profiled launch or one of the throughput build: the
    //  instrumented kernels and the throughput kernels stamp nothing)
    if (c->timing && timing_begin(c, 0, &ev, st, (a_in.prof || plan_kernel_is_throughput(a_in)) ? 0 : a_in.count) != LSC_OK) return LSC_EHIP;
    PlanArgs a = a_in;
    // Neighbour lists cost two launches (~25 us at 1024 agents) and save every workgroup its walks over all N agents (cull: ~5 us per agent at
    // N = 1024, priority rule: ~4 us; both grow with N).  Worth it when the shard takes more than one round of workgroups or the swarm is
    // large; a one-round shard of a 1024-agent swarm is faster with the in-kernel walks (profiles/r06_neighbour_lists.log).
    const bool lists_pay = a.N >= 2048 || (a.cap_tp > 0 && a.count > 2 * c->n_cu) || c->neigh_always;
    c->neigh_skipped = !a.neigh ? "the context has none"
                       : !lists_pay ? "they do not pay for this shard (fewer than 2048 agents and at most one round of workgroups; LSC_NEIGH_ALWAYS forces them)"
                       : a.count <= 0 ? "the shard is empty"
                       : a.out_normal ? "a tick that dumps its constraints walks all obstacles"
                       : a.general_all ? "every agent plans in lsc_general_kernel (BVC or slack mode)"
                       : a.trace ? "a traced tick walks all obstacles"
                       : a.obs ? "a tick with dynamic obstacles walks all obstacles" : nullptr;
    if (a.neigh && lists_pay && a.count > 0 && !a.out_normal && !a.general_all && !a.trace && !a.obs) {
        // large swarm: bounds of every agent + the grid, then the shard's unit lists (two small launches on the tick's stream, inside the timed region)
        NeighArgs &g = *a.neigh;
        if (++g.tag == 0) { HIPCHK(c, hipMemsetAsync(g.cells, 0, 32 * ((size_t)g.hmask + 1), st)); HIPCHK(c, hipMemsetAsync(g.glob, 0, 128, st)); g.tag = 1; }
        g.N = a.N; g.first = a.first; g.count = a.count; g.planner_seq = a.planner_seq; g.dtf = (float)c->hm.m.dt; g.dim2 = a.dim2;
        g.hv_scale = c->hm.m.hv_scale; g.ha_scale = c->hm.m.ha_scale; g.z2d = c->hm.m.z2d;
        g.state = a.state; g.traj_prev = a.traj_prev;
        g.radius = a.radius; g.radius_obs = a.radius_obs; g.downwash = a.downwash; g.downwash_obs = a.downwash_obs; g.vmax = a.vmax; g.amax = a.amax;
        g.order = (a.cap_tp > 0) ? a.order : nullptr; g.iters = a.iters; g.nrows = a.nrows; g.obs_bound = a.obs_bound;
        // phase A's walks over all agents: candidates of the priority rule by position, the disturbance checks once per agent
        g.goal_mode = a.goal_mode; g.prio_thr = a.priority_dist_threshold;
        g.checks = (plan_alt_hooks(a) && a.reset_thr > 0.0 && a.planner_seq >= 2 && a.planner_mode == 0 && a.ever != nullptr) ? 1 : 0;
        g.reset_thr = a.reset_thr; g.ever = a.ever;
        c->neigh_skipped = "the launch of their kernels failed";
        HIPCHK(c, launch_neigh(g, st, ev.first()));      // (the first launch of the timed group)
        c->neigh_skipped = nullptr;
        ev.start = nullptr; ev.t0 = nullptr;
        a.nv = g.view;
    }
    // The hand-over of disturbed agents, folded into the plan kernel (lsc_plan_alt_kernel + general_fold) where that kernel is the one-round
    // latency build of the disturbance checks: the launch of lsc_general_kernel behind it -- 3-4 us per tick, nearly always with nobody to
    // solve -- is gone.  It stays for the modes that send every agent there (BVC, slack), for the throughput build, behind the second pass,
    // and with LSC_GENERAL_HANDOVER.  The LDS request is then the larger of the two kernels' layouts (both fit 160 KB).
    const int n_dyn = a.obs ? c->swarm.obs.K : 0;      // (the second pass and the solver's LDS go by N - 1 + K obstacles per agent)
    a.fold = (a.gen_ws && !a.general_all && a.reset_thr > 0.0 && a.ever && !a.spill_ws && !c->general_handover && a.count <= c->swarm.gen_slots &&
              plan_kernel_folds(a)) ? 1 : 0;
    const size_t smem_plan = a.fold ? std::max(smem, general_lds_bytes(a.N + n_dyn)) : smem;
    // The timed group: start rides on its first launch (the neighbour build above, else the plan kernel), stop on its last -- known before
    // anything is launched: the hand-over if it will be launched, else the second pass, else the plan kernel.
    const int spill_slots = a.obs ? c->swarm.obs.spill_slots : c->swarm.spill_slots;
    const bool spill = a.spill_ws && a.count > 0 && spill_slots >= 1;
    const bool general = !a.fold && want_general(c, general_hint) && a.count > 0 && c->swarm.gen_slots >= 1 && a.gen_ws;
    HIPCHK(c, launch_plan(a, smem_plan, st, (spill || general) ? ev.first() : ev));
    if (spill) HIPCHK(c, launch_plan_spill(a, spill_slots, plan_smem_bytes(c->hm.m.n_terms, c->hm.m.n_entries, 0), st, general ? LaunchEvents() : ev.last()));
    if (general) HIPCHK(c, launch_general(a, c->swarm.gen_slots, st, ev.last(), n_dyn));
    c->last_general = a.fold ? 1 : (general ? 2 : 0);
    return LSC_OK;
}

// ---------------------------------------------------------------------------------------------------
// The goal stage (lsc_mission.hip): patrol / GOBACK on the context's mission tables and the right-hand rule, one launch in front of the tick.
// ---------------------------------------------------------------------------------------------------
static bool stage_in_use(const lsc_ctx *c) { return c->swarm.mission.open || c->goal_rule == LSC_GOAL_RULE_RIGHT_HAND; }

// in front of a tick (and at lsc_mission_open / lsc_set_goal_rule): LSC_OK for a context that uses no stage; with one, what it is not built for
static int mission_tick_ok(lsc_ctx *c, const char *fn)
{
    if (!stage_in_use(c)) return LSC_OK;
    const char *why = nullptr;
    if (c->comm && c->world != 1) why = "the context is a rank of a communicator of several ranks";
    else if (c->N > 0 && (c->first != 0 || c->count != c->N)) why = "the context's shard is not the whole swarm";
    else if (c->goal_path_cap > 0) why = "the goal trace is on";
    else if (c->goal_profiling) why = "goal profiling is on";
    if (!why) return LSC_OK;
    c->err = std::string(fn) + ": a mission state is open or the right-hand goal rule is set, and " + why;
    return LSC_EINVAL;
}

// The obstacle stage's launch: a context with motion models moves its obstacles itself, at the clock's time (refusals: obstacles_tick_ok)
// d_state: the tick's input state [N][9], which a chaser reads its target's position from
static int run_obstacles(lsc_ctx *c, const float *d_state, hipStream_t st)
{
    ObsMem &ob = c->swarm.obs;
    if (!ob.d_models) return LSC_OK;
    const double t = ob.clock_now - ob.clock_start;
    if (ob.n_chasers > 0 || ob.n_walkers > 0) {      // (one launch, instead of the closed forms' stage)
        ObstacleStepArgs a = {};
        a.K = ob.K; a.first = ob.no_step_yet ? 1 : 0; a.t = t; a.table = ob.d_models; a.chasers = ob.d_chasers; a.walkers = ob.d_walkers; a.acc = ob.d_acc;
        a.obs = ob.d_block; a.state = d_state; a.chaser_state = ob.d_chaser_state; a.pos_vel = ob.d_pos_vel; a.pos_f64 = ob.d_pos_f64;
        HIPCHK(c, launch_obstacle_step(a, st));
        ob.no_step_yet = false;
        if (ob.n_chasers > 0) ob.chaser_t_last = t;
    } else {
        ObstacleStageArgs a = {};
        a.K = ob.K; a.t = t; a.table = ob.d_models; a.pos_vel = ob.d_pos_vel; a.pos_f64 = ob.d_pos_f64;
        HIPCHK(c, launch_obstacle_stage(a, st));
    }
    ob.clock_now += ob.clock_step;
    return LSC_OK;
}

// The stage's launch; d_goal leaves as the table the rest of the tick reads: the desired goals of an open mission state, the rule's
// current goals with the right-hand rule, else the caller's pointer as it came.
static int run_mission(lsc_ctx *c, const float *d_state, const float *&d_goal, int seq, hipStream_t st, const char *fn)
{
    if (!stage_in_use(c)) return LSC_OK;             // (what the stage is not built for was refused at plan_context's entry: mission_tick_ok)
    MissionMem &ms = c->swarm.mission;
    const bool rule = c->goal_rule == LSC_GOAL_RULE_RIGHT_HAND;
    const size_t n3 = 3 * (size_t)c->N;
    if (!ms.open && !d_goal) { c->err = std::string(fn) + ": no goal table and no mission state"; return LSC_EINVAL; }
    if (rule && !ms.d_rule_goal) HIPCHK(c, ms.d_rule_goal.alloc_zero(n3));
    MissionArgs a = {};
    a.N = c->N; a.planner_state = ms.open ? ms.planner_state : MISSION_GOTO; a.planner_seq = seq;
    a.seq_threshold = c->deadlock_seq_threshold; a.velocity_threshold = c->deadlock_velocity_threshold;
    a.goal_threshold = c->cfg.goal_threshold;
    a.state = d_state; a.goal_in = d_goal;
    if (ms.open) {
        float *t = ms.d_tables;
        a.desired = t; a.start = t + n3; a.mission_start = t + 2 * n3; a.mission_goal = t + 3 * n3; a.legs = ms.d_legs;
        d_goal = a.desired;
    }
    a.rule_goal = rule ? ms.d_rule_goal.get() : nullptr;
    // (GOTO without the rule: the tables stay as they are, nothing to launch)
    if (a.rule_goal || a.planner_state != MISSION_GOTO) HIPCHK(c, launch_mission(a, st));
    if (rule) d_goal = a.rule_goal;
    return LSC_OK;
}

// One context's tick on a stream, in stream order: [obstacle stage], [goal stage], goal search, [dense constraint dumps allocated], corridor update, plan kernel with
// its second pass and hand-over (run_plan).  A host-buffer tick passes the host copies of its inputs (h_state, h_prev): the host then
// knows whether the hand-over has work (host_disturbance_hint); a device-resident tick passes null and the host mirror of the
// disturbance flags goes stale.  d_state_next: optional, the fused propagation's output.
static int plan_context(lsc_ctx *c, const float *d_state, const float *d_goal, const float *d_prev, int planner_seq, float *d_next,
                        float *d_state_next, double *d_cost, int *d_status, int *d_iters, bool dense_dumps, const float *h_state,
                        const float *h_prev, hipStream_t st, const char *fn, bool obstacles_checked = false)
{
    PlanArgs a;
    int rc = mission_tick_ok(c, fn);     // (a refused tick enqueues nothing: in front of the obstacles' upload)
    if (rc) return rc;
    // dynamic obstacles (a context without them takes none of this): refusals first -- the host-buffer ticks made them in front of their
    // upload, nothing is enqueued by a refused tick --, then their states in front of the tick's launches
    if (c->swarm.obs.K > 0) {
        if (!obstacles_checked) rc = obstacles_tick_ok(c, fn);
        if (!rc) rc = upload_obstacles(c, st);
        if (rc) return rc;
    }
    rc = run_obstacles(c, d_state, st);
    if (rc) return rc;
    rc = run_mission(c, d_state, d_goal, planner_seq, st, fn);
    if (rc) return rc;
    rc = run_goal(c, d_state, d_goal, d_prev, planner_seq, st);
    if (rc) return rc;
    rc = fill_plan_args(c, a, d_state, d_goal, d_prev, planner_seq, d_next, d_cost, d_status, d_iters);
    if (rc) return rc;
    a.state_next = d_state_next;
    if (dense_dumps) {
        // [count][obstacles per agent][M][3 | 6]: the N - 1 other agents, then the dynamic obstacles (buffers of the obstacles' lifetime)
        const size_t N = c->N, nobs = N - 1 + c->swarm.obs.K;
        DevBuf<float> &d_onormal = c->swarm.obs.K > 0 ? c->swarm.obs.d_onormal : c->swarm.d_onormal;
        DevBuf<double> &d_od = c->swarm.obs.K > 0 ? c->swarm.obs.d_od : c->swarm.d_od;
        if (!d_onormal) {
            HIPCHK(c, d_onormal.alloc(3 * M * nobs * N + 4));      // (16 bytes of slack each)
            HIPCHK(c, d_od.alloc(NC * M * nobs * N + 2));
        }
        a.out_normal = d_onormal; a.out_d = d_od;
    }
    rc = run_sfc(c, d_state, d_goal, d_prev, planner_seq, st);
    if (rc) return rc;
    if (h_state) return run_plan(c, a, st, host_disturbance_hint(c, h_state, h_prev, planner_seq));
    if (c->cfg.reset_threshold > 0.0) c->h_ever_stale = true;   // the device may flag agents the host mirror does not see
    return run_plan(c, a, st);
}

int lsc_tick_device(lsc_ctx *c, const float *d_state, const float *d_goal, const float *d_traj_prev, int planner_seq,
                    float *d_traj_next, double *d_cost, int *d_status, int *d_iters, void *hip_stream)
{
    if (!c || !d_state || (!d_goal && !c->swarm.mission.open) || !d_traj_prev || !d_traj_next || !d_cost || !d_status || !d_iters) return LSC_EINVAL;
    if (c->N == 0) return LSC_ESTATE;
    return plan_context(c, d_state, d_goal, d_traj_prev, planner_seq, d_traj_next, nullptr, d_cost, d_status, d_iters, false, nullptr, nullptr,
                        (hipStream_t)hip_stream, "lsc_tick_device");
}

int lsc_tick_device_fused(lsc_ctx *c, const float *d_state, const float *d_goal, const float *d_traj_prev, int planner_seq,
                          float *d_traj_next, float *d_state_next, double *d_cost, int *d_status, int *d_iters, void *hip_stream)
{
    if (!c || !d_state_next || !d_state || (!d_goal && !c->swarm.mission.open) || !d_traj_prev || !d_traj_next || !d_cost || !d_status || !d_iters) return LSC_EINVAL;
    if (c->N == 0) return LSC_ESTATE;
    return plan_context(c, d_state, d_goal, d_traj_prev, planner_seq, d_traj_next, d_state_next, d_cost, d_status, d_iters, false, nullptr,
                        nullptr, (hipStream_t)hip_stream, "lsc_tick_device_fused");
}

// One tick of several independent swarms, batched (blockIdx.y = swarm): the reference's mission list
// (src/multi_sync_simulator_node.cpp:43-70, src/param.cpp:106-122) as a batch axis.  Every context plans exactly what its own tick
// would plan for it -- the same instantiations of the goal search, the corridor update and the planning code read the context's own
// argument block -- so the results are the same bits; what changes is that a 20-agent swarm no longer has a 256-CU chip to itself.
// Stream order: goal batch (one launch per search instantiation among the contexts that plan goals on a distance field), SFC batch
// (contexts with a distance field), plan batch, the hand-over batch when the alternate-mode hooks are on.  `hint` (host-buffer form):
// per context the host's answer whether the hand-over launch has work (host_disturbance_hint); null: the device-resident form.
static int tick_batch(const char *fn, lsc_ctx *const *ctx, int n, const float *const *d_state, const float *const *d_goal,
                      const float *const *d_traj_prev, const int *planner_seq, float *const *d_traj_next, float *const *d_state_next,
                      double *const *d_cost, int *const *d_status, int *const *d_iters, const int *hint, hipStream_t st)
{
    lsc_ctx *c0 = ctx[0];
    PlanArgs a[PLAN_BATCH_MAX];
    GoalArgs g[PLAN_BATCH_MAX];
    SfcArgs s[PLAN_BATCH_MAX];
    int ng = 0, ns = 0;
    size_t smem = 0;
    int slots = 0x7fffffff;
    bool hooks = false, general = false;
    for (int i = 0; i < n; i++) {
        lsc_ctx *c = ctx[i];
        if (c->N == 0) { c0->err = std::string(fn) + ": context " + std::to_string(i) + " has no agents"; return LSC_ESTATE; }
        // what one launch can hold: swarms on this device that take the latency build with their rows in LDS and nothing between
        // their launches (sharded swarms exchange)
        const char *why = nullptr;
        if (c->cfg.device != c0->cfg.device) why = "is on another device";
        else if (c->comm || c->world != 1) why = "is a rank of a sharded swarm";
        else if (c->count > c->n_cu) why = "has more agents than the GPU has CUs (the throughput build is not batched)";
        else if (c->swarm.d_spill) why = "needs the second pass (row capacity below 27 (N - 1))";
        else if (c->profiling || c->trace_agent >= 0) why = "is being profiled / traced";
        else if (c->swarm.obs.K > 0) why = "has dynamic obstacles (lsc_set_obstacles: the batch ticks are not built for them)";
        else if (stage_in_use(c)) why = "has a mission state open or the right-hand goal rule set (lsc_mission_open / lsc_set_goal_rule: the batch ticks launch no goal stage)";
        else if (plans_goals(c) && c->swarm.d_goal_path) why = "has a goal trace on (lsc_set_goal_trace: the goal batch does not record paths)";
        else if (plans_goals(c) && c->goal_profiling) why = "has goal profiling on (the goal batch takes the non-profiling search only)";
        else if ((c->cfg.solver >= 1) != (c0->cfg.solver >= 1)) why = "has another QP solver than the first (one instantiation per launch)";
        for (int j = 0; j < i && !why; j++) if (ctx[j] == c) why = "appears twice (its stale-plan and hand-over buffers belong to ONE swarm of the launch)";
        if (why) { c0->err = std::string(fn) + ": context " + std::to_string(i) + " " + why; return LSC_EINVAL; }
        // the goal search replaces the goal input of the corridor and plan kernels, as run_goal does in a single tick
        const float *d_goal_in = d_goal[i];
        int rc = LSC_OK;
        if (plans_goals(c)) {
            rc = fill_goal_args(c, g[ng], d_state[i], d_goal[i], d_traj_prev[i], planner_seq[i]);
            if (!rc) { ng++; d_goal_in = c->swarm.map.d_goal_planned; }
        }
        if (!rc && c->cfg.use_octomap && !(rc = fill_sfc_args(c, s[ns], d_state[i], d_goal_in, d_traj_prev[i], planner_seq[i]))) ns++;
        if (!rc) rc = fill_plan_args(c, a[i], d_state[i], d_goal_in, d_traj_prev[i], planner_seq[i], d_traj_next[i], d_cost[i], d_status[i], d_iters[i]);
        if (rc) {
            if (c != c0) c0->err = std::string(fn) + ": context " + std::to_string(i) + ": " + c->err;
            return rc;
        }
        a[i].state_next = d_state_next ? d_state_next[i] : nullptr;
        const size_t sm = plan_smem_bytes(c->hm.m.n_terms, c->hm.m.n_entries, c->cap);
        smem = sm > smem ? sm : smem;
        if (want_general(c, -1)) { hooks = true; slots = c->swarm.gen_slots < slots ? c->swarm.gen_slots : slots; }
        general = general || want_general(c, hint ? hint[i] : -1);
    }
    // (all or none: the alternate-mode hooks are one instantiation per launch, and the hand-over launch covers every swarm of the batch)
    for (int i = 0; i < n; i++)
        if (want_general(ctx[i], -1) != hooks) { c0->err = std::string(fn) + ": contexts with and without alternate-mode hooks in one batch"; return LSC_EINVAL; }
    if (!hint)
        for (int i = 0; i < n; i++)
            if (ctx[i]->cfg.reset_threshold > 0.0) ctx[i]->h_ever_stale = true;
    // goal search: one launch per search instantiation (variant slots, Key32 or not), contexts in batch order within each
    if (ng > 0) {
        LaunchEvents ev;
        if (c0->timing && timing_begin(c0, 3, &ev) != LSC_OK) return LSC_EHIP;         // (timed on the first context, as the plan launch)
        int classes = 0;                               // (counted first: start rides on the first class's launch, stop on the last's)
        for (int i = 0; i < ng; i++) {
            bool seen = false;
            for (int j = 0; j < i && !seen; j++) seen = goal_batch_class(g[j]) == goal_batch_class(g[i]);
            classes += seen ? 0 : 1;
        }
        bool done[PLAN_BATCH_MAX] = {};
        int launched = 0;
        for (int i = 0; i < ng; i++) {
            if (done[i]) continue;
            GoalArgs grp[PLAN_BATCH_MAX];
            int k = 0;
            for (int j = i; j < ng; j++)
                if (!done[j] && goal_batch_class(g[j]) == goal_batch_class(g[i])) { grp[k++] = g[j]; done[j] = true; }
            LaunchEvents e;
            if (launched == 0) e.start = ev.start;
            if (++launched == classes) e.stop = ev.stop;
            if (launch_goal_batch(grp, k, st, e) != hipSuccess) { c0->err = std::string(fn) + ": goal batch launch failed (grid too large for the LDS?)"; return LSC_EHIP; }
        }
    }
    if (ns > 0) {
        LaunchEvents ev;
        if (c0->timing && timing_begin(c0, 4, &ev) != LSC_OK) return LSC_EHIP;
        HIPCHK(c0, launch_sfc_batch(s, ns, st, ev));
    }
    LaunchEvents ev;
    int workgroups = 0;                                // (a batch of empty shards launches nothing: events, recorded)
    for (int i = 0; i < n; i++) workgroups = std::max(workgroups, a[i].count);
    if (c0->timing && timing_begin(c0, 0, &ev, st, workgroups * n) != LSC_OK) return LSC_EHIP;      // (the batch launch's grid: largest swarm x swarms)
    const bool handover = hooks && general;            // (the plan launch carries both events unless the hand-over launch follows it)
    if (launch_plan_batch(a, n, smem, st, handover ? ev.first() : ev) != hipSuccess) { c0->err = std::string(fn) + ": launch failed (contexts of different planar / alternate-mode classes?)"; return LSC_EHIP; }
    if (handover) HIPCHK(c0, launch_general_batch(a, n, slots, st, ev.last()));
    for (int i = 0; i < n; i++) ctx[i]->last_general = handover ? 3 : 0;
    return LSC_OK;
}

int lsc_tick_device_fused_batch(lsc_ctx *const *ctx, int n, const float *const *d_state, const float *const *d_goal,
                                const float *const *d_traj_prev, const int *planner_seq, float *const *d_traj_next,
                                float *const *d_state_next, double *const *d_cost, int *const *d_status, int *const *d_iters,
                                void *hip_stream)
{
    if (!ctx || n < 1 || !ctx[0]) return LSC_EINVAL;
    lsc_ctx *c0 = ctx[0];
    if (n > PLAN_BATCH_MAX) { c0->err = "lsc_tick_device_fused_batch: at most " + std::to_string(PLAN_BATCH_MAX) + " swarms per launch"; return LSC_EINVAL; }
    if (!d_state || !d_goal || !d_traj_prev || !planner_seq || !d_traj_next || !d_state_next || !d_cost || !d_status || !d_iters) return LSC_EINVAL;
    for (int i = 0; i < n; i++)
        if (!ctx[i] || !d_state[i] || !d_goal[i] || !d_traj_prev[i] || !d_traj_next[i] || !d_state_next[i] || !d_cost[i] || !d_status[i] || !d_iters[i]) return LSC_EINVAL;
    return tick_batch("lsc_tick_device_fused_batch", ctx, n, d_state, d_goal, d_traj_prev, planner_seq, d_traj_next, d_state_next, d_cost,
                      d_status, d_iters, nullptr, (hipStream_t)hip_stream);
}

// The host inputs of one tick -> the context's device tables (state | goals | previous plans are one allocation), queued on `st`.
// `ce`: the context that reports errors (the first of a batch).
static int upload_inputs(lsc_ctx *c, lsc_ctx *ce, const float *state, const float *goal, const float *prev_traj, int planner_seq, hipStream_t st)
{
    const size_t N = c->N;
    c->last_host_seq = planner_seq;
    std::memcpy(c->swarm.h_in, state, sizeof(float) * 9 * N);
    if (goal) std::memcpy(c->swarm.h_in + 9 * N, goal, sizeof(float) * 3 * N);      // (null: a mission state is open, the tick reads its tables)
    std::memcpy(c->swarm.h_in + 12 * N, prev_traj, sizeof(float) * NV * N);
    HIPCHK(ce, hipMemcpyAsync(c->swarm.d_in, c->swarm.h_in, sizeof(float) * in_block_floats(N), hipMemcpyHostToDevice, st));
    return LSC_OK;
}

// Rows [first, first + count) of the downloaded results (h_out: cost | plans | status | iterations, table_rows rows each) -> the caller's
// arrays.  False when one of them was handed to the general kernel and never solved: an internal error, not a report.
static bool unpack_outputs(const lsc_ctx *c, size_t first, size_t count, float *out_traj, double *out_cost, int *out_status, int *out_iters)
{
    const size_t Np = (size_t)c->table_rows;
    const unsigned char *o = c->swarm.h_out;
    std::memcpy(out_cost, o + sizeof(double) * first, sizeof(double) * count);
    std::memcpy(out_traj, o + sizeof(double) * Np + sizeof(float) * NV * first, sizeof(float) * NV * count);
    const unsigned char *si = o + (sizeof(double) + sizeof(float) * NV) * Np;
    std::memcpy(out_status, si + sizeof(int) * first, sizeof(int) * count);
    if (out_iters) std::memcpy(out_iters, si + sizeof(int) * (Np + first), sizeof(int) * count);
    for (size_t q = 0; q < count; q++)
        if (out_status[q] == LSC_STATUS_GENERAL_K) return false;
    return true;
}

int lsc_replan_tick(lsc_ctx *c, const float *state, const float *goal, const float *prev_traj, int planner_seq,
                    float *out_traj, double *out_cost, int *out_status, int *out_iters, float *out_lsc_normal,
                    double *out_lsc_d, float *out_sfc)
{
    if (!c || !state || (!goal && !c->swarm.mission.open) || !prev_traj || !out_traj || !out_cost || !out_status) return LSC_EINVAL;
    if (c->N == 0) return LSC_ESTATE;
    const auto t_entry = std::chrono::steady_clock::now();
    if (int prc = planar_inputs_ok(c, state, prev_traj, planner_seq)) return prc;
    if (int orc = obstacles_tick_ok(c, "lsc_replan_tick")) return orc;
    if (int mrc = mission_tick_ok(c, "lsc_replan_tick")) return mrc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t N = c->N, cnt = c->count, first = c->first, nobs = N - 1 + c->swarm.obs.K;
    hipStream_t st = c->stream;
    int rc = upload_inputs(c, c, state, goal, prev_traj, planner_seq, st);
    if (rc) return rc;
    rc = plan_context(c, c->swarm.d_state, c->swarm.d_goal, c->swarm.d_prev, planner_seq, c->swarm.d_next, nullptr, c->swarm.d_cost, c->swarm.d_status, c->swarm.d_iters,
                      out_lsc_normal || out_lsc_d, state, prev_traj, st, "lsc_replan_tick", true);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->swarm.h_out, c->swarm.d_out, out_block_bytes(c->table_rows), hipMemcpyDeviceToHost, st));
    const bool dyn = c->swarm.obs.K > 0;
    if (out_lsc_normal) HIPCHK(c, hipMemcpyAsync(out_lsc_normal, dyn ? c->swarm.obs.d_onormal.get() : c->swarm.d_onormal.get(), sizeof(float) * 3 * M * nobs * cnt, hipMemcpyDeviceToHost, st));
    if (out_lsc_d) HIPCHK(c, hipMemcpyAsync(out_lsc_d, dyn ? c->swarm.obs.d_od.get() : c->swarm.d_od.get(), sizeof(double) * NC * M * nobs * cnt, hipMemcpyDeviceToHost, st));
    if (out_sfc) HIPCHK(c, hipMemcpyAsync(out_sfc, c->swarm.d_sfc + first * M * 6, sizeof(float) * M * 6 * cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (c->swarm.obs.upload_stream == st) c->swarm.obs.upload_in_flight = false;
    if (!unpack_outputs(c, first, cnt, out_traj, out_cost, out_status, out_iters)) {
        c->err = "internal: an agent was handed to the alternate-mode kernel, which did not run";
        return LSC_ESTATE;
    }
    c->next_has_all_rows = c->count == c->N;
    if (c->timing)
        c->host_tick_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count());
    return LSC_OK;
}

// Host-buffer form of the batched tick (what a C++ simulator flying several missions in lockstep calls): lsc_replan_tick's per-context
// checks and host work, one upload per context, ONE batched tick (tick_batch), one download per context, one synchronisation.  Everything
// runs on the first context's stream; the outputs are those of lsc_replan_tick on each context alone (no constraint dumps in this form).
int lsc_replan_tick_batch(lsc_ctx *const *ctx, int n, const float *const *state, const float *const *goal, const float *const *prev_traj,
                          const int *planner_seq, float *const *out_traj, double *const *out_cost, int *const *out_status,
                          int *const *out_iters)
{
    if (!ctx || n < 1 || !ctx[0]) return LSC_EINVAL;
    lsc_ctx *c0 = ctx[0];
    if (n > PLAN_BATCH_MAX) { c0->err = "lsc_replan_tick_batch: at most " + std::to_string(PLAN_BATCH_MAX) + " swarms per launch"; return LSC_EINVAL; }
    if (!state || !goal || !prev_traj || !planner_seq || !out_traj || !out_cost || !out_status) return LSC_EINVAL;
    for (int i = 0; i < n; i++)
        if (!ctx[i] || !state[i] || !goal[i] || !prev_traj[i] || !out_traj[i] || !out_cost[i] || !out_status[i]) return LSC_EINVAL;
    const auto t_entry = std::chrono::steady_clock::now();
    for (int i = 0; i < n; i++) {
        lsc_ctx *c = ctx[i];
        if (c->N == 0) { c0->err = "lsc_replan_tick_batch: context " + std::to_string(i) + " has no agents"; return LSC_ESTATE; }
        if (c->cfg.device != c0->cfg.device) { c0->err = "lsc_replan_tick_batch: context " + std::to_string(i) + " is on another device"; return LSC_EINVAL; }
        if (c->swarm.obs.K > 0) { c0->err = "lsc_replan_tick_batch: context " + std::to_string(i) + " has dynamic obstacles (lsc_set_obstacles: the batch ticks are not built for them)"; return LSC_EINVAL; }
        if (stage_in_use(c)) { c0->err = "lsc_replan_tick_batch: context " + std::to_string(i) + " has a mission state open or the right-hand goal rule set (lsc_mission_open / lsc_set_goal_rule: the batch ticks launch no goal stage)"; return LSC_EINVAL; }
        if (int prc = planar_inputs_ok(c, state[i], prev_traj[i], planner_seq[i])) {
            if (c != c0) c0->err = "lsc_replan_tick_batch: context " + std::to_string(i) + ": " + c->err;
            return prc;
        }
    }
    HIPCHK(c0, hipSetDevice(c0->cfg.device));
    hipStream_t st = c0->stream;
    const float *d_state[PLAN_BATCH_MAX], *d_goal[PLAN_BATCH_MAX], *d_prev[PLAN_BATCH_MAX];
    float *d_next[PLAN_BATCH_MAX];
    double *d_cost[PLAN_BATCH_MAX];
    int *d_status[PLAN_BATCH_MAX], *d_iters[PLAN_BATCH_MAX], hint[PLAN_BATCH_MAX];
    for (int i = 0; i < n; i++) {
        lsc_ctx *c = ctx[i];
        if (c->stream != st) HIPCHK(c0, hipStreamSynchronize(c->stream));     // (nothing of this context may still be in flight elsewhere)
        if (int urc = upload_inputs(c, c0, state[i], goal[i], prev_traj[i], planner_seq[i], st)) return urc;
        hint[i] = host_disturbance_hint(c, state[i], prev_traj[i], planner_seq[i]);
        d_state[i] = c->swarm.d_state; d_goal[i] = c->swarm.d_goal; d_prev[i] = c->swarm.d_prev;
        d_next[i] = c->swarm.d_next; d_cost[i] = c->swarm.d_cost; d_status[i] = c->swarm.d_status; d_iters[i] = c->swarm.d_iters;
    }
    int rc = tick_batch("lsc_replan_tick_batch", ctx, n, d_state, d_goal, d_prev, planner_seq, d_next, nullptr, d_cost, d_status, d_iters, hint, st);
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        lsc_ctx *c = ctx[i];
        HIPCHK(c0, hipMemcpyAsync(c->swarm.h_out, c->swarm.d_out, out_block_bytes(c->table_rows), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c0, hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        lsc_ctx *c = ctx[i];
        if (!unpack_outputs(c, c->first, c->count, out_traj[i], out_cost[i], out_status[i], out_iters ? out_iters[i] : nullptr)) {
            c0->err = "internal: an agent of context " + std::to_string(i) + " was handed to the alternate-mode kernel, which did not run";
            return LSC_ESTATE;
        }
        c->next_has_all_rows = c->count == c->N;
    }
    if (c0->timing)
        c0->host_tick_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count());
    return LSC_OK;
}

// ---------------------------------------------------------------------------------------------------
// Agent-sharded multi-GPU.  The reference hands every agent every other agent's previous trajectory in
// MultiSyncSimulator::update (src/multi_sync_simulator.cpp:297-303); with the swarm partitioned over ranks that
// hand-over is the one exchange of a tick: an in-place RCCL all-gather of the freshly planned rows.
// ---------------------------------------------------------------------------------------------------
int lsc_comm_unique_id(unsigned char id[LSC_COMM_ID_BYTES])
{
    static_assert(LSC_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
    const RcclApi *api = rccl_api();
    if (!api || !id) return LSC_ECOMM;
    ncclUniqueId u;
    if (api->GetUniqueId(&u) != ncclSuccess) return LSC_ECOMM;
    std::memcpy(id, u.internal, LSC_COMM_ID_BYTES);
    return LSC_OK;
}

int lsc_comm_init(lsc_ctx *c, int world_size, int rank, const unsigned char id[LSC_COMM_ID_BYTES])
{
    if (!c || world_size < 1 || rank < 0 || rank >= world_size || !id) return LSC_EINVAL;
    if (c->N != 0) { c->err = "lsc_comm_init must precede lsc_set_agents (the tables are padded to the world size)"; return LSC_ESTATE; }
    if (c->comm) { c->err = "lsc_comm_init: communicator already initialised"; return LSC_ESTATE; }
    const RcclApi *api = rccl_api();
    if (!api) { c->err = "librccl.so could not be loaded"; return LSC_ECOMM; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    ncclUniqueId u;
    std::memcpy(u.internal, id, LSC_COMM_ID_BYTES);
    NCCLCHK(c, api, api->CommInitRank(&c->comm, world_size, u, rank));
    c->world = world_size; c->rank = rank;
    return LSC_OK;
}

int lsc_comm_info(const lsc_ctx *c, int *world_size, int *rank, int *shard_rows, int *table_rows)
{
    if (!c) return LSC_EINVAL;
    if (world_size) *world_size = c->world;
    if (rank) *rank = c->rank;
    if (shard_rows) *shard_rows = c->shard_rows;
    if (table_rows) *table_rows = c->table_rows;
    return LSC_OK;
}

// in-place all-gather of `rows_elems` elements per agent row of a table padded to table_rows rows
static int exchange_rows(lsc_ctx *c, const RcclApi *api, void *table, size_t row_bytes, hipStream_t st)
{
    const size_t cnt = (size_t)c->shard_rows * row_bytes;
    NCCLCHK(c, api, api->AllGather(static_cast<unsigned char *>(table) + (size_t)c->rank * cnt, table, cnt, ncclUint8, c->comm, st));
    return LSC_OK;
}

int lsc_tick_device_sharded(lsc_ctx *c, float *d_state, const float *d_goal, const float *d_traj_prev, int planner_seq,
                            float *d_traj_next, double *d_cost, int *d_status, int *d_iters, void *hip_stream)
{
    if (!c || !d_state) return LSC_EINVAL;
    if (!c->comm) { c->err = "lsc_tick_device_sharded: lsc_comm_init was not called"; return LSC_ESTATE; }
    const RcclApi *api = rccl_api();
    hipStream_t st = (hipStream_t)hip_stream;
    int rc = lsc_tick_device(c, d_state, d_goal, d_traj_prev, planner_seq, d_traj_next, d_cost, d_status, d_iters, hip_stream);
    if (rc) return rc;
    hipEvent_t e1 = nullptr;
    if (c->timing && timing_begin_recorded(c, 2, st, &e1) != LSC_OK) return LSC_EHIP;
    rc = exchange_rows(c, api, d_traj_next, sizeof(float) * NV, st);
    if (rc) return rc;
    if (c->timing) HIPCHK(c, hipEventRecord(e1, st));
    // MultiSyncSimulator::update of the next tick: every rank needs every agent's ideal state
    HIPCHK(c, launch_propagate(d_traj_next, d_state, c->N, c->cfg.dt, st));
    return LSC_OK;
}

int lsc_replan_tick_all(lsc_ctx *c, const float *state, const float *goal, const float *prev_traj, int planner_seq,
                        float *out_traj, double *out_cost, int *out_status, int *out_iters, float *out_goal)
{
    if (!c || !state || !goal || !prev_traj || !out_traj || !out_cost || !out_status) return LSC_EINVAL;
    if (c->N == 0) return LSC_ESTATE;
    if (!c->comm) { c->err = "lsc_replan_tick_all: lsc_comm_init was not called"; return LSC_ESTATE; }
    if (int prc = planar_inputs_ok(c, state, prev_traj, planner_seq)) return prc;
    if (int orc = obstacles_tick_ok(c, "lsc_replan_tick_all")) return orc;
    if (int mrc = mission_tick_ok(c, "lsc_replan_tick_all")) return mrc;
    const RcclApi *api = rccl_api();
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t N = c->N, Np = (size_t)c->table_rows;
    hipStream_t st = c->stream;
    int rc = upload_inputs(c, c, state, goal, prev_traj, planner_seq, st);
    if (rc) return rc;
    rc = plan_context(c, c->swarm.d_state, c->swarm.d_goal, c->swarm.d_prev, planner_seq, c->swarm.d_next, nullptr, c->swarm.d_cost, c->swarm.d_status, c->swarm.d_iters, false, state,
                      prev_traj, st, "lsc_replan_tick_all", true);
    if (rc) return rc;
    hipEvent_t e1 = nullptr;
    if (c->timing && timing_begin_recorded(c, 2, st, &e1) != LSC_OK) return LSC_EHIP;
    NCCLCHK(c, api, api->GroupStart());
    {   // the group is closed on every path: a communicator left inside an open group is unusable
        rc = exchange_rows(c, api, c->swarm.d_next, sizeof(float) * NV, st);
        if (!rc) rc = exchange_rows(c, api, c->swarm.d_cost, sizeof(double), st);
        if (!rc) rc = exchange_rows(c, api, c->swarm.d_status, sizeof(int), st);
        if (!rc) rc = exchange_rows(c, api, c->swarm.d_iters, sizeof(int), st);
        if (!rc) rc = exchange_rows(c, api, c->swarm.d_goal_cur, sizeof(float) * 3, st);
        const ncclResult_t ge = api->GroupEnd();
        if (rc) return rc;
        if (ge != ncclSuccess) { c->err = std::string("ncclGroupEnd: ") + api->GetErrorString(ge); return LSC_ECOMM; }
    }
    if (c->timing) HIPCHK(c, hipEventRecord(e1, st));
    HIPCHK(c, hipMemcpyAsync(c->swarm.h_out, c->swarm.d_out, out_block_bytes(Np), hipMemcpyDeviceToHost, st));
    if (out_goal) HIPCHK(c, hipMemcpyAsync(out_goal, c->swarm.d_goal_cur, sizeof(float) * 3 * N, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (!unpack_outputs(c, 0, N, out_traj, out_cost, out_status, out_iters)) {
        c->err = "internal: an agent was handed to the alternate-mode kernel, which did not run";
        return LSC_ESTATE;
    }
    c->next_has_all_rows = true;
    return LSC_OK;
}

// MultiSyncSimulator::savePlanningResult's agent-agent accounting (src/multi_sync_simulator.cpp:446-503) for the plans of the last
// host-buffer tick.  Sample time t falls into segment m = (int)(t / dt) at local parameter t / dt - m (getStateFromControlPoints,
// include/polynomial.hpp); the Bernstein weights are computed here, on the host, with the reference's own expression
// (nChoosek * pow(t, i) * pow(1 - t, n - i)) so that the device only repeats its multiply-adds.
int lsc_safety_ratio(lsc_ctx *c, const double *times, int n_times, double *out_ratio, int *out_partner, double *out_min)
{
    if (!c || !times || n_times < 1 || n_times > 64 || !out_min) return LSC_EINVAL;
    if (c->N < 1 || c->last_host_seq < 1) { if (c) c->err = "lsc_safety_ratio: no host-buffer tick was planned yet"; return LSC_ESTATE; }
    if (!c->next_has_all_rows) {
        // the partners of every pair are read from the context's own table: a sharded lsc_replan_tick leaves the other ranks' rows stale
        c->err = "lsc_safety_ratio: the last tick planned a shard only (use lsc_replan_tick_all, or a context that owns the whole swarm)";
        return LSC_ESTATE;
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int N = c->N, cnt = c->count;
    std::vector<double> w((size_t)n_times * NC);
    std::vector<int> seg(n_times);
    auto choose = [](int n, int k) { if (k * 2 > n) k = n - k; if (k == 0) return 1; int r = n; for (int i = 2; i <= k; i++) { r *= (n - i + 1); r /= i; } return r; };
    for (int ti = 0; ti < n_times; ti++) {
        const double t = times[ti];
        int m = (int)(t / c->cfg.dt);
        if (m == M && t < M * c->cfg.dt + 1e-9) m = M - 1;
        else if (m >= M || t < 0.0) { c->err = "lsc_safety_ratio: sample time outside the planning horizon"; return LSC_EINVAL; }
        seg[ti] = m;
        const double tl = t / c->cfg.dt - m;
        for (int i = 0; i < NC; i++) w[(size_t)ti * NC + i] = choose(DEG, i) * std::pow(tl, i) * std::pow(1 - tl, DEG - i);
    }
    {
        // (sized for THIS call's shard and sample count: lsc_set_shard may have enlarged the shard since the last call, and the
        // carve-up below depends on both)
        const size_t bytes = (size_t)n_times * (sizeof(double) * NC + sizeof(int) * 2 + sizeof(float) * 3 * (size_t)N + (sizeof(double) + sizeof(int)) * (size_t)cnt) + 64;
        if (c->swarm.d_safety.size() < bytes) HIPCHK(c, c->swarm.d_safety.alloc(bytes));
    }
    // carve-up: ratios, weights, global minimum | positions | partners, segments
    double *d_ratio = reinterpret_cast<double *>(c->swarm.d_safety.get());
    double *d_w = d_ratio + (size_t)n_times * cnt;
    double *d_min = d_w + (size_t)n_times * NC;
    float *d_pos = reinterpret_cast<float *>(d_min + 1);
    int *d_partner = reinterpret_cast<int *>(d_pos + (size_t)n_times * 3 * N);
    int *d_seg = d_partner + (size_t)n_times * cnt;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(d_w, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_seg, seg.data(), sizeof(int) * seg.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_safety(c->swarm.d_next, d_w, d_seg, n_times, N, c->first, cnt, c->swarm.d_radius, c->swarm.d_downwash, d_pos, d_ratio, d_partner, st));
    std::vector<double> ratio((size_t)n_times * cnt);
    std::vector<int> partner((size_t)n_times * cnt);
    HIPCHK(c, hipMemcpyAsync(ratio.data(), d_ratio, sizeof(double) * ratio.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(partner.data(), d_partner, sizeof(int) * partner.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    double mn = 1e300;
    for (double r : ratio) mn = r < mn ? r : mn;
    if (c->comm) {                                  // one all-reduce brings the swarm's minimum to every rank
        const RcclApi *api = rccl_api();
        HIPCHK(c, hipMemcpyAsync(d_min, &mn, sizeof(double), hipMemcpyHostToDevice, st));
        NCCLCHK(c, api, api->AllReduce(d_min, d_min, 1, ncclDouble, ncclMin, c->comm, st));
        HIPCHK(c, hipMemcpyAsync(&mn, d_min, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    if (out_ratio) std::memcpy(out_ratio, ratio.data(), sizeof(double) * ratio.size());
    if (out_partner) std::memcpy(out_partner, partner.data(), sizeof(int) * partner.size());
    *out_min = mn;
    return LSC_OK;
}

// ---- K ticks per call with the mission's bookkeeping (include/lsc_planner_amd.h; kernel: lsc_flight.hip, statements: lsc_flight.hpp) ----

int lsc_flight_weights(double dt, const double *times, int n_times, double *w5, double *w4, double *w3, int *seg)
{
    if (!times || n_times < 1 || n_times > FLIGHT_MAX_TIMES || !(dt > 0.0)) return LSC_EINVAL;
    for (int ti = 0; ti < n_times; ti++) {
        const int m = flight_segment(times[ti], dt);
        if (m < 0) return LSC_EINVAL;
        const double tl = flight_local_time(times[ti], dt, m);
        if (seg) seg[ti] = m;
        if (w5) flight_bernstein(DEG, tl, w5 + (size_t)ti * 6);
        if (w4) flight_bernstein(DEG - 1, tl, w4 + (size_t)ti * 5);
        if (w3) flight_bernstein(DEG - 2, tl, w3 + (size_t)ti * 4);
    }
    return LSC_OK;
}

size_t lsc_flight_row_bytes(int N, int n_times, int what)
{
    if (N < 1 || n_times < 1 || n_times > FLIGHT_MAX_TIMES || what < 0 || what > 7) return 0;
    return flight_layout(N, n_times, what).row_bytes;
}

// what a context must be for lsc_flight_begin / lsc_fly_device: it plans the whole swarm alone and keeps no per-tick host-side diagnostics
static int flight_context_ok(lsc_ctx *c, const char *fn)
{
    const char *why = nullptr;
    if (c->comm) why = "the context has a communicator (the closed loop flies one whole swarm on one device)";
    else if (c->first != 0 || c->count != c->N) why = "the context's shard is not the whole swarm";
    else if (c->goal_path_cap > 0) why = "the goal trace is on";
    else if (c->goal_profiling) why = "goal profiling is on";
    else if (c->swarm.obs.K > 0 && !c->swarm.obs.d_models) why = "the context has dynamic obstacles (lsc_set_obstacles: the flight loop does not move them)";
    if (!why) return LSC_OK;
    c->err = std::string(fn) + ": " + why;
    return LSC_EINVAL;
}

int lsc_flight_end(lsc_ctx *c)
{
    if (!c) return LSC_EINVAL;
    SwarmMem &s = c->swarm;
    if (s.d_flight) {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        if (s.flight_flown > 0) HIPCHK(c, hipStreamSynchronize(s.flight_stream));     // the record launches still write to it
    }
    s.d_flight.reset();
    s.d_track.reset();
    s.flight_capacity = s.flight_times = s.flight_what = s.flight_flown = 0;
    s.flight_row_bytes = s.track_row_bytes = 0;
    s.track_K = 0;
    s.flight_stream = nullptr;
    return LSC_OK;
}

int lsc_flight_reset(lsc_ctx *c)
{
    if (!c) return LSC_EINVAL;
    SwarmMem &s = c->swarm;
    if (!s.d_flight) { c->err = "lsc_flight_reset: no flight log is open"; return LSC_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (s.flight_flown > 0) HIPCHK(c, hipStreamSynchronize(s.flight_stream));
    HIPCHK(c, launch_flight_init(s.d_flight.get() + FLIGHT_HEADER_BYTES, s.flight_row_bytes, s.flight_capacity, c->stream));
    if (s.d_track) HIPCHK(c, launch_obstacle_track_init(s.d_track.get(), s.track_row_bytes, s.flight_capacity, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));     // (the next flight may be on any stream)
    s.flight_flown = 0;
    return LSC_OK;
}

int lsc_flight_begin(lsc_ctx *c, const lsc_flight_config *cfg)
{
    if (!c || !cfg) return LSC_EINVAL;
    if (c->N < 1) { c->err = "lsc_flight_begin: lsc_set_agents comes first"; return LSC_ESTATE; }
    int rc = flight_context_ok(c, "lsc_flight_begin");
    if (rc) return rc;
    if (cfg->capacity_ticks < 1 || cfg->what < 0 || cfg->what > 7) { c->err = "lsc_flight_begin: capacity_ticks below 1 or unknown bits in what"; return LSC_EINVAL; }
    if (cfg->n_times < 1 || cfg->n_times > FLIGHT_MAX_TIMES) { c->err = "lsc_flight_begin: n_times outside 1..64"; return LSC_EINVAL; }
    std::vector<unsigned char> head(FLIGHT_HEADER_BYTES, 0);
    if (lsc_flight_weights(c->cfg.dt, cfg->times, cfg->n_times, reinterpret_cast<double *>(head.data() + FLIGHT_W5), reinterpret_cast<double *>(head.data() + FLIGHT_W4),
                           reinterpret_cast<double *>(head.data() + FLIGHT_W3), reinterpret_cast<int *>(head.data() + FLIGHT_SEG)) != LSC_OK) {
        c->err = "lsc_flight_begin: sample time outside the planning horizon";
        return LSC_EINVAL;
    }
    rc = lsc_flight_end(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    SwarmMem &s = c->swarm;
    const size_t row_bytes = flight_layout(c->N, cfg->n_times, cfg->what).row_bytes;
    HIPCHK(c, s.d_flight.alloc(FLIGHT_HEADER_BYTES + row_bytes * (size_t)cfg->capacity_ticks));
    s.flight_capacity = cfg->capacity_ticks; s.flight_times = cfg->n_times; s.flight_what = cfg->what; s.flight_row_bytes = row_bytes;
    if (s.obs.d_models) {                            // the obstacle track, beside the log
        s.track_K = s.obs.K;
        s.track_row_bytes = obstacle_track_layout(c->N, cfg->n_times, s.track_K).row_bytes;
        HIPCHK(c, s.d_track.alloc(s.track_row_bytes * (size_t)cfg->capacity_ticks));
    }
    HIPCHK(c, hipMemcpyAsync(s.d_flight.get(), head.data(), FLIGHT_HEADER_BYTES, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));     // (`head` is pageable and leaves scope)
    return lsc_flight_reset(c);
}

int lsc_fly_device(lsc_ctx *c, float *const d_state[2], const float *d_goal, float *const d_traj[2], int first_planner_seq, int n_ticks,
                   double *d_cost, int *d_status, int *d_iters, void *hip_stream)
{
    if (!c || !d_state || !d_traj || !d_state[0] || !d_state[1] || !d_traj[0] || !d_traj[1] || (!d_goal && !c->swarm.mission.open) || !d_cost || !d_status || !d_iters || n_ticks < 0)
        return LSC_EINVAL;
    if (c->N == 0) return LSC_ESTATE;
    int rc = flight_context_ok(c, "lsc_fly_device");
    if (rc) return rc;
    rc = mission_tick_ok(c, "lsc_fly_device");
    if (rc) return rc;
    if (d_state[0] == d_state[1] || d_traj[0] == d_traj[1]) { c->err = "lsc_fly_device: the two state buffers and the two trajectory tables must be different buffers"; return LSC_EINVAL; }
    SwarmMem &s = c->swarm;
    const bool log = (bool)s.d_flight;
    if (log && s.flight_flown + n_ticks > s.flight_capacity) {
        c->err = "lsc_fly_device: " + std::to_string(n_ticks) + " ticks do not fit the flight log (" + std::to_string(s.flight_flown) + " of " +
                 std::to_string(s.flight_capacity) + " rows are taken; lsc_flight_read, then lsc_flight_reset)";
        return LSC_ESTATE;
    }
    const ObsMem &ob = s.obs;
    if (log && s.track_K != (ob.d_models ? ob.K : 0)) {
        c->err = "lsc_fly_device: the open flight log's obstacle track is for " + std::to_string(s.track_K) + " obstacles and the context moves " +
                 std::to_string(ob.d_models ? ob.K : 0) + " (lsc_flight_begin comes after lsc_obstacle_motion)";
        return LSC_ESTATE;
    }
    if (ob.d_models) {                               // (every tick's time, in front of the first launch)
        rc = obstacles_context_ok(c, "lsc_fly_device", ob.reset_served);
        if (!rc) rc = obstacle_clock_ok(c, "lsc_fly_device", n_ticks);
        if (rc) return rc;
    }
    if (n_ticks == 0) return LSC_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    FlightArgs f = {};
    ObstacleRecordArgs tr = {};
    if (log) {
        unsigned char *h = s.d_flight.get();
        f.N = c->N; f.n_times = s.flight_times; f.what = s.flight_what;
        f.agents_per_block = flight_agents_per_block(c->N, s.flight_what);
        f.dt_inv = (float)std::pow(c->cfg.dt, -1);
        f.goal_threshold = c->cfg.goal_threshold;
        // (the record's goal tests are on the DESIRED goals: the mission state's table as the tick's stage left it, else the caller's)
        f.goal = s.mission.open ? s.mission.d_tables.get() : d_goal; f.cost = d_cost; f.status = d_status;
        f.radius = s.d_radius; f.downwash = s.d_downwash;
        f.w5 = reinterpret_cast<const double *>(h + FLIGHT_W5); f.w4 = reinterpret_cast<const double *>(h + FLIGHT_W4);
        f.w3 = reinterpret_cast<const double *>(h + FLIGHT_W3); f.seg = reinterpret_cast<const int *>(h + FLIGHT_SEG);
        s.flight_stream = st;
        if (s.d_track) {
            tr.N = c->N; tr.n_times = s.flight_times; tr.K = s.track_K;
            tr.radius = s.d_radius; tr.w5 = f.w5; tr.seg = f.seg; tr.obs = ob.d_block; tr.pos_vel = ob.d_pos_vel; tr.pos_f64 = ob.d_pos_f64;
        }
    }
    for (int j = 0; j < n_ticks; j++) {
        const int seq = first_planner_seq + j;
        rc = plan_context(c, d_state[j & 1], d_goal, d_traj[j & 1], seq, d_traj[(j + 1) & 1], d_state[(j + 1) & 1], d_cost, d_status, d_iters, false,
                          nullptr, nullptr, st, "lsc_fly_device");
        if (rc) return rc;
        if (!log) continue;
        f.planner_seq = seq; f.state = d_state[j & 1]; f.traj_prev = d_traj[j & 1]; f.traj_next = d_traj[(j + 1) & 1];
        f.row = s.d_flight.get() + FLIGHT_HEADER_BYTES + s.flight_row_bytes * (size_t)s.flight_flown;
        LaunchEvents ev;
        if (c->timing && timing_begin(c, 6, &ev) != LSC_OK) return LSC_EHIP;
        HIPCHK(c, launch_flight(f, st, ev));
        if (s.d_track) {
            tr.traj_next = f.traj_next;
            tr.row = s.d_track.get() + s.track_row_bytes * (size_t)s.flight_flown;
            HIPCHK(c, launch_obstacle_record(tr, st));
        }
        s.flight_flown++;
    }
    return LSC_OK;
}

int lsc_flight_read(lsc_ctx *c, int first_tick, int n_ticks, lsc_flight_tick *summary, float *samples, double *ratio, int *partner,
                    double *cost, int *status, float *end)
{
    static_assert(sizeof(lsc_flight_tick) == FLIGHT_SUMMARY_BYTES && offsetof(lsc_flight_tick, min_ratio) == 40, "the summary the record kernel writes");
    if (!c) return LSC_EINVAL;
    SwarmMem &s = c->swarm;
    if (!s.d_flight) { c->err = "lsc_flight_read: no flight log is open"; return LSC_ESTATE; }
    if (first_tick < 0 || n_ticks < 0 || first_tick + n_ticks > s.flight_flown) {
        c->err = "lsc_flight_read: rows " + std::to_string(first_tick) + ".." + std::to_string(first_tick + n_ticks - 1) + " were not all flown (" +
                 std::to_string(s.flight_flown) + " rows are)";
        return LSC_EINVAL;
    }
    if ((samples && !(s.flight_what & FLIGHT_SAMPLES)) || ((ratio || partner) && !(s.flight_what & FLIGHT_SAFETY)) ||
        ((cost || status || end) && !(s.flight_what & FLIGHT_AGENTS))) {
        c->err = "lsc_flight_read: a part was asked for that the log does not record";
        return LSC_EINVAL;
    }
    if (n_ticks == 0) return LSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(s.flight_stream));
    const size_t rb = s.flight_row_bytes, N = (size_t)c->N, TN = (size_t)s.flight_times * N;
    const FlightLayout L = flight_layout(c->N, s.flight_times, s.flight_what);
    std::vector<unsigned char> h(rb * (size_t)n_ticks);
    HIPCHK(c, hipMemcpy(h.data(), s.d_flight.get() + FLIGHT_HEADER_BYTES + rb * (size_t)first_tick, h.size(), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < (size_t)n_ticks; j++) {
        const unsigned char *r = h.data() + rb * j;
        if (summary) std::memcpy(summary + j, r, FLIGHT_SUMMARY_BYTES);
        if (samples) std::memcpy(samples + j * 9 * TN, r + L.samples, 4 * 9 * TN);
        if (ratio) std::memcpy(ratio + j * TN, r + L.ratio, 8 * TN);
        if (partner) std::memcpy(partner + j * TN, r + L.partner, 4 * TN);
        if (cost) std::memcpy(cost + j * N, r + L.cost, 8 * N);
        if (status) std::memcpy(status + j * N, r + L.status, 4 * N);
        if (end) std::memcpy(end + j * 3 * N, r + L.end, 4 * 3 * N);
    }
    return LSC_OK;
}

int lsc_obstacle_positions_read(lsc_ctx *c, double *pos)
{
    if (!c || !pos) return LSC_EINVAL;
    const ObsMem &ob = c->swarm.obs;
    if (!ob.d_models) { c->err = "lsc_obstacle_positions_read: the context has no motion models (lsc_obstacle_motion)"; return LSC_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(pos, ob.d_pos_f64.get(), sizeof(double) * 3 * (size_t)ob.K, hipMemcpyDeviceToHost));
    return LSC_OK;
}

int lsc_flight_obstacle_positions_read(lsc_ctx *c, int first_tick, int n_ticks, double *pos)
{
    if (!c || !pos) return LSC_EINVAL;
    SwarmMem &s = c->swarm;
    if (!s.d_flight || !s.d_track) { c->err = "lsc_flight_obstacle_positions_read: no flight log with an obstacle track is open (lsc_flight_begin on a context with motion models)"; return LSC_ESTATE; }
    if (first_tick < 0 || n_ticks < 0 || first_tick + n_ticks > s.flight_flown) {
        c->err = "lsc_flight_obstacle_positions_read: rows " + std::to_string(first_tick) + ".." + std::to_string(first_tick + n_ticks - 1) + " were not all flown (" +
                 std::to_string(s.flight_flown) + " rows are)";
        return LSC_EINVAL;
    }
    if (n_ticks == 0) return LSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(s.flight_stream));
    const size_t rb = s.track_row_bytes, K3 = 3 * (size_t)s.track_K;
    const ObstacleTrackLayout L = obstacle_track_layout(c->N, s.flight_times, s.track_K);
    std::vector<unsigned char> h(rb * (size_t)n_ticks);
    HIPCHK(c, hipMemcpy(h.data(), s.d_track.get() + rb * (size_t)first_tick, h.size(), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < (size_t)n_ticks; j++) std::memcpy(pos + j * K3, h.data() + rb * j + L.positions, 8 * K3);
    return LSC_OK;
}

int lsc_flight_obstacles_read(lsc_ctx *c, int first_tick, int n_ticks, double *min_ratio, int *below_one, float *pos_vel, double *ratio, int *partner)
{
    if (!c) return LSC_EINVAL;
    SwarmMem &s = c->swarm;
    if (!s.d_flight || !s.d_track) { c->err = "lsc_flight_obstacles_read: no flight log with an obstacle track is open (lsc_flight_begin on a context with motion models)"; return LSC_ESTATE; }
    if (first_tick < 0 || n_ticks < 0 || first_tick + n_ticks > s.flight_flown) {
        c->err = "lsc_flight_obstacles_read: rows " + std::to_string(first_tick) + ".." + std::to_string(first_tick + n_ticks - 1) + " were not all flown (" +
                 std::to_string(s.flight_flown) + " rows are)";
        return LSC_EINVAL;
    }
    if (n_ticks == 0) return LSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(s.flight_stream));
    const size_t rb = s.track_row_bytes, TN = (size_t)s.flight_times * (size_t)c->N, K6 = 6 * (size_t)s.track_K;
    const ObstacleTrackLayout L = obstacle_track_layout(c->N, s.flight_times, s.track_K);
    std::vector<unsigned char> h(rb * (size_t)n_ticks);
    HIPCHK(c, hipMemcpy(h.data(), s.d_track.get() + rb * (size_t)first_tick, h.size(), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < (size_t)n_ticks; j++) {
        const unsigned char *r = h.data() + rb * j;
        if (min_ratio) std::memcpy(min_ratio + j, r, 8);
        if (below_one) std::memcpy(below_one + j, r + 8, 4);
        if (pos_vel) std::memcpy(pos_vel + j * K6, r + L.states, 4 * K6);
        if (ratio) std::memcpy(ratio + j * TN, r + L.ratio, 8 * TN);
        if (partner) std::memcpy(partner + j * TN, r + L.partner, 4 * TN);
    }
    return LSC_OK;
}

int lsc_mission_open(lsc_ctx *c, const float *start, const float *goal)
{
    if (!c || !start || !goal) return LSC_EINVAL;
    if (c->N < 1) { c->err = "lsc_mission_open: lsc_set_agents comes first"; return LSC_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());                  // (ticks in flight may still read the tables being replaced)
    const size_t n3 = 3 * (size_t)c->N;
    std::vector<float> h(4 * n3);
    std::memcpy(h.data(), goal, sizeof(float) * n3);            // desired
    std::memcpy(h.data() + n3, start, sizeof(float) * n3);      // start
    std::memcpy(h.data() + 2 * n3, start, sizeof(float) * n3);  // the mission's start
    std::memcpy(h.data() + 3 * n3, goal, sizeof(float) * n3);   // the mission's goal
    MissionMem ms;
    HIPCHK(c, ms.d_tables.upload(h.data(), h.size()));
    HIPCHK(c, ms.d_legs.alloc_zero((size_t)c->N));
    ms.open = true;
    c->swarm.mission = std::move(ms);
    if (int rc = mission_tick_ok(c, "lsc_mission_open")) { c->swarm.mission = MissionMem{}; return rc; }
    return LSC_OK;
}

int lsc_mission_set_state(lsc_ctx *c, int planner_state)
{
    if (!c) return LSC_EINVAL;
    if (!c->swarm.mission.open) { c->err = "lsc_mission_set_state: no mission state is open"; return LSC_ESTATE; }
    if (planner_state != LSC_MISSION_GOTO && planner_state != LSC_MISSION_PATROL && planner_state != LSC_MISSION_GOBACK) {
        c->err = "lsc_mission_set_state: unknown planner state";
        return LSC_EINVAL;
    }
    c->swarm.mission.planner_state = planner_state;
    return LSC_OK;
}

int lsc_mission_read(lsc_ctx *c, float *desired, float *start, int *legs)
{
    if (!c) return LSC_EINVAL;
    const MissionMem &ms = c->swarm.mission;
    if (!ms.open) { c->err = "lsc_mission_read: no mission state is open"; return LSC_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());
    const size_t n3 = 3 * (size_t)c->N;
    if (desired) HIPCHK(c, hipMemcpy(desired, ms.d_tables.get(), sizeof(float) * n3, hipMemcpyDeviceToHost));
    if (start) HIPCHK(c, hipMemcpy(start, ms.d_tables.get() + n3, sizeof(float) * n3, hipMemcpyDeviceToHost));
    if (legs) HIPCHK(c, hipMemcpy(legs, ms.d_legs.get(), sizeof(int) * (size_t)c->N, hipMemcpyDeviceToHost));
    return LSC_OK;
}

int lsc_mission_close(lsc_ctx *c)
{
    if (!c) return LSC_EINVAL;
    if (!c->swarm.mission.open && !c->swarm.mission.d_rule_goal) return LSC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());                  // (ticks in flight may still read the tables)
    c->swarm.mission = MissionMem{};                    // (the rule's table goes too: the next tick that flies the rule allocates it)
    return LSC_OK;
}

int lsc_set_goal_rule(lsc_ctx *c, int rule, int seq_threshold, double velocity_threshold)
{
    if (!c) return LSC_EINVAL;
    if (rule != LSC_GOAL_RULE_CONFIG && rule != LSC_GOAL_RULE_RIGHT_HAND) { c->err = "lsc_set_goal_rule: unknown rule"; return LSC_EINVAL; }
    if (rule == LSC_GOAL_RULE_RIGHT_HAND) {
        if (c->cfg.goal_mode != 0) { c->err = "lsc_set_goal_rule: right_hand replaces the static rule (the tick behind the stage plans as goal_mode 0): create the context with goal_mode 0"; return LSC_EINVAL; }
        if (seq_threshold < 0 || !(velocity_threshold >= 0.0)) { c->err = "lsc_set_goal_rule: negative threshold"; return LSC_EINVAL; }
        const int before = c->goal_rule;
        c->goal_rule = rule;
        if (int rc = mission_tick_ok(c, "lsc_set_goal_rule")) { c->goal_rule = before; return rc; }
        c->deadlock_seq_threshold = seq_threshold; c->deadlock_velocity_threshold = velocity_threshold;
    }
    c->goal_rule = rule;
    return LSC_OK;
}

int lsc_propagate_device(lsc_ctx *c, const float *d_traj, float *d_state, void *hip_stream)
{
    if (!c || !d_traj || !d_state) return LSC_EINVAL;
    if (c->N == 0) return LSC_ESTATE;
    HIPCHK(c, launch_propagate(d_traj, d_state, c->N, c->cfg.dt, (hipStream_t)hip_stream));
    return LSC_OK;
}

static int sweep_device(lsc_ctx *c, const float *d_state, const float *d_traj_prev, int planner_seq, float *d_normal, double *d_d,
                        float *d_d32, void *hip_stream)
{
    if (!c || !d_state || !d_traj_prev || !d_normal || (!d_d && !d_d32)) return LSC_EINVAL;
    if (c->N < 2) return LSC_ESTATE;
    SweepArgs a;
    a.N = c->N; a.first = c->first; a.count = c->count; a.planner_seq = planner_seq; a.dtf = (float)c->cfg.dt;
    a.state = d_state; a.traj_prev = d_traj_prev;
    a.radius = c->swarm.d_radius; a.radius_obs = c->swarm.d_radius_obs; a.downwash = c->swarm.d_downwash; a.downwash_obs = c->swarm.d_downwash_obs;
    a.out_normal = d_normal; a.out_d = d_d; a.out_d32 = d_d32;
    hipStream_t st = (hipStream_t)hip_stream;
    LaunchEvents ev;
    if (c->timing && timing_begin(c, 1, &ev) != LSC_OK) return LSC_EHIP;
    HIPCHK(c, launch_sweep(a, st, ev));
    return LSC_OK;
}

int lsc_sweep_device(lsc_ctx *c, const float *d_state, const float *d_traj_prev, int planner_seq, float *d_normal,
                     double *d_d, void *hip_stream)
{
    return sweep_device(c, d_state, d_traj_prev, planner_seq, d_normal, d_d, nullptr, hip_stream);
}

int lsc_sweep_device_f32(lsc_ctx *c, const float *d_state, const float *d_traj_prev, int planner_seq, float *d_normal,
                         float *d_d32, void *hip_stream)
{
    return sweep_device(c, d_state, d_traj_prev, planner_seq, d_normal, nullptr, d_d32, hip_stream);
}

int lsc_gjk_batch(lsc_ctx *c, const double *pts, int count, double *v, double *dist)
{
    if (!c || !pts || count < 1 || !v || !dist) return LSC_EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    DevBuf<double> d_p, d_v, d_d;           // (released on every return)
    HIPCHK(c, d_p.upload(pts, 18 * (size_t)count));
    HIPCHK(c, d_v.alloc(3 * (size_t)count));
    HIPCHK(c, d_d.alloc((size_t)count));
    HIPCHK(c, launch_gjk(d_p, count, d_v, d_d, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(v, d_v, sizeof(double) * 3 * (size_t)count, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(dist, d_d, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    return LSC_OK;
}

int lsc_set_timing(lsc_ctx *c, int enabled)
{
    if (!c) return LSC_EINVAL;
    // The stamp slots in use go back to "armed" -- after the launches that may still write them: the stream of the last stamped group is
    // synchronised first.  (Their samples are dropped with everybody else's.)
    if (c->stamp_used > 0) {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        HIPCHK(c, hipStreamSynchronize(c->stamp_stream));
        HIPCHK(c, arm_stamps(c, c->stamp_used));
    }
    if (enabled && !c->timing_events && !c->own.d_stamps) {
        // (the first lsc_set_timing(1) of the context: the device's clock rate and the slots, armed -- here and not at the first timed launch,
        //  which would pay an allocation and a copy inside somebody's timed window)
        HIPCHK(c, hipSetDevice(c->cfg.device));
        int khz = 0;
        HIPCHK(c, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->cfg.device));
        if (khz <= 0) { c->err = "lsc_set_timing: the device reports no wall clock rate"; return LSC_EHIP; }
        c->clock_khz = (double)khz;
        HIPCHK(c, c->own.d_stamps.alloc(2 * (size_t)c->stamp_slots));
        HIPCHK(c, arm_stamps(c, (size_t)c->stamp_slots));
    }
    c->timing = enabled != 0;
    for (int w = 0; w < TIMED_GROUPS; w++) c->ev_used[w] = 0;
    c->stamp_used = 0;
    c->plan_samples.clear();
    c->host_tick_ms.clear();
    return LSC_OK;
}

// sample i of an event pool: the pair's dispatch-bound timestamps
static int event_sample_ms(lsc_ctx *c, int which, size_t i, double *ms_out)
{
    auto &p = c->ev_pool[which][i];
    HIPCHK(c, hipEventSynchronize(p.second));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, p.first, p.second));
    *ms_out = ms;
    return LSC_OK;
}

// Samples [0, n) of group `which` in launch order -> out (null: only their sum).  The plan group's stamped samples cost one synchronisation
// of the stream they were launched on and ONE copy of the slots in use; ticks of the device's constant-rate clock -> ms by its rate.
static int timed_samples_ms(lsc_ctx *c, int which, long n, double *out, double *sum)
{
    double tot = 0;
    if (which != 0) {
        for (long i = 0; i < n; i++) {
            double ms = 0;
            if (event_sample_ms(c, which, (size_t)i, &ms) != LSC_OK) return LSC_EHIP;
            if (out) out[i] = ms;
            tot += ms;
        }
        if (sum) *sum = tot;
        return LSC_OK;
    }
    std::vector<long long> h(2 * c->stamp_used);
    if (c->stamp_used > 0) {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        HIPCHK(c, hipStreamSynchronize(c->stamp_stream));
        HIPCHK(c, hipMemcpy(h.data(), c->own.d_stamps, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
    }
    for (long i = 0; i < n; i++) {
        const int src = c->plan_samples[(size_t)i];
        double ms = 0;
        if (src >= 0) {
            const long long t0 = h[2 * (size_t)src], t1 = h[2 * (size_t)src + 1];
            // (a slot that is still armed: the group's launch failed; it reads as 0, as an event pair that was never bound would fail)
            if (t0 != STAMP_ARMED[0] && t1 != STAMP_ARMED[1]) ms = (double)(t1 - t0) / c->clock_khz;
        } else if (event_sample_ms(c, 0, (size_t)~src, &ms) != LSC_OK) return LSC_EHIP;
        if (out) out[i] = ms;
        tot += ms;
    }
    if (sum) *sum = tot;
    return LSC_OK;
}
static long timed_samples(const lsc_ctx *c, int which) { return which == 0 ? (long)c->plan_samples.size() : (long)c->ev_used[which]; }

int lsc_kernel_time_ms(lsc_ctx *c, int which, double *avg_ms, long *launches)
{
    if (c && which == LSC_TIME_STAMPED_COUNT && avg_ms) {      // (no time: where the plan group's samples came from)
        *avg_ms = 0.0;
        if (launches) *launches = (long)c->stamp_used;
        return LSC_OK;
    }
    if (!c || which < 0 || which >= TIMED_GROUPS || !avg_ms) return LSC_EINVAL;
    if (which == 5) {
        double t = 0;
        for (double v : c->host_tick_ms) t += v;
        *avg_ms = c->host_tick_ms.empty() ? 0.0 : t / (double)c->host_tick_ms.size();
        if (launches) *launches = (long)c->host_tick_ms.size();
        return LSC_OK;
    }
    const long n = timed_samples(c, which);
    double tot = 0;
    if (int rc = timed_samples_ms(c, which, n, nullptr, &tot)) return rc;
    *avg_ms = n ? tot / (double)n : 0.0;
    if (launches) *launches = n;
    return LSC_OK;
}

int lsc_kernel_times_ms(lsc_ctx *c, int which, double *out_ms, long capacity, long *launches)
{
    if (!c || which < 0 || which >= TIMED_GROUPS || (capacity > 0 && !out_ms)) return LSC_EINVAL;
    if (which == 5) {
        const long nh = (long)c->host_tick_ms.size();
        for (long i = 0; i < nh && i < capacity; i++) out_ms[i] = c->host_tick_ms[(size_t)i];
        if (launches) *launches = nh;
        return LSC_OK;
    }
    const long n = timed_samples(c, which);
    if (int rc = timed_samples_ms(c, which, n < capacity ? n : (capacity > 0 ? capacity : 0), out_ms, nullptr)) return rc;
    if (launches) *launches = n;
    return LSC_OK;
}

// Diagnostics: phase profile of the plan kernel.  enable=1 switches to the instrumented kernel variant and clears
// the counters; out (may be null) receives [N][12] cycle counts (100 MHz wall clock) accumulated since then.
int lsc_phase_profile(lsc_ctx *c, int enable, long long *out)
{
    if (!c || c->N == 0) return LSC_EINVAL;
    // (checked before anything is copied: a refused call leaves `out` untouched)
    if (enable > 0 && c->cfg.world_dimension == 2) { c->err = "lsc_phase_profile: the instrumented plan kernel exists for 3-D worlds only"; return LSC_EINVAL; }
    if (enable > 0 && c->swarm.obs.K > 0) { c->err = "lsc_phase_profile: no instrumented plan kernel is built for a context with dynamic obstacles (lsc_set_obstacles)"; return LSC_EINVAL; }
    HIPCHK(c, hipDeviceSynchronize());
    if (out) HIPCHK(c, hipMemcpy(out, c->swarm.d_prof, sizeof(long long) * PROF_PHASES * (size_t)c->N, hipMemcpyDeviceToHost));
    if (enable >= 0) {
        c->profiling = enable != 0;
        HIPCHK(c, hipMemset(c->swarm.d_prof, 0, sizeof(long long) * 2 * PROF_PHASES * (size_t)c->N));
    }
    return LSC_OK;
}

// Diagnostics: section profile of lsc_general_kernel (the alternate planner modes), collected while lsc_phase_profile is
// enabled and cleared with it.  out receives [N][16] shader cycles: set-up, start, then per interior-point section (residual
// pass, row reduction, assembly, factorization, both solves, affine pass, corrector right-hand side, its reduction and
// assembly, step), the iteration count and the number of solves of the agent.
int lsc_general_profile(lsc_ctx *c, long long *out)
{
    if (!c || c->N == 0 || !out) return LSC_EINVAL;
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, c->swarm.d_prof + PROF_PHASES * (size_t)c->N, sizeof(long long) * PROF_PHASES * (size_t)c->N, hipMemcpyDeviceToHost));
    return LSC_OK;
}

// Diagnostics of the alternate-mode solver, read-only: up to how many kept obstacles an agent of this swarm has all its row arrays in LDS
// (general_agent<true>; beyond, general_agent<false> with its last arrays in the HBM workspace), and how the last tick reached the solver.
int lsc_general_info(const lsc_ctx *c, int *lds_obstacles, int *last_launch)
{
    if (!c || c->N == 0) return LSC_EINVAL;
    if (lds_obstacles) *lds_obstacles = general_lds_obstacles(c->N + c->swarm.obs.K);      // (of N - 1 + K obstacles per agent)
    if (last_launch) *last_launch = c->last_general;
    return LSC_OK;
}

// Diagnostics: section profile of the goal planner's register-resident search.  enable = 1 switches to the instrumented
// kernel and clears the counters, 0 switches back, < 0 only reads; out (may be null) receives [N][8] shader cycles accumulated
// since then: prologue (priority / retreat rule), grid set-up, search, path + line-of-sight goal; of the search: findMin,
// deleteMin, neighbour screening, insertions.
int lsc_goal_profile(lsc_ctx *c, int enable, long long *out)
{
    if (!c || c->N == 0) return LSC_EINVAL;
    if (enable == 1 && c->goal_hbm) {
        c->err = "lsc_goal_profile: this context's grid is searched in HBM; the profile covers the LDS searches only";
        return LSC_ESTATE;
    }
    HIPCHK(c, hipDeviceSynchronize());
    if (!c->swarm.d_goal_prof) HIPCHK(c, c->swarm.d_goal_prof.alloc_zero(16 * (size_t)c->N));
    if (out) HIPCHK(c, hipMemcpy(out, c->swarm.d_goal_prof, sizeof(long long) * 16 * (size_t)c->N, hipMemcpyDeviceToHost));
    if (enable >= 0) {
        c->goal_profiling = enable != 0;
        HIPCHK(c, hipMemset(c->swarm.d_goal_prof, 0, sizeof(long long) * 16 * (size_t)c->N));
    }
    return LSC_OK;
}

// ---------------------------------------------------------------------------------------------------
// QP failure forensics.  On a solver failure the reference exports the model it could not solve (log/QPmodel.lp, CPLEX LP
// format, src/traj_optimizer.cpp:99-153); lsc_dump_qp writes the same file for one agent of the LAST host-buffer tick: variables
// x_m_i / y_m_i / z_m_i, rows c1.. in populatebyrow's order (:394-536: 15 equalities per axis, corridor rows, LSC rows of
// every obstacle, velocity / acceleration rows per axis, stop-at-horizon equalities), bounds (:274-303), objective as
// "linear + [ quadratic ] / 2 + constant".  Numbers are what the kernels used: LSC normals / margins from the dense sweep
// kernel on the tick's inputs, corridor boxes and planned goal from the context's device state.  LSC mode without slack
// rows (an agent whose rows carry slack variables after a disturbance has an alternate-mode QP: LSC_EINVAL).
int lsc_dump_qp(lsc_ctx *c, int agent, const char *path)
{
    if (!c || !path || c->N < 1 || agent < 0 || agent >= c->N) return LSC_EINVAL;
    if (agent < c->first || agent >= c->first + c->count) {
        // corridor boxes and plan inputs are only valid for the context's own shard: the owning rank writes the dump
        c->err = "lsc_dump_qp: the agent is not in this context's shard";
        return LSC_EINVAL;
    }
    if (c->last_host_seq < 1 || !c->swarm.h_in) { c->err = "lsc_dump_qp: no host-buffer tick has run on this context"; return LSC_ESTATE; }
    if (c->cfg.planner_mode != 0) { c->err = "lsc_dump_qp: LSC mode only"; return LSC_EINVAL; }
    if (c->swarm.obs.K > 0) { c->err = "lsc_dump_qp: the dump is not built for a context with dynamic obstacles (lsc_set_obstacles): its rows come from the agents' sweep"; return LSC_EINVAL; }
    const int N = c->N, nobs = N - 1, seq = c->last_host_seq;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());
    if (c->cfg.reset_threshold > 0.0 && c->swarm.d_ever) {
        std::vector<unsigned char> ever(N);
        HIPCHK(c, hipMemcpy(ever.data(), c->swarm.d_ever, N, hipMemcpyDeviceToHost));
        for (int q = 0; q < N; q++)
            if (ever[q]) { c->err = "lsc_dump_qp: the swarm carries slack rows of a disturbance reset (alternate-mode QP)"; return LSC_EINVAL; }
    }
    const float *state = c->swarm.h_in, *prev = c->swarm.h_in + 12 * (size_t)N;
    // the agent's LSC (generateLSC) from the sweep kernel, its corridor and planned goal from the context
    std::vector<float> normal((size_t)std::max(nobs, 1) * M * 3), sfc(M * 6), goal(3);
    std::vector<double> dd((size_t)std::max(nobs, 1) * M * NC), vmax(3), amax(3);
    double vnom = 1.0;
    if (nobs > 0) {
        DevBuf<float> d_n;
        DevBuf<double> d_d;
        HIPCHK(c, d_n.alloc(normal.size()));
        HIPCHK(c, d_d.alloc(dd.size()));
        SweepArgs s;
        s.N = N; s.first = agent; s.count = 1; s.planner_seq = seq; s.dtf = (float)c->cfg.dt;
        s.state = c->swarm.d_state; s.traj_prev = c->swarm.d_prev;
        s.radius = c->swarm.d_radius; s.radius_obs = c->swarm.d_radius_obs; s.downwash = c->swarm.d_downwash; s.downwash_obs = c->swarm.d_downwash_obs;
        s.out_normal = d_n; s.out_d = d_d;
        HIPCHK(c, launch_sweep(s, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(normal.data(), d_n, sizeof(float) * normal.size(), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(dd.data(), d_d, sizeof(double) * dd.size(), hipMemcpyDeviceToHost));
    }
    HIPCHK(c, hipMemcpy(goal.data(), c->swarm.d_goal_cur + 3 * (size_t)agent, sizeof(float) * 3, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(vmax.data(), c->swarm.d_vmax + 3 * (size_t)agent, sizeof(double) * 3, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(amax.data(), c->swarm.d_amax + 3 * (size_t)agent, sizeof(double) * 3, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&vnom, c->swarm.d_vnom + agent, sizeof(double), hipMemcpyDeviceToHost));
    if (c->cfg.use_octomap) HIPCHK(c, hipMemcpy(sfc.data(), c->swarm.d_sfc + (size_t)agent * M * 6, sizeof(float) * M * 6, hipMemcpyDeviceToHost));
    FILE *f = std::fopen(path, "w");
    if (!f) { c->err = std::string("lsc_dump_qp: cannot write ") + path; return LSC_EINVAL; }
    const char ax[3] = {'x', 'y', 'z'};
    const int n = DEG, phi = 3;
    const int dim = c->cfg.world_dimension == 2 ? 2 : 3;      // dim = param.world_dimension: a planar world has 60 variables (:8, 264-266)
    const double dt = c->cfg.dt, wc = c->cfg.control_weight, wt = c->cfg.terminal_weight;
    auto var = [&](int k, int m, int i) { char b[32]; std::snprintf(b, sizeof b, "%c_%d_%d", ax[k], m, i); return std::string(b); };
    struct Term { double v; std::string name; };
    auto emit = [&](const std::vector<Term> &t) {       // " - 25 x_0_0 + 25 x_0_1"; unit coefficients are left out like CPLEX does
        bool first = true;
        for (const Term &q : t) {
            if (q.v == 0.0) continue;
            const double m = std::fabs(q.v);
            std::fprintf(f, "%s", q.v < 0 ? (first ? " - " : " - ") : (first ? " " : " + "));
            if (m != 1.0) std::fprintf(f, "%.15g ", m);
            std::fprintf(f, "%s", q.name.c_str());
            first = false;
        }
        if (first) std::fprintf(f, " 0 %s", var(0, 0, 0).c_str());
    };
    // ---- objective: w_c sum x^T Q_base x + w_t sum_{m >= M - T} |c_{m,n} - goal|^2   (:329-372)
    const float *sa = state + 9 * (size_t)agent;
    int T;
    {
        const float dx = goal[0] - sa[0], dy = goal[1] - sa[1], dz = goal[2] - sa[2];
        const float n2 = dx * dx + dy * dy + dz * dz;
        const double ideal = std::sqrt((double)n2) / vnom;       // octomath norm: float32 sum of squares, double sqrt
        T = std::max((int)((M * dt - ideal + 1e-9) / dt), 1);
    }
    double Q[NC * NC];
    build_qbase(dt, Q);
    std::fprintf(f, "\\ENCODING=ISO-8859-1\n\\Problem name: lsc_planner_amd (agent %d, planner_seq %d)\n\nMinimize\n obj1:", agent, seq);
    {
        std::vector<Term> lin;
        for (int k = dim - 1; k >= 0; k--)
            for (int m = M - 1; m >= M - T; m--) lin.push_back({-2.0 * wt * (double)goal[k], var(k, m, n)});
        emit(lin);
        std::fprintf(f, " + [");
        bool first = true;
        for (int k = dim - 1; k >= 0; k--)
            for (int m = M - 1; m >= 0; m--)
                for (int i = n; i >= 0; i--)
                    for (int j = i; j >= 0; j--) {
                        // "[ ... ] / 2": the bracket holds twice the objective's quadratic coefficients
                        double v = i == j ? 2.0 * wc * Q[i * NC + i] : 2.0 * wc * (Q[i * NC + j] + Q[j * NC + i]);
                        if (i == j && i == n && m >= M - T) v += 2.0 * wt;
                        if (v == 0.0) continue;
                        std::fprintf(f, "%s%.15g %s", v < 0 ? " - " : (first ? " " : " + "), std::fabs(v), var(k, m, i).c_str());
                        if (i == j) std::fprintf(f, " ^2"); else std::fprintf(f, " * %s", var(k, m, j).c_str());
                        first = false;
                    }
        double cst = 0.0;
        for (int k = 0; k < dim; k++) cst += wt * T * (double)goal[k] * (double)goal[k];
        std::fprintf(f, " ] / 2 + %.15g\nSubject To\n", cst);
    }
    int row = 0;
    auto begin_row = [&]() { std::fprintf(f, " c%d:", ++row); };
    // ---- equalities (:394-405, Aeq_base :186-236, deq :239-259)
    const double A0[3][3] = {{1, 0, 0}, {-1, 1, 0}, {1, -2, 1}};       // A_0 rows 0..2, columns 0..2
    const double AT[3][3] = {{0, 0, 1}, {0, -1, 1}, {1, -2, 1}};       // A_T rows 0..2, columns n-2..n
    for (int k = 0; k < dim; k++) {
        int nn = 1;
        for (int i = 0; i < phi; i++) {
            std::vector<Term> t;
            for (int j = 0; j < 3; j++) t.push_back({std::pow(dt, -i) * nn * A0[i][j], var(k, 0, j)});
            begin_row(); emit(t);
            std::fprintf(f, " = %.15g\n", (double)sa[3 * i + k]);
            nn *= n - i;
        }
        for (int m = 1; m < M; m++) {
            nn = 1;
            for (int j = 0; j < phi; j++) {
                std::vector<Term> t;
                for (int q = 0; q < 3; q++) t.push_back({-std::pow(dt, -j) * nn * A0[j][q], var(k, m, q)});
                for (int q = 2; q >= 0; q--) t.push_back({std::pow(dt, -j) * nn * AT[j][q], var(k, m - 1, n - 2 + q)});
                begin_row(); emit(t);
                std::fprintf(f, " = 0\n");
                nn *= n - j;
            }
        }
    }
    const int ncs = c->cfg.n_constraint_segments > 0 ? std::min(c->cfg.n_constraint_segments, (int)M) : (int)M;
    // ---- corridor rows (:409-434; Box::convertToLSCs src/collision_constraints.cpp:37-59)
    if (c->cfg.use_octomap)
        for (int m = 0; m < ncs; m++)
            for (int k = 0; k < dim; k++)                         // Box::convertToLSCs(world_dimension): 2 dim half-spaces
                for (int side = 0; side < 2; side++)
                    for (int j = 0; j <= n; j++) {
                        if (m == 0 && j < phi) continue;
                        begin_row();
                        emit({{side == 0 ? 1.0 : -1.0, var(k, m, j)}});
                        std::fprintf(f, " >= %.15g\n", side == 0 ? (double)sfc[m * 6 + k] : -(double)sfc[m * 6 + 3 + k]);
                    }
    // ---- LSC rows (:437-466): n . (c_{m,i} - q_i) - d_i >= 0, q = the obstacle's predicted control point
    for (int oi = 0; oi < nobs; oi++) {
        const int qj = oi < agent ? oi : oi + 1;
        for (int m = 0; m < ncs; m++)
            for (int i = 0; i <= n; i++) {
                if (m == 0 && i < phi) continue;
                float q[3];
                if (seq < 2) {
                    const float *s = state + 9 * (size_t)qj;
                    const float mi = (float)((double)m + (double)i / (double)n), dtf = (float)dt;
                    for (int k = 0; k < 3; k++) { const float a1 = s[3 + k] * mi; const float a2 = a1 * dtf; q[k] = s[k] + a2; }
                } else {
                    const float *t = prev + (size_t)qj * NV;
                    const int cc = m < M - 1 ? (m + 1) * NC + i : (M - 1) * NC + n;
                    for (int k = 0; k < 3; k++) q[k] = t[k * SEGV + cc];
                }
                const float *nv = normal.data() + ((size_t)oi * M + m) * 3;
                double rhs = dd[((size_t)oi * M + m) * NC + i];
                std::vector<Term> t;
                for (int k = dim - 1; k >= 0; k--) { t.push_back({(double)nv[k], var(k, m, i)}); }
                for (int k = 0; k < dim; k++) rhs += (double)nv[k] * (double)q[k];   // (the z term only `if (dim == 3)`, :450)
                begin_row(); emit(t);
                std::fprintf(f, " >= %.15g\n", rhs);
            }
    }
    // ---- velocity / acceleration rows (:469-523)
    for (int k = 0; k < dim; k++)
        for (int m = 0; m < M; m++) {
            const double cv = std::pow(dt, -1) * n, ca = std::pow(dt, -2) * n * (n - 1);
            for (int i = 0; i < n; i++) {
                if (m == 0 && (i == 0 || i == 1)) continue;
                for (int sg = 1; sg >= -1; sg -= 2) {
                    begin_row(); emit({{sg * cv, var(k, m, i + 1)}, {-sg * cv, var(k, m, i)}});
                    std::fprintf(f, " <= %.15g\n", vmax[k]);
                }
            }
            for (int i = 0; i < n - 1; i++) {
                if (m == 0 && i == 0) continue;
                for (int sg = 1; sg >= -1; sg -= 2) {
                    begin_row(); emit({{sg * ca, var(k, m, i + 2)}, {-2.0 * sg * ca, var(k, m, i + 1)}, {sg * ca, var(k, m, i)}});
                    std::fprintf(f, " <= %.15g\n", amax[k]);
                }
            }
        }
    // ---- stop at the horizon (:529-536)
    for (int k = 0; k < dim; k++)
        for (int i = 1; i < phi; i++) {
            begin_row(); emit({{1.0, var(k, M - 1, n)}, {-1.0, var(k, M - 1, n - i)}});
            std::fprintf(f, " = 0\n");
        }
    // ---- bounds (:274-303)
    std::fprintf(f, "Bounds\n");
    for (int k = dim - 1; k >= 0; k--)
        for (int m = M - 1; m >= 0; m--)
            for (int i = n; i >= 0; i--) {
                if (m == 0 && i < 3) continue;
                std::fprintf(f, " %.15g <= %s <= %.15g\n", (double)c->cfg.world_min[k], var(k, m, i).c_str(), (double)c->cfg.world_max[k]);
            }
    for (int k = dim - 1; k >= 0; k--)
        for (int i = 0; i < 3; i++) std::fprintf(f, "      %s Free\n", var(k, 0, i).c_str());
    std::fprintf(f, "End\n");
    std::fclose(f);
    return LSC_OK;
}

// per-iteration solver trace of one agent: [64][8] = gap, |rp|, objective, affine step, sigma, step, |dx_aff|, mu
int lsc_solver_trace(lsc_ctx *c, int agent, double *out)
{
    if (!c || c->N == 0) return LSC_EINVAL;
    HIPCHK(c, hipDeviceSynchronize());
    if (!c->own.d_trace) HIPCHK(c, c->own.d_trace.alloc(64 * 8 + NY * KLD + W_SIZE + 512));
    if (out) HIPCHK(c, hipMemcpy(out, c->own.d_trace, sizeof(double) * (64 * 8 + NY * KLD + W_SIZE + 512), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemset(c->own.d_trace, 0, sizeof(double) * (64 * 8 + NY * KLD + W_SIZE + 512)));
    c->trace_agent = agent;
    return LSC_OK;
}

// last (gap, |rp|, |rd|, objective) of every agent's solve, [N][4]
int lsc_solver_residuals(lsc_ctx *c, double *out)
{
    if (!c || !out || c->N == 0) return LSC_EINVAL;
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, c->swarm.d_dbg, sizeof(double) * 4 * (size_t)c->N, hipMemcpyDeviceToHost));
    return LSC_OK;
}

// sum over agents of the interior-point iterations run since the last reset (bench flop accounting)
int lsc_iterations_total(lsc_ctx *c, long long *total, int reset)
{
    if (!c || !total || c->N == 0) return LSC_EINVAL;
    std::vector<long long> h(c->N);
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(h.data(), c->swarm.d_iters_acc, sizeof(long long) * (size_t)c->N, hipMemcpyDeviceToHost));
    long long t = 0;
    for (long long v : h) t += v;
    *total = t;
    if (reset) HIPCHK(c, hipMemset(c->swarm.d_iters_acc, 0, sizeof(long long) * (6 * (size_t)c->N)));
    return LSC_OK;
}

// sum over agents of (interior-point iterations x LSC rows the agent's QP carried) since the last reset of lsc_iterations_total:
// the row passes the kernels executed, against the 27 (N - 1) rows per iteration the reference's model holds
int lsc_row_iterations_total(lsc_ctx *c, long long *total)
{
    if (!c || !total || c->N == 0) return LSC_EINVAL;
    std::vector<long long> h(c->N);
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(h.data(), c->swarm.d_iters_acc + c->N, sizeof(long long) * (size_t)c->N, hipMemcpyDeviceToHost));
    long long t = 0;
    for (long long v : h) t += v;
    *total = t;
    return LSC_OK;
}

// counters of the active-set solve since the last reset of lsc_iterations_total: agent-replans it finished, agent-replans it handed to
// the interior point, changes of the working set, interior-point iterations of the handed-over agents
int lsc_solver_stats(lsc_ctx *c, long long out[4])
{
    if (!c || !out || c->N == 0) return LSC_EINVAL;
    HIPCHK(c, hipDeviceSynchronize());
    // (kept per agent on the device -- four counters every workgroup of a tick added to were 0.6 us at the end of a 64-agent tick -- and summed here)
    std::vector<long long> h(4 * (size_t)c->N);
    HIPCHK(c, hipMemcpy(h.data(), c->swarm.d_iters_acc + 2 * (size_t)c->N, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; k++) out[k] = 0;
    for (int q = 0; q < c->N; q++) for (int k = 0; k < 4; k++) out[k] += h[4 * (size_t)q + k];
    return LSC_OK;
}

// largest working set of every agent's last active-set solve (diagnostics, tests): the first call allocates the per-agent array -- from
// then on the plan kernel stores into it -- and reads zeros; GQ + 1 = 13: the solve handed the agent over for want of a thirteenth slot
int lsc_working_set_peaks(lsc_ctx *c, int *peaks /*[N]*/)
{
    if (!c || !peaks || c->N == 0) return LSC_EINVAL;
    HIPCHK(c, hipDeviceSynchronize());
    if (!c->swarm.d_ws_peak) HIPCHK(c, c->swarm.d_ws_peak.alloc_zero((size_t)c->N));
    HIPCHK(c, hipMemcpy(peaks, c->swarm.d_ws_peak, sizeof(int) * (size_t)c->N, hipMemcpyDeviceToHost));
    return LSC_OK;
}

int lsc_set_goal_trace(lsc_ctx *c, int path_cap)
{
    if (!c || c->N == 0 || path_cap < 0) return LSC_EINVAL;
    c->swarm.d_goal_path.reset();
    c->swarm.d_goal_plen.reset();
    c->goal_path_cap = path_cap;
    if (path_cap > 0) {
        HIPCHK(c, c->swarm.d_goal_path.alloc((size_t)c->N * path_cap));
        HIPCHK(c, c->swarm.d_goal_plen.alloc_zero((size_t)c->N));
    }
    return LSC_OK;
}

int lsc_get_goal_trace(lsc_ctx *c, int *path_cells, int *path_len, int *flags, int *expansions, int grid_dims[3],
                       double grid_min[3])
{
    if (!c || c->N == 0) return LSC_EINVAL;
    if (!c->swarm.map.d_goal_flags) { c->err = "goal trace: the goal planner is not active (goal_mode 1 + use_octomap + distmap)"; return LSC_ESTATE; }
    HIPCHK(c, hipDeviceSynchronize());
    const size_t cnt = c->count, first = c->first;
    if (flags) HIPCHK(c, hipMemcpy(flags, c->swarm.map.d_goal_flags + first, sizeof(int) * cnt, hipMemcpyDeviceToHost));
    if (expansions) HIPCHK(c, hipMemcpy(expansions, c->swarm.map.d_goal_exp + first, sizeof(int) * cnt, hipMemcpyDeviceToHost));
    if (grid_dims) for (int k = 0; k < 3; k++) grid_dims[k] = c->grid_dims[k];
    if (grid_min) for (int k = 0; k < 3; k++) grid_min[k] = c->grid_min[k];
    if (path_len || path_cells) {
        if (!c->swarm.d_goal_path) { c->err = "goal trace: call lsc_set_goal_trace(ctx, path_cap) first"; return LSC_ESTATE; }
        std::vector<int> len(cnt), keys(cnt * (size_t)c->goal_path_cap);
        HIPCHK(c, hipMemcpy(len.data(), c->swarm.d_goal_plen, sizeof(int) * cnt, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(keys.data(), c->swarm.d_goal_path, sizeof(int) * keys.size(), hipMemcpyDeviceToHost));
        const int H = c->grid_dims[0], W = c->grid_dims[1];
        for (size_t q = 0; q < cnt; q++) {
            if (path_len) path_len[q] = len[q];
            if (!path_cells) continue;
            for (int t = 0; t < len[q] && t < c->goal_path_cap; t++) {
                const int key = keys[q * c->goal_path_cap + t];
                const int z = key / (H * W), rem = key % (H * W);
                int *o = path_cells + (q * c->goal_path_cap + t) * 3;
                o[0] = rem / W; o[1] = rem % W; o[2] = z;
            }
        }
    }
    return LSC_OK;
}

int lsc_last_goals(lsc_ctx *c, float *goals)
{
    if (!c || !goals || c->N == 0) return LSC_EINVAL;
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(goals, c->swarm.d_goal_cur, sizeof(float) * 3 * (size_t)c->N, hipMemcpyDeviceToHost));
    return LSC_OK;
}

int lsc_goal_storage(lsc_ctx *c, int *where)
{
    if (!c || !where || c->N == 0) return LSC_EINVAL;
    if (!plans_goals(c) || !c->swarm.map.d_goal_storage) { c->err = "lsc_goal_storage: the context plans no goals on a distance field"; return LSC_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipDeviceSynchronize());
    if (c->count > 0) HIPCHK(c, hipMemcpy(where, c->swarm.map.d_goal_storage + c->first, sizeof(int) * (size_t)c->count, hipMemcpyDeviceToHost));
    return LSC_OK;
}

// LSC rows an agent may carry before it is handed to the pass with its rows in HBM: latency build (512 lanes, shards that fit
// the chip) and throughput build (256 lanes, two workgroups per CU; 0 when that build is not available for this context)
int lsc_row_capacity(const lsc_ctx *c, int *lds_rows, int *throughput_rows)
{
    if (!c || c->N == 0) return LSC_EINVAL;
    if (lds_rows) *lds_rows = c->cap;
    if (throughput_rows) *throughput_rows = c->cap_tp;
    return LSC_OK;
}

// rows of the fullest control-point bucket of every agent in the last tick (what the LDS row capacity has to hold)
int lsc_last_bucket_max(lsc_ctx *c, int *rows /*[N]*/)
{
    if (!c || !rows || c->N == 0) return LSC_EINVAL;
    HIPCHK(c, hipMemcpy(rows, c->swarm.d_bmax, sizeof(int) * (size_t)c->N, hipMemcpyDeviceToHost));
    return LSC_OK;
}

// read-back of per-agent active LSC row counts of the last tick (diagnostics for bench / tests)
int lsc_last_row_counts(lsc_ctx *c, int *rows /*[N]*/)
{
    if (!c || !rows || c->N == 0) return LSC_EINVAL;
    HIPCHK(c, hipMemcpy(rows, c->swarm.d_nrows, sizeof(int) * (size_t)c->N, hipMemcpyDeviceToHost));
    return LSC_OK;
}

// read-back of the neighbour-list lengths of the last tick (diagnostics)
int lsc_neighbour_counts(lsc_ctx *c, int *units /*[N]*/, int *priority_candidates /*[N] or null*/)
{
    if (!c || !units || c->N == 0) return LSC_EINVAL;
    if (!c->swarm.neigh.cnt) { c->err = "this context builds no neighbour lists (fewer than 512 or more than 65536 agents, prune != 1, or LSC_NO_NEIGHBOUR_LISTS)"; return LSC_ESTATE; }
    HIPCHK(c, hipMemcpy(units, c->swarm.neigh.cnt, sizeof(int) * (size_t)c->N, hipMemcpyDeviceToHost));
    if (priority_candidates) {
        HIPCHK(c, hipMemcpy(priority_candidates, c->swarm.neigh.pcnt, sizeof(int) * (size_t)c->N, hipMemcpyDeviceToHost));
        for (int q = 0; q < c->N; q++) if (priority_candidates[q] >= 0) priority_candidates[q] &= 0xffff;      // (bit 30: the swarm's disturbance bit)
    }
    return LSC_OK;
}

// read-back of everything the two kernels of lsc_neigh.hip wrote in the last tick (diagnostics: tests/test_gpu_neighbour_lists.py holds it
// to a float64 statement of the same bounds).  Copies only; the lists are decoded as phase B of plan_agent decodes them.
int lsc_neighbour_dump(lsc_ctx *c, int caps[2], float *obs_bound, float *seg_bound, float *reach, float *query_radius, int *unit_count, int *units,
                       int *priority_count, int *priority, int *disturbed)
{
    if (!c || c->N == 0) return LSC_EINVAL;
    const NeighArgs &g = c->swarm.neigh;
    if (!g.cnt) { c->err = "this context builds no neighbour lists (fewer than 512 or more than 65536 agents, prune != 1, or LSC_NO_NEIGHBOUR_LISTS)"; return LSC_ESTATE; }
    if (c->neigh_skipped) { c->err = std::string("the last tick built no neighbour lists: ") + c->neigh_skipped; return LSC_ESTATE; }
    if (caps) { caps[0] = g.list_cap; caps[1] = g.plist_cap; }
    const size_t N = (size_t)c->N;
    HIPCHK(c, hipDeviceSynchronize());
    if (obs_bound) HIPCHK(c, hipMemcpy(obs_bound, g.obs_bound, sizeof(float) * 4 * N, hipMemcpyDeviceToHost));
    if (seg_bound) HIPCHK(c, hipMemcpy(seg_bound, g.seg_bound, sizeof(float) * 4 * M * N, hipMemcpyDeviceToHost));
    if (reach) HIPCHK(c, hipMemcpy(reach, g.reach, sizeof(float) * M * N, hipMemcpyDeviceToHost));
    if (query_radius) {
        // slot 0 of NeighArgs::glob (G_RADIUS of lsc_neigh.hip): the tick's tag in the upper word, the float's bits in the lower; a stale tag reads as 0
        unsigned long long w = 0;
        HIPCHK(c, hipMemcpy(&w, g.glob, sizeof(w), hipMemcpyDeviceToHost));
        const unsigned bits = (unsigned)(w >> 32) == g.tag ? (unsigned)w : 0u;
        memcpy(query_radius, &bits, sizeof(float));
    }
    std::vector<int> cnt(N), pcnt(N);
    HIPCHK(c, hipMemcpy(cnt.data(), g.cnt, sizeof(int) * N, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(pcnt.data(), g.pcnt, sizeof(int) * N, hipMemcpyDeviceToHost));
    if (unit_count) for (size_t q = 0; q < N; q++) unit_count[q] = cnt[q];
    if (units) {
        std::vector<unsigned short> list((size_t)g.list_cap * N);
        std::vector<unsigned long long> blk(g.blk ? N : 0);
        HIPCHK(c, hipMemcpy(list.data(), g.list, sizeof(unsigned short) * list.size(), hipMemcpyDeviceToHost));
        if (g.blk) HIPCHK(c, hipMemcpy(blk.data(), g.blk, sizeof(unsigned long long) * N, hipMemcpyDeviceToHost));
        for (size_t q = 0; q < N; q++) {
            int *out = units + q * (size_t)g.list_cap;
            const int n = std::min(std::max(cnt[q], 0), g.list_cap);
            // (plan_agent: the high part of entry i is the number of k with i >= start k, start k = field k of blk, 0xffff = none)
            int start[4];
            for (int k = 0; k < 4; k++) {
                const unsigned s = g.blk ? (unsigned)(blk[q] >> (16 * k)) & 0xffffu : 0xffffu;
                start[k] = s == 0xffffu ? 0x7fffffff : (int)s;
            }
            for (int i = 0; i < n; i++)
                out[i] = (int)list[q * (size_t)g.list_cap + i] | (((i >= start[0]) + (i >= start[1]) + (i >= start[2]) + (i >= start[3])) << 16);
            for (int i = n; i < g.list_cap; i++) out[i] = -1;
        }
    }
    if (priority_count) for (size_t q = 0; q < N; q++) priority_count[q] = pcnt[q] < 0 ? -1 : (pcnt[q] & 0xffff);
    if (disturbed) for (size_t q = 0; q < N; q++) disturbed[q] = pcnt[q] < 0 ? -1 : ((pcnt[q] >> 30) & 1);
    if (priority) {
        std::vector<unsigned short> pl((size_t)g.plist_cap * N);
        HIPCHK(c, hipMemcpy(pl.data(), g.plist, sizeof(unsigned short) * pl.size(), hipMemcpyDeviceToHost));
        for (size_t q = 0; q < N; q++) {
            const int n = pcnt[q] < 0 ? 0 : std::min(pcnt[q] & 0xffff, g.plist_cap);
            for (int i = 0; i < g.plist_cap; i++) priority[q * (size_t)g.plist_cap + i] = i < n ? (int)pl[q * (size_t)g.plist_cap + i] : -1;
        }
    }
    return LSC_OK;
}

}  // extern "C"
