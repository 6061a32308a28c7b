// lsc_obstacle_motion.hpp -- getObstacle(t) of the reference's include/obstacle.hpp, each statement ONCE: the three obstacle types whose
// motion is a closed form of the time alone -- straight (:123-173), spin (:68-121), multisim_patrol (:175-231) -- and, further down, the
// two with state or history of their own: chasing (:234-328, obstacle_chase_step) and gaussian (:330-435, obstacle_gaussian_at).
//
// Value in, value out, like lsc_rules.hpp / lsc_flight.hpp: the obstacle stage (lsc_obstacles.hip), the installation of the table
// (lsc_obstacle_motion, lsc_abi.cpp) and the stand-alone host check of tests/test_obstacle_motion_device_rules.py call the same text (LSC_HD).
// The statements are ObstacleMotion's (host/lsc_host.hpp), which the simulator feeds its ticks with today:
//
//   straight, patrol   + - x / sqrt and comparisons only, every one correctly rounded on host and device, nothing contracted: the same
//                      bits as ObstacleMotion::at.
//   chasing, gaussian  the same: + - x / sqrt and comparisons only, the same bits on host and device and the bits of ObstacleSet's float64
//                      restatement (tests/test_obstacle_reactive.py).  A chaser is the one obstacle with state (pos, vel, t_last) and the
//                      one that reads the swarm and the other obstacles: lsc_obstacle_step_kernel reads the previous tick, then writes
//   spin               goes through the platform's double sin / cos: within one float32 step of the rounded result (the bound
//                      tests/test_obstacle_motion.py holds the C++ host and ObstacleSet to).
//
// Everything that depends on the mission alone -- a leg's velocity and flight time, the spin's normalised axis and angular rate -- is
// formed ONCE, by the host, when the models are installed (obstacle_entry_build, a host function like obstacle_walk_ok: no kernel calls
// them); the stage reads the table.
#pragma once
#include <math.h>
#include <stddef.h>

#include "lsc_gjk.hpp"

namespace lsc {

constexpr int OBSTACLE_POINTS_MAX = 8;                                       // LSC_OBSTACLE_POINTS_MAX of include/lsc_planner_amd.h
constexpr int OBSTACLE_STRAIGHT = 0, OBSTACLE_SPIN = 1, OBSTACLE_PATROL = 2; // LSC_OBSTACLE_* (ObstacleMotion::kind)
constexpr double OBSTACLE_WALK_MAX = 65536.0;                                // legs a patrol walk may step over in one tick (obstacle_walk_ok)

// One obstacle's host-built constants.
//   straight   n_legs 1: leg 0 = start -> goal
//   patrol     n_legs n: leg i = waypoint i -> waypoint (i + 1) % n
//   spin       n_legs 0: a[0] the axis position, a[1] the normalised axis, a[2] start - axis position, w = speed / |r|
struct ObstacleEntry {
    int kind, n_legs;
    double w;
    double leg_time[OBSTACLE_POINTS_MAX];      // dist / speed
    double a[OBSTACLE_POINTS_MAX][3];          // where a leg starts
    double b[OBSTACLE_POINTS_MAX][3];          // where it ends
    double v[OBSTACLE_POINTS_MAX][3];          // speed * (d / dist) per axis
};

// why obstacle_entry_build refused its input
constexpr int OBSTACLE_OK = 0, OBSTACLE_BAD_KIND = 1, OBSTACLE_BAD_POINTS = 2, OBSTACLE_NOT_FINITE = 3, OBSTACLE_BAD_SPEED = 4,
              OBSTACLE_ON_AXIS = 5, OBSTACLE_NO_DISTANCE = 6;
inline const char *obstacle_refusal(int why)
{
    switch (why) {
    case OBSTACLE_BAD_KIND: return "unknown kind (straight 0, spin 1, multisim_patrol 2)";
    case OBSTACLE_BAD_POINTS: return "number of points (straight: start, goal; spin: axis position, axis, start; patrol: 2 to 8 waypoints)";
    case OBSTACLE_NOT_FINITE: return "a point or the speed is not finite";
    case OBSTACLE_BAD_SPEED: return "the speed is not positive";
    case OBSTACLE_ON_AXIS: return "the spin's start lies on its axis (or the axis has no length)";
    case OBSTACLE_NO_DISTANCE: return "the patrol's waypoints span no distance";
    }
    return "";
}

// ObstacleMotion::leg's constants: d = b - a, dist = sqrt(d . d), v = speed * (d / dist), flight time = dist / speed.  A leg of zero
// length has flight time 0: `t < 0` never holds, its velocity is never read (0 here instead of the quotient 0 / 0).
inline void obstacle_leg_build(ObstacleEntry &e, int i, const double a[3], const double b[3], double speed)
{
#pragma clang fp contract(off)
    const double d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, dist = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int k = 0; k < 3; k++) {
        e.a[i][k] = a[k]; e.b[i][k] = b[k];
        e.v[i][k] = dist > 0.0 ? speed * (d[k] / dist) : 0.0;
    }
    e.leg_time[i] = dist / speed;
}

// The table entry of one model (lsc_obstacle_model: kind, n_points, speed, points), with what Mission::initialize / ObstacleSet refuse.
// points of a spin: axis position, axis orientation of any length, start.
inline int obstacle_entry_build(int kind, int n_points, double speed, const double (*pts)[3], ObstacleEntry &e)
{
#pragma clang fp contract(off)
    e = ObstacleEntry{};
    if (kind != OBSTACLE_STRAIGHT && kind != OBSTACLE_SPIN && kind != OBSTACLE_PATROL) return OBSTACLE_BAD_KIND;
    const bool count_ok = kind == OBSTACLE_STRAIGHT ? n_points == 2 : kind == OBSTACLE_SPIN ? n_points == 3 : (n_points >= 2 && n_points <= OBSTACLE_POINTS_MAX);
    if (!count_ok || !pts) return OBSTACLE_BAD_POINTS;
    if (!isfinite(speed)) return OBSTACLE_NOT_FINITE;
    for (int i = 0; i < n_points; i++)
        for (int k = 0; k < 3; k++)
            if (!isfinite(pts[i][k])) return OBSTACLE_NOT_FINITE;
    if (!(speed > 0.0)) return OBSTACLE_BAD_SPEED;
    e.kind = kind;
    if (kind == OBSTACLE_STRAIGHT) {
        e.n_legs = 1;
        obstacle_leg_build(e, 0, pts[0], pts[1], speed);
    } else if (kind == OBSTACLE_PATROL) {
        e.n_legs = n_points;
        double total = 0.0;
        for (int i = 0; i < n_points; i++) {
            obstacle_leg_build(e, i, pts[i], pts[(i + 1) % n_points], speed);
            total += e.leg_time[i];
        }
        if (!(total > 0.0) || !isfinite(total)) return OBSTACLE_NO_DISTANCE;
    } else {
        // Mission::initialize: n /= |n|, start -= axis position; ObstacleMotion::at: r = a - (a . n) n, w = speed / |r|
        const double *c = pts[0], *n = pts[1], *st = pts[2];
        const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (!(nn > 0.0)) return OBSTACLE_ON_AXIS;
        for (int k = 0; k < 3; k++) { e.a[0][k] = c[k]; e.a[1][k] = n[k] / nn; e.a[2][k] = st[k] - c[k]; }
        const double *un = e.a[1], *a = e.a[2];
        const double dot = a[0] * un[0] + a[1] * un[1] + a[2] * un[2];
        const double r[3] = {a[0] - dot * un[0], a[1] - dot * un[1], a[2] - dot * un[2]};
        const double rr = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (!(rr > 0.0) || !isfinite(rr)) return OBSTACLE_ON_AXIS;
        e.w = speed / rr;
    }
    return OBSTACLE_OK;
}

// The patrol walk is the one loop whose trip count depends on data: a tick at time t steps over about t / (shortest positive leg time)
// legs at the most (legs of zero length come with a positive one each round).  Beyond OBSTACLE_WALK_MAX the tick is refused.
inline bool obstacle_walk_ok(const ObstacleEntry &e, double t)
{
    if (e.kind != OBSTACLE_PATROL) return true;
    double shortest = 0.0;
    for (int i = 0; i < e.n_legs; i++)
        if (e.leg_time[i] > 0.0 && (shortest == 0.0 || e.leg_time[i] < shortest)) shortest = e.leg_time[i];
    return shortest > 0.0 && t / shortest <= OBSTACLE_WALK_MAX;
}

// ObstacleMotion::leg
LSC_HD void obstacle_leg_at(const ObstacleEntry &e, int i, double t, double p[3], double v[3])
{
#pragma clang fp contract(off)
    const bool flying = t < e.leg_time[i];
    for (int k = 0; k < 3; k++) {
        const double vk = e.v[i][k];
        p[k] = flying ? e.a[i][k] + vk * t : e.b[i][k];
        v[k] = flying ? vk : 0.0;
    }
}

// ObstacleMotion::rotate (Rodrigues: q a q^-1 with q = (cos th/2, sin th/2 n))
LSC_HD void obstacle_rotate(const double n[3], const double a[3], double th, double o[3])
{
#pragma clang fp contract(off)
    const double c = cos(th), sn = sin(th), dot = n[0] * a[0] + n[1] * a[1] + n[2] * a[2];
    const double cr[3] = {n[1] * a[2] - n[2] * a[1], n[2] * a[0] - n[0] * a[2], n[0] * a[1] - n[1] * a[0]};
    for (int k = 0; k < 3; k++) o[k] = a[k] * c + cr[k] * sn + n[k] * dot * (1.0 - c);
}

constexpr double OBSTACLE_QUARTER_TURN = 1.57079632679489661923;       // M_PI / 2

// ObstacleMotion::at: position and velocity of the obstacle t seconds after the simulation's start, in doubles (the stage rounds to float32)
LSC_HD void obstacle_at(const ObstacleEntry &e, double t, double p[3], double v[3])
{
#pragma clang fp contract(off)
    if (e.kind == OBSTACLE_STRAIGHT) {
        obstacle_leg_at(e, 0, t, p, v);
    } else if (e.kind == OBSTACLE_SPIN) {
        double q[3], u[3];
        obstacle_rotate(e.a[1], e.a[2], e.w * t, q);
        obstacle_rotate(e.a[1], q, OBSTACLE_QUARTER_TURN, u);
        for (int k = 0; k < 3; k++) { p[k] = e.a[0][k] + q[k]; v[k] = e.w * u[k]; }
    } else {
        int i = 0;
        const int n = e.n_legs;
        while (t >= e.leg_time[i]) { t -= e.leg_time[i]; i = (i + 1) % n; }
        obstacle_leg_at(e, i, t, p, v);
    }
}

// ---- the two obstacle types with state or history of their own: chasing (include/obstacle.hpp:234-328, fed by updateObstacles of
// include/obstacle_generator.hpp:102-118) and gaussian (:330-435).  Like straight and patrol they use + - x / sqrt and comparisons only,
// every one correctly rounded on host and device, nothing contracted: obstacle_chase_step and obstacle_gaussian_at give the same bits on
// host and device (tests/test_obstacle_reactive.py holds the host build to ObstacleSet's float64 restatement, bit for bit).
constexpr int OBSTACLE_CHASING = 3, OBSTACLE_GAUSSIAN = 4;                   // LSC_OBSTACLE_CHASING / LSC_OBSTACLE_GAUSSIAN
constexpr int OBSTACLE_ACC_MAX = 4096;                                       // entries of one walker's acceleration history
constexpr double OBSTACLE_EPS = 1e-5;                                        // SP_EPSILON_FLOAT

// One chaser's parameters (ChasingObstacle's members).  radius is the class member, the mission file's double; target the agent whose
// position is the goal point of every step.
struct ObstacleChaser {
    int target, pad;
    double radius, max_vel, max_acc, gamma_target, gamma_obs;
    double start[3];
};
// current_state and t_last_called: 7 doubles, the row lsc_obstacle_chaser_states_read returns.  At installation start, 0, 0.
struct ObstacleChaserState { double pos[3], vel[3], t_last; };
// One walker's parameters (GaussianObstacle's members); its acc_history is n_acc rows of the context's acceleration table from acc_first on.
struct ObstacleWalker {
    int n_acc, acc_first;
    double max_vel, cycle;
    double start[3], initial_vel[3];
};

constexpr int OBSTACLE_BAD_MAX_VEL = 7, OBSTACLE_BAD_MAX_ACC = 8, OBSTACLE_BAD_TARGET = 9, OBSTACLE_BAD_CYCLE = 10, OBSTACLE_BAD_ACC_COUNT = 11;
inline const char *obstacle_refusal_ex(int why)
{
    switch (why) {
    case OBSTACLE_NOT_FINITE: return "a value is not finite";
    case OBSTACLE_BAD_MAX_VEL: return "max_vel is not positive";
    case OBSTACLE_BAD_MAX_ACC: return "max_acc is not above 0.01 (the acceleration clamp max_acc - 0.01 would divide 0 by 0)";
    case OBSTACLE_BAD_TARGET: return "the target is not an agent (0 .. N - 1)";
    case OBSTACLE_BAD_CYCLE: return "acc_update_cycle is not positive";
    case OBSTACLE_BAD_ACC_COUNT: return "the acceleration history has fewer than 1 or more than 4096 entries";
    }
    return obstacle_refusal(why);
}

inline int obstacle_chaser_build(int target, int n_agents, const double start[3], double radius, double max_vel, double max_acc, double gamma_target,
                                 double gamma_obs, ObstacleChaser &c)
{
    c = ObstacleChaser{};
    const double vals[5] = {radius, max_vel, max_acc, gamma_target, gamma_obs};
    for (double x : vals) if (!isfinite(x)) return OBSTACLE_NOT_FINITE;
    for (int k = 0; k < 3; k++) if (!isfinite(start[k])) return OBSTACLE_NOT_FINITE;
    if (!(max_vel > 0.0)) return OBSTACLE_BAD_MAX_VEL;
    if (!(max_acc > 0.01)) return OBSTACLE_BAD_MAX_ACC;
    if (target < 0 || target >= n_agents) return OBSTACLE_BAD_TARGET;
    c.target = target; c.radius = radius; c.max_vel = max_vel; c.max_acc = max_acc; c.gamma_target = gamma_target; c.gamma_obs = gamma_obs;
    for (int k = 0; k < 3; k++) c.start[k] = start[k];
    return OBSTACLE_OK;
}

// acc: host [n_acc][3] (null with n_acc < 1 is refused by the count)
inline int obstacle_walker_build(const double start[3], const double initial_vel[3], double max_vel, double cycle, int n_acc, const double *acc, int acc_first,
                                 ObstacleWalker &w)
{
    w = ObstacleWalker{};
    if (!isfinite(max_vel) || !isfinite(cycle)) return OBSTACLE_NOT_FINITE;
    for (int k = 0; k < 3; k++) if (!isfinite(start[k]) || !isfinite(initial_vel[k])) return OBSTACLE_NOT_FINITE;
    if (!(max_vel > 0.0)) return OBSTACLE_BAD_MAX_VEL;
    if (!(cycle > 0.0)) return OBSTACLE_BAD_CYCLE;
    if (n_acc < 1 || n_acc > OBSTACLE_ACC_MAX || !acc) return OBSTACLE_BAD_ACC_COUNT;
    for (int i = 0; i < 3 * n_acc; i++) if (!isfinite(acc[i])) return OBSTACLE_NOT_FINITE;
    w.n_acc = n_acc; w.acc_first = acc_first; w.max_vel = max_vel; w.cycle = cycle;
    for (int k = 0; k < 3; k++) { w.start[k] = start[k]; w.initial_vel[k] = initial_vel[k]; }
    return OBSTACLE_OK;
}

// history entries getGaussianObstacle reads at time t: floor((t + SP_EPSILON_FLOAT) / cycle) + 1 (:401, :408); a tick that needs more than
// n_acc is refused (the reference would draw more from std::random_device)
inline double obstacle_walker_entries(const ObstacleWalker &w, double t) { return floor((t + OBSTACLE_EPS) / w.cycle) + 1.0; }

// Eigen's norm of a 3-vector as every statement below uses it
LSC_HD double obstacle_norm3(const double x[3])
{
#pragma clang fp contract(off)
    return sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
}

// getChasingObstacle (:278-327), statement by statement.  goal: the goal point setGoalPoint was given (the target agent's position);
// others_pos / others_radius: the obstacles where the PREVIOUS step put them (setObstacles), n_others rows of which row `self` (the chaser's
// own, -1: none) is left out as obstacles_prev_step.erase does (obstacle_generator.hpp:108-110); others_radius null: every radius is 0.
// Before the first step the generator's `obstacles` are default-constructed (obstacle_generator.hpp:30): positions 0 and radii 0 -- the
// caller passes zeros and a null others_radius then.
LSC_HD void obstacle_chase_step(const ObstacleChaser &c, ObstacleChaserState &s, double t, const double goal[3], const double (*others_pos)[3],
                                const double *others_radius, int n_others, int self = -1)
{
#pragma clang fp contract(off)
    double a[3], v[3] = {s.vel[0], s.vel[1], s.vel[2]};
    for (int k = 0; k < 3; k++) a[k] = c.gamma_target * (goal[k] - s.pos[k]);                      // :280-284
    const double dt = t - s.t_last;                                                                // :288
    for (int o = 0; o < n_others; o++) {                                                           // :290-303
        if (o == self) continue;
        const double d[3] = {others_pos[o][0] - s.pos[0], others_pos[o][1] - s.pos[1], others_pos[o][2] - s.pos[2]};
        const double dist = obstacle_norm3(d);
        if (dist < OBSTACLE_EPS) continue;
        const double q = 2.0 * (c.radius + (others_radius ? others_radius[o] : 0.0));
        if (dist < q) {
            const double g = c.gamma_obs * (1.0 - dist / q) * (1.0 / (dist * q));
            for (int k = 0; k < 3; k++) a[k] += g * (-(d[k] / dist));
        }
    }
    const double an = obstacle_norm3(a), amax = c.max_acc - 0.01;                                  // :305-307
    if (an > amax)
        for (int k = 0; k < 3; k++) a[k] = a[k] / an * amax;
    for (int k = 0; k < 3; k++) v[k] = v[k] + a[k] * dt;                                           // :308
    const double vn = obstacle_norm3(v);                                                           // :309-311
    if (vn > c.max_vel)
        for (int k = 0; k < 3; k++) v[k] = v[k] / vn * c.max_vel;
    for (int k = 0; k < 3; k++) { s.pos[k] = s.pos[k] + v[k] * dt; s.vel[k] = v[k]; }              // :314-319
    s.t_last = t;                                                                                  // :325
}

// getGaussianObstacle (:388-434) with the history as an input: acc = the walker's own rows, [n_acc][3].  The caller has checked
// obstacle_walker_entries(w, t) <= n_acc.
LSC_HD void obstacle_gaussian_at(const ObstacleWalker &w, const double (*acc)[3], double t, double p[3], double vel[3])
{
#pragma clang fp contract(off)
    double v[3], vn[3];
    for (int k = 0; k < 3; k++) { p[k] = w.start[k]; vel[k] = v[k] = w.initial_vel[k]; }          // :390-391, :405
    const int n = (int)floor((t + OBSTACLE_EPS) / w.cycle);                                        // :401
    double dt = w.cycle;
    for (int i = 0; i < n + 1; i++) {                                                              // :408-431
        if (i == n) dt = t - (double)n * w.cycle;
        const double *ai = acc[i];
        for (int k = 0; k < 3; k++) vn[k] = v[k] + ai[k] * dt;
        if (obstacle_norm3(vn) > w.max_vel) {
            for (int k = 0; k < 3; k++) p[k] += v[k] * dt;                                         // (the entry is ignored: v and vel stay)
        } else {
            for (int k = 0; k < 3; k++) {
                p[k] += v[k] * dt + 0.5 * ai[k] * dt * dt;
                vel[k] += ai[k] * dt;
                v[k] = vn[k];
            }
        }
    }
}

// ---- the obstacle track: one row per tick of a recorded flight, beside the flight log's row (lsc_obstacle_record_kernel)
//   summary  16 B               double min_ratio (1e300 at reset) | int below_one (agent-time pairs with ratio < 1) | pad
//   states   float  [K][6]      what the stage wrote for this tick
//   ratio    double [T][N]      min over the obstacles of rule_distf(sample, obstacle) / (r_a + (double)(float) r_o)
//   partner  int    [T][N]      the FIRST obstacle attaining it
//   positions double [K][3]     the stage's positions before the rounding to float32 (what a simulator writes into its CSV: for straight
//                               and patrol the host's doubles), behind the parts above, on an 8-byte boundary
// rounded up to a multiple of 64 bytes.
constexpr int OBSTACLE_TRACK_SUMMARY_BYTES = 16;
constexpr double OBSTACLE_NO_RATIO = 1e300;
struct ObstacleTrackLayout { size_t states, ratio, partner, positions, row_bytes; };
LSC_HD ObstacleTrackLayout obstacle_track_layout(int N, int T, int K)
{
    const size_t tn = (size_t)T * (size_t)N;
    ObstacleTrackLayout l;
    size_t o = OBSTACLE_TRACK_SUMMARY_BYTES;
    l.states = o;  o += 24 * (size_t)K;
    l.ratio = o;   o += 8 * tn;
    l.partner = o; o += 4 * tn;
    o = (o + 7) / 8 * 8;
    l.positions = o; o += 24 * (size_t)K;
    l.row_bytes = (o + 63) / 64 * 64;
    return l;
}

}  // namespace lsc
