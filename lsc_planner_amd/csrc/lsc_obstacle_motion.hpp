// lsc_obstacle_motion.hpp -- getObstacle(t) of the reference's include/obstacle.hpp for the three obstacle types whose motion is a closed
// form of the time alone, each statement ONCE: straight (:123-173), spin (:68-121), multisim_patrol (:175-231).
//
// Value in, value out, like lsc_rules.hpp / lsc_flight.hpp: the obstacle stage (lsc_obstacles.hip), the installation of the table
// (lsc_obstacle_motion, lsc_abi.cpp) and the stand-alone host check of tests/test_obstacle_motion_device_rules.py call the same text (LSC_HD).
// The statements are ObstacleMotion's (host/lsc_host.hpp), which the simulator feeds its ticks with today:
//
//   straight, patrol   + - x / sqrt and comparisons only, every one correctly rounded on host and device, nothing contracted: the same
//                      bits as ObstacleMotion::at.
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
