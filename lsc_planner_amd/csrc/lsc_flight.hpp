// lsc_flight.hpp -- the simulator's per-tick accounting, each statement ONCE (file:line in the reference's src/ and include/).
//
// Value in, value out, like lsc_rules.hpp: the record kernel (lsc_flight.hip), the host routine that forms the Bernstein weights
// (lsc_flight_weights, lsc_abi.cpp) and the stand-alone host check of tests/test_flight_host.py call the same text (LSC_HD).
// Everything a sample needs beyond multiply-adds -- pow() of the weights, the segment of a time -- is formed on the host: the
// device's pow is not the host's, and the record has to be the bits the reference's simulator writes.
#pragma once
#include <math.h>
#include <stddef.h>

#include "lsc_rules.hpp"

namespace lsc {

constexpr int FLIGHT_SAMPLES = 1, FLIGHT_SAFETY = 2, FLIGHT_AGENTS = 4;     // LSC_FLIGHT_* of include/lsc_planner_amd.h
constexpr int FLIGHT_MAX_TIMES = 64;
constexpr int FLIGHT_SUMMARY_BYTES = 64;                                    // lsc_flight_tick
constexpr double FLIGHT_NO_PARTNER = 1e300;                                 // ratio of an agent without a partner (lsc_safety_kernel)
constexpr double FLIGHT_MOVED_EPS = 1e-5;                                   // SP_EPSILON_FLOAT, include/sp_const.hpp

// ---- layout of one log row: the summary, then the recorded parts, doubles first so that every part is aligned by construction.
//   summary  64 B                      lsc_flight_tick
//   ratio    double [T][N]             LSC_FLIGHT_SAFETY
//   cost     double [N]                LSC_FLIGHT_AGENTS
//   samples  float  [T][N][9]          LSC_FLIGHT_SAMPLES
//   end      float  [N][3]             LSC_FLIGHT_AGENTS
//   partner  int    [T][N]             LSC_FLIGHT_SAFETY
//   status   int    [N]                LSC_FLIGHT_AGENTS
// rounded up to a multiple of 64 bytes.
struct FlightLayout { size_t ratio, cost, samples, end, partner, status, row_bytes; };
LSC_HD FlightLayout flight_layout(int N, int T, int what)
{
    const size_t n = (size_t)N, tn = (size_t)T * n;
    FlightLayout l;
    size_t o = FLIGHT_SUMMARY_BYTES;
    l.ratio = o;   o += (what & FLIGHT_SAFETY) ? 8 * tn : 0;
    l.cost = o;    o += (what & FLIGHT_AGENTS) ? 8 * n : 0;
    l.samples = o; o += (what & FLIGHT_SAMPLES) ? 4 * 9 * tn : 0;
    l.end = o;     o += (what & FLIGHT_AGENTS) ? 4 * 3 * n : 0;
    l.partner = o; o += (what & FLIGHT_SAFETY) ? 4 * tn : 0;
    l.status = o;  o += (what & FLIGHT_AGENTS) ? 4 * n : 0;
    l.row_bytes = (o + 63) / 64 * 64;
    return l;
}

// nChoosek (include/polynomial.hpp:9-22)
LSC_HD int flight_choose(int n, int k)
{
    if (k > n) return 0;
    if (k * 2 > n) k = n - k;
    if (k == 0) return 1;
    int r = n;
    for (int i = 2; i <= k; i++) { r *= (n - i + 1); r /= i; }
    return r;
}

// The segment of sample time t (getStateFromControlPoints, include/polynomial.hpp:63-74): m = (int)(t / dt); exactly the horizon is the
// last segment at local parameter 1; -1: outside the horizon (the reference throws; a negative time is refused here too).
LSC_HD int flight_segment(double t, double dt)
{
    if (!(t >= 0.0)) return -1;
    const int m = (int)(t / dt);
    if (m == M && t < M * dt + 1e-9) return M - 1;
    return m >= M ? -1 : m;
}
LSC_HD double flight_local_time(double t, double dt, int m) { return t / dt - m; }

// Bernstein weights of degree n at local parameter tl, w[0..n] (getBernsteinBasis, include/polynomial.hpp:22-24): the
// reference's own expression.  A host function: no kernel calls it.
inline void flight_bernstein(int n, double tl, double *w)
{
    for (int i = 0; i <= n; i++) w[i] = flight_choose(n, i) * pow(tl, (double)i) * pow(1 - tl, (double)(n - i));
}

// getPointFromControlPoints (include/polynomial.hpp:26-45) along one axis: a double sum of float x double weight, rounded to float.
// c: the n + 1 control values of the axis, w: their weights.
LSC_HD float flight_point(const float *c, const double *w, int n)
{
#pragma clang fp contract(off)
    double x = 0.0;
    for (int i = 0; i <= n; i++) x += (double)c[i] * w[i];
    return (float)x;
}

// Velocity and acceleration control values of one axis of one segment (getStateFromControlPoints, include/polynomial.hpp:80-94):
//   v[i] = ((c[i+1] - c[i]) * 5f) * (float)pow(dt, -1),   a[i] = ((v[i+1] - v[i]) * 4f) * (float)pow(dt, -1)      in float32
// dt_inv = (float)pow(dt, -1), formed by the host.
LSC_HD void flight_derivative_points(const float *c, float dt_inv, float v[5], float a[4])
{
#pragma clang fp contract(off)
    for (int i = 0; i < DEG; i++) v[i] = ((c[i + 1] - c[i]) * (float)DEG) * dt_inv;
    for (int i = 0; i < DEG - 1; i++) a[i] = ((v[i + 1] - v[i]) * (float)(DEG - 1)) * dt_inv;
}

// One record sample of one axis: position, velocity, acceleration at a time whose weights are w5 / w4 / w3 (degrees 5, 4, 3).
// c: the six control values of the time's segment along the axis.
struct FlightAxisSample { float p, v, a; };
LSC_HD FlightAxisSample flight_axis_sample(const float *c, const double *w5, const double *w4, const double *w3, float dt_inv)
{
    float v[5], a[4];
    flight_derivative_points(c, dt_inv, v, a);
    return FlightAxisSample{flight_point(c, w5, DEG), flight_point(v, w4, DEG - 1), flight_point(a, w3, DEG - 2)};
}

// Position of an agent at a sample time from its plan (traj: the agent's [3][M*6] block, seg: the time's segment)
LSC_HD void flight_position(const float *traj, int seg, const double *w5, float p[3])
{
    for (int k = 0; k < 3; k++) p[k] = flight_point(traj + k * SEGV + seg * NC, w5, DEG);
}

// savePlanningResult's pair statement (src/multi_sync_simulator.cpp:446-503, distBetweenAgents include/util.hpp:225-229): the
// downwash of the pair mixed by the radii, the z difference divided by it in double and rounded to float, the float squared
// norm, and its double square root over the sum of the radii.
LSC_HD double flight_pair_ratio(const float *pa, const float *pb, double r_a, double dw_a, double r_b, double dw_b)
{
#pragma clang fp contract(off)
    const double dw = (dw_a * r_a + dw_b * r_b) / (r_a + r_b);
    const float dx = pa[0] - pb[0], dy = pa[1] - pb[1];
    const float dz = (float)((double)(pa[2] - pb[2]) / dw);
    const float n2 = dx * dx + dy * dy + dz * dz;
    return sqrt((double)n2) / (r_a + r_b);
}

// checkDeadlock's "moved" (src/traj_planner.cpp:396-409): the horizon end point is at least SP_EPSILON_FLOAT from the previous plan's;
// in the first tick there is no previous plan and every agent counts.
LSC_HD bool flight_moved(const float *end, const float *end_prev, int planner_seq)
{
    return planner_seq <= 1 || rule_distf(end, end_prev) >= FLIGHT_MOVED_EPS;
}

// The horizon end point traj[M-1][5] of a plan
LSC_HD void flight_end_point(const float *traj, float e[3])
{
    for (int k = 0; k < 3; k++) e[k] = traj[k * SEGV + (M - 1) * NC + DEG];
}

}  // namespace lsc
