// lsc_rules.hpp -- the small arithmetic rules taken over from the reference, each stated ONCE (file:line in the reference's src/).
//
// Value in, value out: floats or `const float *` to three floats, thresholds as doubles; no argument blocks, no shared memory, no
// lane ids -- a wave that holds its inputs in registers and a kernel that reads them through pointers call the same text, and so
// does the host (LSC_HD).  The float32 rules are octomath's: differences, products and sums in float without contraction, the
// square root in double.  tests/native/rules_host_check.cpp strings these functions together in the reference's sequential order
// and tests/test_host_layer.py holds the result to the oracle bit for bit, without a GPU.
#pragma once
#include <math.h>
#include <stddef.h>

#include "lsc_gjk.hpp"
#include "lsc_model.hpp"

namespace lsc {

// octomath::Vector3::distance (every distance of goalPlanningWithPriority and of the disturbance checks)
LSC_HD double rule_distf(const float *p, const float *q)
{
#pragma clang fp contract(off)
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    const float n2 = dx * dx + dy * dy + dz * dz;
    return sqrt((double)n2);
}

// obstaclePredictionCheck / initialTrajPlanningCheck (traj_planner.cpp:866-878, 1047-1061): an agent whose position is farther than
// reset_threshold from where its plan puts it now -- the first point of its shifted previous plan -- is off its plan.  (Whether the checks
// run at all -- reset_threshold > 0, planner_seq >= 2, LSC mode -- is the caller's business.)
LSC_HD bool rule_off_plan(const float *plan_now, const float *pos, double reset_threshold)
{
    return rule_distf(plan_now, pos) > reset_threshold;
}

// The mission's own test of an agent's goal (isFinished, multi_sync_simulator.cpp:358-380; the deadlock bookkeeping, traj_planner.cpp:396-409):
// farther than goal_threshold from it
LSC_HD bool rule_goal_unmet(const float *pos, const float *goal, double goal_threshold)
{
    return rule_distf(pos, goal) > goal_threshold;
}

// goalPlanning's patrol test (traj_planner.cpp:479-480): a patrolling agent has arrived at its desired goal -- STRICTLY closer than
// goal_threshold.  (rule_goal_unmet is strictly farther: exactly at the threshold an agent neither swaps nor counts as unmet.)
LSC_HD bool rule_patrol_arrived(const float *desired, const float *pos, double goal_threshold)
{
#pragma clang fp contract(off)
    return rule_distf(desired, pos) < goal_threshold;
}

// The two ends of the leg an agent flies: where it wants to go and where it came from (Agent::desired_goal_position, start_position)
struct MissionLeg { F3 desired, start; };
// ... of an agent that has arrived while patrolling (traj_planner.cpp:481-484): the ends trade places
LSC_HD MissionLeg rule_patrol_swap(const float *desired, const float *start)
{
    return MissionLeg{F3{start[0], start[1], start[2]}, F3{desired[0], desired[1], desired[2]}};
}
// ... in PlannerState::GOBACK (traj_planner.cpp:486-490), on every tick: home is the MISSION's start, whatever leg the agent was on
LSC_HD MissionLeg rule_goback_leg(const float *mission_start, const float *mission_goal)
{
    return MissionLeg{F3{mission_start[0], mission_start[1], mission_start[2]}, F3{mission_goal[0], mission_goal[1], mission_goal[2]}};
}

// isDeadlock (traj_planner.cpp:1733-1740, the velocity test; deadlock_seq_threshold 5 and deadlock_velocity_threshold 0.1 in
// param.cpp:79-80): the agent has planned more than seq_threshold times, is slower than velocity_threshold and farther than
// goal_threshold from its desired goal
LSC_HD bool rule_deadlock(const float *pos, const float *vel, const float *desired, int planner_seq, int seq_threshold,
                          double velocity_threshold, double goal_threshold)
{
#pragma clang fp contract(off)
    const double dist_to_goal = rule_distf(pos, desired);
    const float v2 = vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2];
    return planner_seq > seq_threshold && sqrt((double)v2) < velocity_threshold && dist_to_goal > goal_threshold;
}

// goalPlanningWithRightHandRule's goal of a deadlocked agent (traj_planner.cpp:531-533): pos + (desired - pos).cross((0, 0, 1)), the
// cross product as octomath::Vector3::cross states it (y b.z - z b.y, z b.x - x b.z, x b.y - y b.x) with b = (0, 0, 1)
LSC_HD F3 rule_right_hand_goal(const float *pos, const float *desired)
{
#pragma clang fp contract(off)
    const float dx = desired[0] - pos[0], dy = desired[1] - pos[1], dz = desired[2] - pos[2];
    const float bx = 0.0f, by = 0.0f, bz = 1.0f;
    const float cx = dy * bz - dz * by, cy = dz * bx - dx * bz, cz = dx * by - dy * bx;
    return F3{pos[0] + cx, pos[1] + cy, pos[2] + cz};
}

// goalPlanningWithPriority (traj_planner.cpp:547-577): whether another agent (position opos, desired goal ogoal, last and first end point
// of its unshifted previous plan) has priority over the agent at pos, dist_to_goal from its own goal.  dist_to_obs is what the retreat
// rule minimises over those that have (:569-575, first strict minimum in agent order).
LSC_HD bool rule_has_priority(const float *pos, double dist_to_goal, const float *opos, const float *ogoal, const float *oprev_last,
                              const float *oprev_first, double goal_threshold, double &dist_to_obs)
{
#pragma clang fp contract(off)
    const double obs_dist_to_goal = rule_distf(opos, ogoal);
    dist_to_obs = rule_distf(opos, pos);
    if (obs_dist_to_goal < goal_threshold) return false;                                 // :560-562
    const float ax = oprev_last[0] - oprev_first[0], ay = oprev_last[1] - oprev_first[1], az = oprev_last[2] - oprev_first[2];
    const float bx = oprev_first[0] - pos[0], by = oprev_first[1] - pos[1], bz = oprev_first[2] - pos[2];
    const float dp = ax * bx + ay * by + az * bz;
    if (dist_to_goal > goal_threshold && (double)dp > 0.0) return false;                 // same direction :564-566
    return dist_to_goal < goal_threshold || obs_dist_to_goal < dist_to_goal;
}

// the retreat goal (traj_planner.cpp:580-587): priority_dist_threshold + 0.1 away from the closest agent that has priority
LSC_HD F3 rule_retreat_goal(const float *pos, const float *opos, double priority_dist_threshold)
{
#pragma clang fp contract(off)
    const F3 dir = normalized_f32(F3{opos[0] - pos[0], opos[1] - pos[1], opos[2] - pos[2]});
    const float keep = (float)(priority_dist_threshold + 0.1);
    return F3{pos[0] - dir.x * keep, pos[1] - dir.y * keep, pos[2] - dir.z * keep};
}

// findLOSFreeGoal (traj_planner.cpp:350-407) on an empty map, where every line of sight is free: the desired goal, clamped to goal_radius
// from the end of the initial trajectory
LSC_HD F3 rule_los_free_goal(const float *goal, const float *end, double goal_radius)
{
#pragma clang fp contract(off)
    F3 delta = F3{goal[0] - end[0], goal[1] - end[1], goal[2] - end[2]};
    const float n2 = delta.x * delta.x + delta.y * delta.y + delta.z * delta.z;
    if (!(sqrt((double)n2) > goal_radius)) return F3{goal[0], goal[1], goal[2]};
    delta = normalized_f32(delta);
    const float r = (float)goal_radius;
    return F3{end[0] + delta.x * r, end[1] + delta.y * r, end[2] + delta.z * r};
}

// getTerminalSegments (traj_optimizer.cpp:541-548): the segments whose end point the terminal cost pulls to the goal
LSC_HD int rule_terminal_segments(const float *goal, const float *pos, double v_nom, double dt)
{
#pragma clang fp contract(off)
    const double flight = rule_distf(goal, pos) / v_nom;
    const int T = (int)((M * dt - flight + 1e-9) / dt);
    return T > 1 ? T : 1;
}

// The control points the current state fixes, per axis (traj_optimizer.cpp:394-405, solved for c_{0,0..2}; lsc_model.hpp): hv = dt / n,
// ha = dt^2 / (n (n - 1)).  pinned: the z axis of a planar world, which rests at z_2d (:87-90, 239-259).
LSC_HD void rule_state_constants(float p, float v, float acc, double hv, double ha, bool pinned, double z2d, double &c0, double &c1, double &c2)
{
    c0 = (double)p;
    c1 = c0 + (double)v * hv;
    c2 = (double)acc * ha + 2.0 * c1 - c0;
    if (pinned) c0 = c1 = c2 = z2d;
}

// Box bounds of one segment along axis k (traj_optimizer.cpp:274-303, 406-435): the world box, cut by the segment's corridor box
// (min[3] | max[3]; read only when there are corridors: boxed) where the segment is held to one (opt/N_constraint_segments)
LSC_HD void rule_box_bounds(float world_min, float world_max, const float *box, bool boxed, int k, bool held, double &lo, double &hi)
{
    lo = (double)world_min; hi = (double)world_max;
    if (boxed && held) {
        lo = fmax(lo, (double)box[k]);
        hi = fmin(hi, (double)box[3 + k]);
    }
}

// isObstacleInBox along ONE axis (include/corridor_constructor.hpp:81-122), in cells of the distance field.  The reference visits the lattice
// points lo, lo + res, ... of a slab [lo, hi], each formed in float32 and nudged by a float 1e-5: the first one downwards (unless the box
// sits on the world boundary wmin), all others upwards; a slab of one point is visited twice, down and up.  A cell is (int)floor(rf * sample)
// + 32768 - kmin (OcTreeBaseImpl::coordToKey; rf = 1 / map resolution, kmin the key of the field's cell 0).  The visited cells are {a0} u
// [b0, b1] -- the cell just above `lo` is skipped by the reference -- as long as the nudged samples fall into consecutive cells: that needs
// the nudge to survive the float32 addition, |sample| < 256 m (there a float32 step is 3.05e-5 m and `x + 1e-5f` rounds back to x, so the
// reference's run of cells has holes that [b0, b1] has not).  lsc_set_distmap refuses worlds beyond that bound;
// tests/native/sfc_host_check.cpp and tests/test_sfc_axis_cells.py walk every lattice index below it against the literal samples.
constexpr double SFC_WORLD_REACH_MAX = 256.0;    // max(|world_min|, |world_max|) + world_resolution stays below this (metres)
struct SfcAxisCells { int a0, b0, b1; };
LSC_HD SfcAxisCells rule_sfc_axis_cells(double lo, double hi, double wres, double rf, int kmin, double wmin)
{
#pragma clang fp contract(off)
    const int size = (int)round((hi - lo) / wres) + 1;
    const int last = (size > 2 ? size : 2) - 1;
    const float d0 = (lo > wmin + 1e-5) ? (float)-1e-5 : (float)1e-5;
    const float p0 = (float)lo + d0;
    const float p1 = ((size == 1) ? (float)lo : (float)(lo + 1 * wres)) + (float)1e-5;
    const float pl = ((size == 1) ? (float)lo : (float)(lo + last * wres)) + (float)1e-5;
    SfcAxisCells c;
    c.a0 = (int)floor(rf * (double)p0) + 32768 - kmin;
    c.b0 = (int)floor(rf * (double)p1) + 32768 - kmin;
    c.b1 = (int)floor(rf * (double)pl) + 32768 - kmin;
    if (c.b1 < c.b0) { const int t = c.b0; c.b0 = c.b1; c.b1 = t; }
    return c;
}

// Axis-row slot sl = type * NV + k * SEGV + m * NC + i: type 0/1 upper / lower bound of c_{m,i}, 2/3 velocity difference, 4/5 acceleration difference
struct AxisSlot { int type, k, m, i; };
LSC_HD AxisSlot axis_slot_of(int sl)
{
    const int kt = sl % NV, t = kt % SEGV;
    return AxisSlot{sl / NV, kt / SEGV, t / NC, t % NC};
}
// Whether the row of a slot exists (traj_optimizer.cpp:274-303, 468-525: none on what the state fixes, none across the horizon's end, and
// `for (k < dim)` in a planar world) and its right-hand side h, from the bounds of the slot's segment and the limits of its axis
LSC_HD bool rule_axis_row(const AxisSlot &s, bool planar, double hi, double lo, double vlim, double alim, double &h)
{
    bool valid;
    if (s.type < 2) { valid = !(s.m == 0 && s.i < 3); h = s.type == 0 ? hi : -lo; }
    else if (s.type < 4) { valid = s.i <= 4 && !(s.m == 0 && s.i < 2); h = vlim; }
    else { valid = s.i <= 3 && !(s.m == 0 && s.i == 0); h = alim; }
    if (planar && s.k == 2) valid = false;
    return valid;
}

// Control point (m, i) along axis k of an agent's own initial trajectory (initialTrajPlanning, traj_planner.cpp:997-1037):
//   at_rest         : the current position (after a disturbance reset, and in BVC mode)
//   planner_seq < 2 : pos + vel * m_intp * dt
//   else            : the previous plan (prev_k: its axis k) shifted by one segment, the last segment resting at its end point
LSC_HD float rule_initial_point(const float *state, const float *prev_k, int k, int m, int i, int planner_seq, bool at_rest, float dtf)
{
#pragma clang fp contract(off)
    if (at_rest) return state[k];
    if (planner_seq < 2) {
        const float mi = (float)((double)m + (double)i / (double)DEG);
        return state[k] + (state[3 + k] * mi) * dtf;
    }
    return (m < M - 1) ? prev_k[(m + 1) * NC + i] : prev_k[(M - 1) * NC + DEG];
}

// Predicted / initial control points of agent q for segment m (obstaclePredictionWithPrevSol / initialTrajPlanningPrevSol,
// traj_planner.cpp:699-712, 829-864, 1030-1037).
//   planner_seq < 2 : pos + vel * m_intp * dt
//   else            : previous plan shifted by one segment, last segment = 6 x previous end point
LSC_HD void load_segment(const float *__restrict__ state, const float *__restrict__ traj_prev, int q, int m, int planner_seq, float dtf, F3 out[6])
{
#pragma clang fp contract(off)   // float32 semantics of octomath::Vector3: no fused multiply-add
    if (planner_seq < 2) {
        const float *s = state + 9 * q;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            float mi = (float)((double)m + (double)i / (double)DEG);
            float ax = (s[3] * mi) * dtf, ay = (s[4] * mi) * dtf, az = (s[5] * mi) * dtf;
            out[i] = F3{s[0] + ax, s[1] + ay, s[2] + az};
        }
    } else {
        const float *t = traj_prev + (size_t)q * NV;
        if (m < M - 1) {
#pragma unroll
            for (int i = 0; i < 6; i++) {
                int c = (m + 1) * NC + i;
                out[i] = F3{t[c], t[SEGV + c], t[2 * SEGV + c]};
            }
        } else {
            int c = (M - 1) * NC + DEG;
            F3 e = F3{t[c], t[SEGV + c], t[2 * SEGV + c]};
#pragma unroll
            for (int i = 0; i < 6; i++) out[i] = e;
        }
    }
}

// Downwash of the pair (agent, obstacle oi) that scales the z axis of both trajectories (generateLSC, traj_planner.cpp:1339-1345): the
// radius-weighted mean of the two downwash values for a cooperating agent; for any other obstacle (ObstacleType::DYNAMICOBSTACLE) the
// planning agent's own downwash does not enter, its radius does
LSC_HD double rule_pair_downwash(double r_a, double dw_a, double r_o, double dw_o, bool obstacle_is_agent)
{
#pragma clang fp contract(off)
    if (obstacle_is_agent) return (dw_a * r_a + dw_o * r_o) / (r_a + r_o);
    return (r_a + dw_o * r_o) / (r_a + r_o);
}

// Predicted control points of a non-agent obstacle for segment m (obstaclePredictionWithPrevSol, traj_planner.cpp:838-846, and
// obstaclePredictionWithCurrVel behind :830-833): pos + vel * m_intp * dt from its current position and velocity (pos_vel: three floats
// each) at EVERY planner_seq -- such an obstacle has no previous plan to shift
LSC_HD void rule_obstacle_segment(const float *__restrict__ pos_vel, int m, float dtf, F3 out[6])
{
#pragma clang fp contract(off)   // float32 semantics of octomath::Vector3: no fused multiply-add
#pragma unroll
    for (int i = 0; i < 6; i++) {
        float mi = (float)((double)m + (double)i / (double)DEG);
        float ax = (pos_vel[3] * mi) * dtf, ay = (pos_vel[4] * mi) * dtf, az = (pos_vel[5] * mi) * dtf;
        out[i] = F3{pos_vel[0] + ax, pos_vel[1] + ay, pos_vel[2] + az};
    }
}

// Segments over which a non-agent obstacle's predicted size grows (obstacleSizePredictionWithConstAcc, traj_planner.cpp:882):
// M_u = int((obs/uncertainty_horizon + SP_EPSILON) / dt), SP_EPSILON = 1e-9 (include/sp_const.hpp)
LSC_HD int rule_uncertainty_segments(double uncertainty_horizon, double dt)
{
#pragma clang fp contract(off)
    return (int)((uncertainty_horizon + 1e-9) / dt);
}

// Predicted size of a non-agent obstacle at control point (m, i) (obstacleSizePredictionWithConstAcc, traj_planner.cpp:880-919): with
// obs/size_prediction the radius plus what max_acc can move the obstacle off its constant-velocity prediction -- for a segment m < M_u the
// degree-5 Bernstein control points of 0.5 a dt^2 (m + t)^2 on t in [0, 1], which are 0.5 a dt^2 (m^2 + 2 m i / n + i (i - 1) / (n (n - 1)))
// (the reference multiplies the monomial coefficients by a numerically inverted basis matrix, include/polynomial.hpp:427: this closed
// form is the statement here); from M_u on the growth rests at 0.5 a (M_u dt)^2.  Without size prediction: the radius.
LSC_HD double rule_obstacle_size(double r_o, double max_acc, double dt, int M_u, bool size_prediction, int m, int i)
{
#pragma clang fp contract(off)
    if (!size_prediction) return r_o;
    const double half_a = 0.5 * max_acc;
    if (m >= M_u) {
        const double T = (double)M_u * dt;
        return r_o + half_a * (T * T);
    }
    const double md = (double)m, id = (double)i, n = (double)DEG;
    const double poly = (md * md + (2.0 * md * id) / n) + (id * (id - 1.0)) / (n * (n - 1.0));
    return r_o + (half_a * (dt * dt)) * poly;
}

// Margin of a row against a non-agent obstacle that is in the agent's slack set (generateLSC's "reciprocal RSFC" branch,
// traj_planner.cpp:1395-1400): not half of the separation -- the obstacle's whole predicted size plus the agent's radius.  (An agent in
// the slack set keeps the half-separation margin of lsc_segment, :1388-1394.)
LSC_HD double rule_slack_obstacle_margin(double predicted_size, double r_a)
{
#pragma clang fp contract(off)
    return predicted_size + r_a;
}

}  // namespace lsc
