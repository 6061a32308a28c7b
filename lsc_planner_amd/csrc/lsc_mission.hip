// lsc_mission.hip -- the goal stage: what TrajPlanner::goalPlanning does in front of its goal mode (src/traj_planner.cpp:477-509), for
// the whole swarm, as the first launch of a tick.
//
//   PATROL   an agent that has arrived swaps its desired goal and its start       (:479-485)  -> desired, start, legs
//   GOBACK   every agent flies to the mission's start, on every tick              (:486-490)  -> desired, start
//   right-hand rule: a deadlocked agent's goal moves to its right                 (:528-538, isDeadlock :1733-1740)  -> rule_goal
//
// Shape.  One lane per agent, 256 lanes per workgroup, no LDS, no atomics: an agent's rows of the tables are read and written by its
// lane alone, with plain vector loads and stores.  Every statement is a rule of lsc_rules.hpp.  The tables are read by the launches
// BEHIND this one (neighbour lists, goal search, corridor, plan kernel, flight record), which the stream orders.
#include "lsc_kernels.h"
#include "lsc_rules.hpp"

namespace lsc {

constexpr int MT = 256;                        // lanes of a stage workgroup

__global__ __launch_bounds__(MT) void lsc_mission_kernel(const MissionArgs a)
{
#pragma clang fp contract(off)
    const int q = blockIdx.x * MT + threadIdx.x;
    if (q >= a.N) return;
    const float *s = a.state + 9 * (size_t)q;
    const float pos[3] = {s[0], s[1], s[2]}, vel[3] = {s[3], s[4], s[5]};
    float des[3];
    if (a.desired) {
        float *d = a.desired + 3 * (size_t)q, *st = a.start + 3 * (size_t)q;
        des[0] = d[0]; des[1] = d[1]; des[2] = d[2];
        bool changed = false;
        MissionLeg leg;
        if (a.planner_state == MISSION_PATROL && rule_patrol_arrived(des, pos, a.goal_threshold)) {
            const float from[3] = {st[0], st[1], st[2]};
            leg = rule_patrol_swap(des, from);
            a.legs[q] = a.legs[q] + 1;
            changed = true;
        } else if (a.planner_state == MISSION_GOBACK) {
            leg = rule_goback_leg(a.mission_start + 3 * (size_t)q, a.mission_goal + 3 * (size_t)q);
            changed = true;
        }
        if (changed) {
            des[0] = leg.desired.x; des[1] = leg.desired.y; des[2] = leg.desired.z;
            d[0] = des[0]; d[1] = des[1]; d[2] = des[2];
            st[0] = leg.start.x; st[1] = leg.start.y; st[2] = leg.start.z;
        }
    } else {
        const float *g = a.goal_in + 3 * (size_t)q;
        des[0] = g[0]; des[1] = g[1]; des[2] = g[2];
    }
    if (a.rule_goal) {
        float *o = a.rule_goal + 3 * (size_t)q;
        if (rule_deadlock(pos, vel, des, a.planner_seq, a.seq_threshold, a.velocity_threshold, a.goal_threshold)) {
            const F3 g = rule_right_hand_goal(pos, des);
            o[0] = g.x; o[1] = g.y; o[2] = g.z;
        } else {                                                      // goalPlanningWithStaticGoal
            o[0] = des[0]; o[1] = des[1]; o[2] = des[2];
        }
    }
}

hipError_t launch_mission(const MissionArgs &a, hipStream_t st)
{
    if (a.N < 1 || !a.state || (!a.desired && !a.goal_in) || (a.desired && (!a.start || !a.mission_start || !a.mission_goal || !a.legs)))
        return hipErrorInvalidValue;
    return launch_variant(kernel_address(lsc_mission_kernel), dim3((a.N + MT - 1) / MT), dim3(MT), 0, st, a);
}

}  // namespace lsc
