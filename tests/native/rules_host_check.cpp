// Test-only: compiles the product's rules header (csrc/lsc_rules.hpp) for the HOST and strings its functions together in the
// reference's sequential order -- agents in index order, first strict minimum -- so that the CPU test-suite can hold them to the
// oracle bit for bit without a GPU.  Not part of the product library.  Built once per segment count (-DLSC_SEGMENTS=4).
#include <cmath>
#include "../../lsc_planner_amd/csrc/lsc_rules.hpp"

using namespace lsc;

extern "C" int ruleshdr_segments() { return M; }

// current goal of every agent, mode/goal = prior_based on an empty map; branch[q]: 0 the goal as given, 1 clamped to goal_radius, 2 retreat
extern "C" void ruleshdr_goals(int N, const float *state, const float *goal, const float *prev, int planner_seq, double dt, double goal_threshold,
                               double priority_dist_threshold, double goal_radius, float *out, int *branch)
{
    const int cl = (M - 1) * NC + DEG, cf = DEG;
    for (int qi = 0; qi < N; qi++) {
        const float *pos = state + 9 * qi, *goal_i = goal + 3 * qi;
        const double dist_to_goal = rule_distf(pos, goal_i);
        double best = 1e9;
        int bq = -1;
        for (int qj = 0; qj < N; qj++) {
            if (qj == qi) continue;
            const float *pt = prev + (size_t)qj * NV;
            const float tl[3] = {pt[cl], pt[SEGV + cl], pt[2 * SEGV + cl]}, tf[3] = {pt[cf], pt[SEGV + cf], pt[2 * SEGV + cf]};
            double d;
            if (rule_has_priority(pos, dist_to_goal, state + 9 * qj, goal + 3 * qj, tl, tf, goal_threshold, d) && d < best) { best = d; bq = qj; }
        }
        F3 g;
        if (best < priority_dist_threshold) {
            g = rule_retreat_goal(pos, state + 9 * bq, priority_dist_threshold);
            branch[qi] = 2;
        } else {
            float end[3];
            for (int k = 0; k < 3; k++) end[k] = rule_initial_point(pos, prev + (size_t)qi * NV + k * SEGV, k, M - 1, DEG, planner_seq, false, (float)dt);
            g = rule_los_free_goal(goal_i, end, goal_radius);
            branch[qi] = (g.x == goal_i[0] && g.y == goal_i[1] && g.z == goal_i[2]) ? 0 : 1;
        }
        out[3 * qi] = g.x; out[3 * qi + 1] = g.y; out[3 * qi + 2] = g.z;
    }
}

// the two disturbance checks at planner_seq >= 2: whether each agent is off its (shifted previous) plan
extern "C" void ruleshdr_off_plan(int N, const float *state, const float *prev, double reset_threshold, unsigned char *off)
{
    for (int q = 0; q < N; q++) {
        const float *t = prev + (size_t)q * NV + NC;
        const float t1[3] = {t[0], t[SEGV], t[2 * SEGV]};
        off[q] = rule_off_plan(t1, state + 9 * q, reset_threshold) ? 1 : 0;
    }
}

extern "C" int ruleshdr_terminal_segments(const float *goal, const float *pos, double v_nom, double dt)
{
    return rule_terminal_segments(goal, pos, v_nom, dt);
}

// an agent's own initial trajectory [3][SEGV]
extern "C" void ruleshdr_initial_traj(const float *state, const float *prev, int planner_seq, int at_rest, double dt, float *out)
{
    for (int k = 0; k < 3; k++)
        for (int m = 0; m < M; m++)
            for (int i = 0; i < NC; i++)
                out[k * SEGV + m * NC + i] = rule_initial_point(state, prev + k * SEGV, k, m, i, planner_seq, at_rest != 0, (float)dt);
}
