// extern "C" shim around the REFERENCE's Astar-3D (compiled from the reference checkout in place by oracle/Makefile;
// never copied).  Lets tests run AstarPlanner::plan on a flat occupancy grid via ctypes, and has the signature of the
// oracle's search hook (orc_astar_hook_fn, lsc_oracle.h) so that the oracle's goal stage can run with it in the loop.
#include <array>
#include <vector>

#include "Astar-3D/astarplanner.h"

// grid: int [ni][nj][nk], 0 = free.  path_out: int [max_len][3] (may be NULL with max_len 0).  *steps receives
// SearchResult::numberofsteps (one per pop, the pop of the goal included).  Returns the number of cells of lppath,
// or -1 when no path was found.  Cells beyond max_len are not written; the full length is returned all the same.
extern "C" int ref_astar(const int *grid, int ni, int nj, int nk, const int *start, const int *goal, int *path_out, int max_len,
                         long long *steps)
{
    std::vector<std::vector<std::vector<int>>> g(ni, std::vector<std::vector<int>>(nj, std::vector<int>(nk, 0)));
    for (int i = 0; i < ni; i++)
        for (int j = 0; j < nj; j++)
            for (int k = 0; k < nk; k++) g[i][j][k] = grid[((size_t)i * nj + j) * nk + k];
    AstarPlanner planner;
    EnvironmentOptions options;                      // the defaults, as GridBasedPlanner::planAstar passes them
    const SearchResult sr = planner.plan(g, {start[0], start[1], start[2]}, {goal[0], goal[1], goal[2]}, options);
    if (steps) *steps = (long long)sr.numberofsteps;
    if (!sr.pathfound || sr.lppath == nullptr) return -1;
    int n = 0;
    for (const Node &c : sr.lppath->List) {
        if (n < max_len) { path_out[3 * n] = c.i; path_out[3 * n + 1] = c.j; path_out[3 * n + 2] = c.z; }
        n++;
    }
    return n;
}
