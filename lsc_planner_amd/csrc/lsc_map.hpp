// lsc_map.hpp -- the products of the map, from an occupancy grid, each statement ONCE: the truncated exact Euclidean distance field
// (lsc_edt_from_bt, lsc_octomap.cpp), the blocked-cell integral images of the corridor kernel (build_integrals, lsc_abi.cpp) and the goal
// planner's static occupancy (build_goal_grid).  Value in, value out, like lsc_flight.hpp / lsc_obstacle_motion.hpp: the kernels of
// lsc_map.hip call these functions one lane per cell or per line, and tests/test_map_device_rules.py compiles the same text for the host.
//
// Why the bytes are the host path's.  Every product is an integer or the comparison of a float with a double:
//   distance field   integer squared lattice distances, min'ed with trunc2 = md^2, md = (int)(maxdist / res + 1).  The passes look
//                    +-(md - 1) cells along each axis only: when the nearest occupied cell is closer than md cells, each of its three
//                    offsets is at most md - 1, so the window holds it and the minimum is exact; when it is not, the windowed minimum
//                    is >= the true one >= trunc2 and both are truncated to trunc2.  The float of a cell is read from a table the HOST
//                    forms with lsc_edt_from_bt's own closing statement (map_edt_table_entry): the device takes no square root.
//   integral images  blocked = (double)edt < thr, thr a double the host forms; integer prefix sums are exact in any order.
//   goal occupancy   occupied = (double)edt_at(p) < thr; which field cell a grid index reads along an axis does not depend on the
//                    occupancy: the host forms the three index tables with build_goal_grid's statements (map_goal_cell), the kernel gathers.
// With md <= MAP_MD_MAX = 127 three passes stay below 3 * 126^2 = 47628 < MAP_FAR, the "nothing in the window" mark of the 16-bit passes.
#pragma once
#include <math.h>
#include <stddef.h>

#include "lsc_gjk.hpp"

namespace lsc {

constexpr int MAP_MD_MAX = 127;                    // largest truncation distance in cells
constexpr int MAP_BOXES_MAX = 64;                  // boxes of one lsc_map_update
constexpr unsigned MAP_FAR = 0xffffu;              // a pass found no occupied cell in its window

// the edits of one update, in call order (a later box wins); lo inclusive, hi exclusive, field cell indices
struct MapBoxes {
    int n;
    int box[MAP_BOXES_MAX][6];
    unsigned char value[MAP_BOXES_MAX];
};

// md of lsc_edt_from_bt
inline int map_truncation_cells(double maxdist, double res) { return (int)(maxdist / res + 1); }
// the float of squared lattice distance d2 (<= trunc2): the statement lsc_edt_from_bt ends with.  Host only.
inline float map_edt_table_entry(int d2, double res)
{
    const float cells = (float)sqrt((double)d2);
    return (float)((double)cells * res);
}
// which field cell grid index i reads along an axis (build_goal_grid: edt_at of the float32 grid point); -1: outside the field.  Host only.
inline int map_goal_cell(double grid_min, int i, double grid_res, double rf, int key_min, int n)
{
    const float p = (float)(grid_min + i * grid_res);
    const int c = (int)floor(rf * (double)p) + 32768 - key_min;
    return c < 0 || c >= n ? -1 : c;
}

// a cell's occupancy behind the edits
LSC_HD unsigned char map_edit_cell(unsigned char cur, int x, int y, int z, const MapBoxes &b)
{
    for (int i = 0; i < b.n; i++)
        if (x >= b.box[i][0] && x < b.box[i][3] && y >= b.box[i][1] && y < b.box[i][4] && z >= b.box[i][2] && z < b.box[i][5]) cur = b.value[i];
    return cur;
}

// One cell of a pass along a line of n cells (line[p * stride], p = 0 .. n - 1), at position q.
// first pass: squared distance to the nearest occupied cell of the line inside the window
LSC_HD unsigned map_edt_first(const unsigned char *line, size_t stride, int n, int q, int md)
{
    const int lo = q - (md - 1) < 0 ? 0 : q - (md - 1), hi = q + (md - 1) > n - 1 ? n - 1 : q + (md - 1);
    unsigned best = MAP_FAR;
    for (int p = lo; p <= hi; p++) {
        const unsigned d = (unsigned)((q - p) * (q - p));
        if (line[(size_t)p * stride] != 0 && d < best) best = d;
    }
    return best;
}
// later passes: min over the window of (the earlier passes' value + the squared offset along this axis)
LSC_HD unsigned map_edt_next(const unsigned short *line, size_t stride, int n, int q, int md)
{
    const int lo = q - (md - 1) < 0 ? 0 : q - (md - 1), hi = q + (md - 1) > n - 1 ? n - 1 : q + (md - 1);
    unsigned best = MAP_FAR;
    for (int p = lo; p <= hi; p++) {
        const unsigned v = line[(size_t)p * stride];
        const unsigned d = v + (unsigned)((q - p) * (q - p));
        if (v != MAP_FAR && d < best) best = d;
    }
    return best;
}
// the cell's distance in metres: table[min(d2, trunc2)] (MAP_FAR > trunc2)
LSC_HD float map_edt_value(unsigned d2, int trunc2, const float *table) { return table[d2 < (unsigned)trunc2 ? d2 : (unsigned)trunc2]; }

// build_integrals' predicate; thr = r + 0.5 world_resolution - 1e-5 in the host's doubles
LSC_HD int map_blocked(float edt, double thr) { return (double)edt < thr ? 1 : 0; }

// Integral image I [(nx+1)][(ny+1)][(nz+1)] in three scans.  z: line (x, y), x = 0 .. nx, y = 0 .. ny, writes every entry of the line
// (zeros on the planes x = 0, y = 0, z = 0); then y and x: in-place running sums along a line of n + 1 entries that starts with 0.
LSC_HD void map_integral_scan_z(const float *edt, int *I, int nx, int ny, int nz, int x, int y, double thr)
{
    int *line = I + ((size_t)x * (ny + 1) + y) * (nz + 1);
    int sum = 0;
    line[0] = 0;
    for (int z = 1; z <= nz; z++) {
        if (x > 0 && y > 0) sum += map_blocked(edt[((size_t)(x - 1) * ny + (y - 1)) * nz + (z - 1)], thr);
        line[z] = sum;
    }
}
LSC_HD void map_integral_scan(int *line, size_t stride, int n)
{
    int sum = 0;
    for (int p = 1; p <= n; p++) {
        sum += line[(size_t)p * stride];
        line[(size_t)p * stride] = sum;
    }
}

// build_goal_grid's predicate for the grid cell whose field cell is (cx, cy, cz), -1 on an axis: outside, reads -1;
// thr = r + (double)(float)grid_margin in the host's doubles
LSC_HD unsigned char map_goal_occupied(const float *edt, int ny, int nz, int cx, int cy, int cz, double thr)
{
    const float e = cx < 0 || cy < 0 || cz < 0 ? -1.0f : edt[((size_t)cx * ny + cy) * nz + cz];
    return (double)e < thr ? 1 : 0;
}

}  // namespace lsc
