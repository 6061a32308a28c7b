// lsc_map.hip -- the map's products on the device, from an occupancy grid (lsc_set_occupancy, lsc_map_update): the distance field,
// the corridor kernel's integral images and the goal planner's static occupancy.  What lsc_edt_from_bt + build_integrals +
// build_goal_grid compute on the host, to the same bytes (the argument is in lsc_map.hpp, whose statements these kernels call).
//
// Shape.  One lane per cell (the passes, the edits, the goal occupancy) or per line (the scans of the integral images), 256 lanes per
// workgroup, no LDS, no atomics, plain vector loads and stores.  Lanes run over the flattened index with z fastest, so the loads of
// the y and x passes and of the y and x scans are coalesced; the z pass and the z scan read their own line.  Every update rebuilds the
// whole grid: the chain is about eight small dependent launches which the stream orders, each lane's window is at most 2 md - 1 loads.
// Every index is formed in size_t and every lane checks its bound before it touches memory.
#include "lsc_kernels.h"
#include "lsc_map.hpp"

namespace lsc {

constexpr int MAPT = 256;                      // lanes of a workgroup

struct MapEditArgs {
    unsigned char *occ;
    int nx, ny, nz;
    MapBoxes boxes;
};

__global__ __launch_bounds__(MAPT) void lsc_map_edit_kernel(const MapEditArgs a)
{
    const size_t i = (size_t)blockIdx.x * MAPT + threadIdx.x, cells = (size_t)a.nx * a.ny * a.nz;
    if (i >= cells) return;
    const int z = (int)(i % a.nz), y = (int)(i / a.nz % a.ny), x = (int)(i / a.nz / a.ny);
    a.occ[i] = map_edit_cell(a.occ[i], x, y, z, a.boxes);
}

// axis 2: occ -> pass_a along z; axis 1: pass_a -> pass_b along y; axis 0: pass_b -> edt along x
template <int AXIS>
__global__ __launch_bounds__(MAPT) void lsc_map_edt_kernel(const MapArgs a)
{
    const size_t i = (size_t)blockIdx.x * MAPT + threadIdx.x, cells = (size_t)a.nx * a.ny * a.nz;
    if (i >= cells) return;
    const int z = (int)(i % a.nz), y = (int)(i / a.nz % a.ny), x = (int)(i / a.nz / a.ny);
    if (AXIS == 2) {
        a.pass_a[i] = (unsigned short)map_edt_first(a.occ + (i - z), 1, a.nz, z, a.md);
    } else if (AXIS == 1) {
        a.pass_b[i] = (unsigned short)map_edt_next(a.pass_a + (i - (size_t)y * a.nz), (size_t)a.nz, a.ny, y, a.md);
    } else {
        const size_t plane = (size_t)a.ny * a.nz;
        a.edt[i] = map_edt_value(map_edt_next(a.pass_b + (i - (size_t)x * plane), plane, a.nx, x, a.md), a.trunc2, a.table);
    }
}

// blockIdx.y: the radius.  axis 2: lines (x, y) of the image, from the field; axis 1: lines (x, z); axis 0: lines (y, z)
template <int AXIS>
__global__ __launch_bounds__(MAPT) void lsc_map_integral_kernel(const MapArgs a)
{
    const size_t l = (size_t)blockIdx.x * MAPT + threadIdx.x;
    const int r = blockIdx.y, X = a.nx + 1, Y = a.ny + 1, Z = a.nz + 1;
    int *I = a.integral + (size_t)r * X * Y * Z;
    if (AXIS == 2) {
        if (l >= (size_t)X * Y) return;
        map_integral_scan_z(a.edt, I, a.nx, a.ny, a.nz, (int)(l / Y), (int)(l % Y), a.thr_blocked[r]);
    } else if (AXIS == 1) {
        if (l >= (size_t)X * Z) return;
        map_integral_scan(I + (l / Z) * Y * Z + l % Z, (size_t)Z, a.ny);
    } else {
        if (l >= (size_t)Y * Z) return;
        map_integral_scan(I + l, (size_t)Y * Z, a.nx);
    }
}

__global__ __launch_bounds__(MAPT) void lsc_map_goal_kernel(const MapArgs a)
{
    const size_t g = (size_t)blockIdx.x * MAPT + threadIdx.x, C = (size_t)a.H * a.W * a.A;
    if (g >= C) return;
    const int r = blockIdx.y;
    const int j = (int)(g % a.W), i = (int)(g / a.W % a.H), k = (int)(g / a.W / a.H);      // index H W k + W i + j
    a.goal_occ[(size_t)r * C + g] = map_goal_occupied(a.edt, a.ny, a.nz, a.cell_of[i], a.cell_of[a.H + j], a.cell_of[a.H + a.W + k], a.thr_goal[r]);
}

static dim3 map_grid(size_t lanes, int rows = 1) { return dim3((unsigned)((lanes + MAPT - 1) / MAPT), (unsigned)rows); }

hipError_t launch_map_edit(unsigned char *occ, int nx, int ny, int nz, const MapBoxes &boxes, hipStream_t st)
{
    if (!occ || nx < 1 || ny < 1 || nz < 1 || boxes.n < 0 || boxes.n > MAP_BOXES_MAX) return hipErrorInvalidValue;
    if (boxes.n == 0) return hipSuccess;
    MapEditArgs a;
    a.occ = occ; a.nx = nx; a.ny = ny; a.nz = nz; a.boxes = boxes;
    return launch_variant(kernel_address(lsc_map_edit_kernel), map_grid((size_t)nx * ny * nz), dim3(MAPT), 0, st, a);
}

hipError_t launch_map_build(const MapArgs &a, hipStream_t st)
{
    if (a.nx < 1 || a.ny < 1 || a.nz < 1 || a.md < 1 || a.md > MAP_MD_MAX || a.trunc2 != a.md * a.md || !a.occ || !a.pass_a || !a.pass_b || !a.table || !a.edt)
        return hipErrorInvalidValue;
    if (a.n_radii < 0 || a.n_radii > 65535 || (a.n_radii > 0 && (!a.thr_blocked || !a.integral))) return hipErrorInvalidValue;
    if (a.goal_occ && (a.n_radii < 1 || a.H < 1 || a.W < 1 || a.A < 1 || !a.cell_of || !a.thr_goal)) return hipErrorInvalidValue;
    const size_t cells = (size_t)a.nx * a.ny * a.nz, X = a.nx + 1, Y = a.ny + 1, Z = a.nz + 1;
    if ((cells + MAPT - 1) / MAPT > 0x7fffffffull) return hipErrorInvalidValue;
    hipError_t e = launch_variant(kernel_address(lsc_map_edt_kernel<2>), map_grid(cells), dim3(MAPT), 0, st, a);
    if (e == hipSuccess) e = launch_variant(kernel_address(lsc_map_edt_kernel<1>), map_grid(cells), dim3(MAPT), 0, st, a);
    if (e == hipSuccess) e = launch_variant(kernel_address(lsc_map_edt_kernel<0>), map_grid(cells), dim3(MAPT), 0, st, a);
    if (a.n_radii == 0) return e;
    if (e == hipSuccess) e = launch_variant(kernel_address(lsc_map_integral_kernel<2>), map_grid(X * Y, a.n_radii), dim3(MAPT), 0, st, a);
    if (e == hipSuccess) e = launch_variant(kernel_address(lsc_map_integral_kernel<1>), map_grid(X * Z, a.n_radii), dim3(MAPT), 0, st, a);
    if (e == hipSuccess) e = launch_variant(kernel_address(lsc_map_integral_kernel<0>), map_grid(Y * Z, a.n_radii), dim3(MAPT), 0, st, a);
    if (e == hipSuccess && a.goal_occ) e = launch_variant(kernel_address(lsc_map_goal_kernel), map_grid((size_t)a.H * a.W * a.A, a.n_radii), dim3(MAPT), 0, st, a);
    return e;
}

}  // namespace lsc
