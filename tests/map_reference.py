"""The four products of a map, restated in numpy from an occupancy array [nx][ny][nz] (non-zero = occupied): what lsc_edt_from_bt,
build_integrals and build_goal_grid (csrc/lsc_octomap.cpp, csrc/lsc_abi.cpp) compute on the host and csrc/lsc_map.hip on the device.

  edt             brute force: every cell against every offset inside the truncation ball -- no separable passes, no windows --, the float
                  by the formula of tests/test_map_assumptions.py:99
  integral        the blocked predicate and three cumsums
  goal_occupancy  the grid geometry of GridBasedPlanner::updateGridInfo, the float32 grid point, octomap's key formula, the predicate

Everything is an integer or a comparison of a float32 with a float64, so the comparisons against this module are exact."""
import math

import numpy as np


def truncation_cells(maxdist, res):
    return int(maxdist / res + 1)


def squared_distance(occ, md):
    """Squared lattice distance to the nearest occupied cell, truncated at md^2: int32 [nx][ny][nz]."""
    occ = np.asarray(occ) != 0
    nx, ny, nz = occ.shape
    trunc2 = md * md
    out = np.full(occ.shape, trunc2, np.int32)
    if not occ.any():
        return out
    w = md - 1                                               # an offset of md cells on any axis is at least md away
    pad = np.zeros((nx + 2 * w, ny + 2 * w, nz + 2 * w), bool)
    pad[w:w + nx, w:w + ny, w:w + nz] = occ
    for dx in range(-w, w + 1):
        for dy in range(-w, w + 1):
            dxy = dx * dx + dy * dy
            if dxy >= trunc2:
                continue
            plane = pad[w + dx:w + dx + nx, w + dy:w + dy + ny]
            if not plane.any():
                continue
            for dz in range(-w, w + 1):
                d2 = dxy + dz * dz
                if d2 >= trunc2:
                    continue
                np.minimum(out, np.where(plane[:, :, w + dz:w + dz + nz], np.int32(d2), np.int32(trunc2)), out=out)
    return out


def edt(occ, res, maxdist=1.0):
    """float32 [nx][ny][nz] metres: float32(float64(float32(sqrt(min(d2, md^2)))) * res)."""
    d2 = squared_distance(occ, truncation_cells(maxdist, res))
    return (np.sqrt(d2.astype(np.float64)).astype(np.float32).astype(np.float64) * res).astype(np.float32)


def distinct_radii(radius):
    """Distinct radii in order of first appearance, and every agent's image."""
    radii, img = [], []
    for r in np.asarray(radius, np.float64):
        if r not in radii:
            radii.append(float(r))
        img.append(radii.index(float(r)))
    return radii, np.asarray(img, np.int32)


def integral(dist, radii, world_res):
    """int32 [n_radii][nx+1][ny+1][nz+1]: I[x][y][z] = blocked cells in [0, x) x [0, y) x [0, z)."""
    nx, ny, nz = dist.shape
    out = np.zeros((len(radii), nx + 1, ny + 1, nz + 1), np.int32)
    for i, r in enumerate(radii):
        blocked = dist.astype(np.float64) < r + 0.5 * world_res - 1e-5
        out[i, 1:, 1:, 1:] = blocked.astype(np.int32).cumsum(0).cumsum(1).cumsum(2)
    return out


def grid_geometry(world_min, world_max, grid_res, planar_z=None):
    """(grid_min float64[3], dims [H, W, A]) of the goal planner's grid."""
    gmin, dims = np.zeros(3), [0, 0, 0]
    for a in range(3):
        lo, hi = float(np.float32(world_min[a])), float(np.float32(world_max[a]))
        gmin[a] = -math.floor((-lo + 1e-9) / grid_res) * grid_res
        gmax = math.floor((hi + 1e-9) / grid_res) * grid_res
        if a == 2 and planar_z is not None:
            gmin[a], dims[a] = planar_z, 1
        else:
            dims[a] = int(math.floor((gmax - gmin[a]) / grid_res + 0.5)) + 1
    return gmin, dims


def goal_occupancy(dist, key_min, res, radii, world_min, world_max, grid_res=0.3, grid_margin=0.2, planar_z=None):
    """uint8 [n_radii][A][H][W] (flat index H W k + W i + j): occupied = float64(edt_at(p)) < r + float64(float32(grid_margin)), a
    point outside the field reads -1."""
    gmin, (H, W, A) = grid_geometry(world_min, world_max, grid_res, planar_z)
    rf = 1.0 / res
    cells = []
    for a, n in enumerate((H, W, A)):
        p = (gmin[a] + np.arange(n) * grid_res).astype(np.float32)
        c = np.floor(rf * p.astype(np.float64)).astype(np.int64) + 32768 - int(key_min[a])
        cells.append(np.where((c < 0) | (c >= dist.shape[a]), -1, c))
    ci, cj, ck = np.meshgrid(cells[0], cells[1], cells[2], indexing="ij")              # [H][W][A]
    outside = (ci < 0) | (cj < 0) | (ck < 0)
    e = np.where(outside, np.float32(-1.0), dist[np.maximum(ci, 0), np.maximum(cj, 0), np.maximum(ck, 0)]).astype(np.float64)
    margin = float(np.float32(grid_margin))
    out = np.zeros((len(radii), A, H, W), np.uint8)
    for i, r in enumerate(radii):
        out[i] = (e < r + margin).transpose(2, 0, 1)
    return out


def apply_boxes(occ, boxes, values):
    """The occupancy behind a list of edits, in order: box = x0, y0, z0, x1, y1, z1 (lo inclusive, hi exclusive)."""
    occ = (np.asarray(occ) != 0).astype(np.uint8)
    for b, v in zip(np.asarray(boxes).reshape(-1, 6), values):
        occ[b[0]:b[3], b[1]:b[4], b[2]:b[5]] = v
    return occ
