"""The map's device statements (csrc/lsc_map.hpp) and the occupancy reader, without a GPU.

The kernels of csrc/lsc_map.hip call the LSC_HD functions of lsc_map.hpp one lane per cell or per line.  A host build of the same text --
a stand-alone program, walking the cells and lines in the kernels' order -- is run on random occupancies and compared, byte for byte,
with the numpy restatement of tests/map_reference.py (brute force over the truncation ball, cumsum, the goal grid's own geometry)."""
import os
import subprocess

import numpy as np
import pytest

import map_reference as MR
from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "lsc_planner_amd", "csrc")

HOST_CHECK = r"""
// The chain of lsc_map.hip on the host: edits, three passes, three scans per radius, the goal gather -- each through lsc_map.hpp's statement.
// argv: parameters (text), occupancy in (bytes), products out (edt floats | integral ints | goal occupancy bytes | occupancy bytes)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lsc_map.hpp"

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx, ny, nz, kmin[3], H, W, A, R;
    double res, maxdist, gmin[3], gres;
    lsc::MapBoxes boxes = {};
    if (std::fscanf(f, "%d %d %d %d %d %d %lf %lf %lf %lf %lf %lf %d %d %d %d %d", &nx, &ny, &nz, &kmin[0], &kmin[1], &kmin[2], &res, &maxdist, &gmin[0],
                    &gmin[1], &gmin[2], &gres, &H, &W, &A, &R, &boxes.n) != 17) return 2;
    std::vector<double> thr_blocked(R), thr_goal(R);
    for (int r = 0; r < R; r++) if (std::fscanf(f, "%lf %lf", &thr_blocked[r], &thr_goal[r]) != 2) return 2;
    for (int i = 0; i < boxes.n; i++) {
        int v;
        for (int k = 0; k < 6; k++) if (std::fscanf(f, "%d", &boxes.box[i][k]) != 1) return 2;
        if (std::fscanf(f, "%d", &v) != 1) return 2;
        boxes.value[i] = (unsigned char)v;
    }
    std::fclose(f);
    const size_t cells = (size_t)nx * ny * nz, plane = (size_t)ny * nz;
    std::vector<unsigned char> occ(cells);
    f = std::fopen(argv[2], "rb");
    if (!f || std::fread(occ.data(), 1, cells, f) != cells) return 2;
    std::fclose(f);

    const int md = lsc::map_truncation_cells(maxdist, res), trunc2 = md * md;
    if (md < 1 || md > lsc::MAP_MD_MAX) return 3;
    std::vector<float> table(trunc2 + 1);
    for (int d2 = 0; d2 <= trunc2; d2++) table[d2] = lsc::map_edt_table_entry(d2, res);
    const int dims[3] = {nx, ny, nz}, gdim[3] = {H, W, A};
    std::vector<int> cell_of;
    for (int a = 0; a < 3; a++)
        for (int i = 0; i < gdim[a]; i++) cell_of.push_back(lsc::map_goal_cell(gmin[a], i, gres, 1.0 / res, kmin[a], dims[a]));

    auto xyz = [&](size_t i, int &x, int &y, int &z) { z = (int)(i % nz); y = (int)(i / nz % ny); x = (int)(i / nz / ny); };
    int x, y, z;
    for (size_t i = 0; i < cells; i++) { xyz(i, x, y, z); occ[i] = lsc::map_edit_cell(occ[i], x, y, z, boxes); }
    std::vector<unsigned short> pa(cells), pb(cells);
    std::vector<float> edt(cells);
    for (size_t i = 0; i < cells; i++) { xyz(i, x, y, z); pa[i] = (unsigned short)lsc::map_edt_first(occ.data() + (i - z), 1, nz, z, md); }
    for (size_t i = 0; i < cells; i++) { xyz(i, x, y, z); pb[i] = (unsigned short)lsc::map_edt_next(pa.data() + (i - (size_t)y * nz), (size_t)nz, ny, y, md); }
    for (size_t i = 0; i < cells; i++) {
        xyz(i, x, y, z);
        edt[i] = lsc::map_edt_value(lsc::map_edt_next(pb.data() + (i - (size_t)x * plane), plane, nx, x, md), trunc2, table.data());
    }
    const int X = nx + 1, Y = ny + 1, Z = nz + 1;
    const size_t isz = (size_t)X * Y * Z, C = (size_t)H * W * A;
    std::vector<int> integral(isz * R, -77);                       // (every entry must be written)
    std::vector<unsigned char> gocc(C * R, 0xee);
    for (int r = 0; r < R; r++) {
        int *I = integral.data() + (size_t)r * isz;
        for (size_t l = 0; l < (size_t)X * Y; l++) lsc::map_integral_scan_z(edt.data(), I, nx, ny, nz, (int)(l / Y), (int)(l % Y), thr_blocked[r]);
        for (size_t l = 0; l < (size_t)X * Z; l++) lsc::map_integral_scan(I + (l / Z) * Y * Z + l % Z, (size_t)Z, ny);
        for (size_t l = 0; l < (size_t)Y * Z; l++) lsc::map_integral_scan(I + l, (size_t)Y * Z, nx);
        for (size_t g = 0; g < C; g++) {
            const int j = (int)(g % W), i = (int)(g / W % H), k = (int)(g / W / H);
            gocc[(size_t)r * C + g] = lsc::map_goal_occupied(edt.data(), ny, nz, cell_of[i], cell_of[H + j], cell_of[H + W + k], thr_goal[r]);
        }
    }
    f = std::fopen(argv[3], "wb");
    if (!f) return 2;
    std::fwrite(edt.data(), sizeof(float), cells, f);
    std::fwrite(integral.data(), sizeof(int), integral.size(), f);
    std::fwrite(gocc.data(), 1, gocc.size(), f);
    std::fwrite(occ.data(), 1, cells, f);
    std::fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """The stand-alone program (never loaded into Python), built with the address and undefined-behaviour sanitizers."""
    d = tmp_path_factory.mktemp("map_host")
    src, exe = d / "map_host_check.cpp", d / "map_host_check"
    src.write_text(HOST_CHECK)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe), d


WORLD = (np.array([-2.0, -2.0, 0.0], np.float32), np.array([2.0, 2.0, 2.0], np.float32))

# (shape, density, maxdist, radii, boxes): shapes with an axis shorter than the window, of exactly md and 2 md - 1 cells, a single cell
CASES = [
    ((1, 1, 1), 1.0, 1.0, [0.15], 0),
    ((1, 1, 1), 0.0, 1.0, [0.15], 0),
    ((3, 2, 1), 0.3, 1.0, [0.15], 1),
    ((5, 40, 3), 0.02, 1.0, [0.15, 0.25], 2),
    ((11, 12, 21), 0.01, 1.0, [0.15], 0),
    ((30, 17, 9), 0.0, 0.35, [0.15], 0),
    ((30, 17, 9), 1.0, 0.35, [0.15], 0),
    ((41, 41, 21), 0.01, 1.0, [0.15, 0.3], 5),
    ((41, 41, 21), 0.3, 0.35, [0.15], 64),
    ((23, 19, 12), 0.002, 1.0, [0.1, 0.15, 0.2], 3),
]


def _field_key_min(shape):
    """A field of `shape` cells around the middle of WORLD."""
    res = 0.1
    return np.array([int(np.floor((WORLD[0][a] + WORLD[1][a]) / 2 / res)) + 32768 - shape[a] // 2 for a in range(3)], np.int32)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_device_statements_equal_the_numpy_restatement(host_check, case):
    exe, d = host_check
    shape, density, maxdist, radii, n_boxes = CASES[case]
    rng = np.random.default_rng(500 + case)
    res, gres, margin = 0.1, 0.3, 0.2
    occ = (rng.random(shape) < density).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)      # any non-zero byte is occupied
    kmin = _field_key_min(shape)
    boxes, values = [], []
    for _ in range(n_boxes):
        lo = [int(rng.integers(0, n)) for n in shape]
        hi = [int(rng.integers(l + 1, min(l + 4, n) + 1)) for l, n in zip(lo, shape)]
        boxes.append(lo + hi); values.append(int(rng.integers(0, 2)))
    gmin, (H, W, A) = MR.grid_geometry(WORLD[0], WORLD[1], gres)
    thr = [(r + 0.5 * res - 1e-5, r + float(np.float32(margin))) for r in radii]
    par, fin, fout = d / f"p{case}.txt", d / f"occ{case}.bin", d / f"out{case}.bin"
    par.write_text(" ".join([*map(str, shape), *map(str, kmin), repr(res), repr(maxdist), *(repr(float(g)) for g in gmin), repr(gres), str(H), str(W), str(A),
                             str(len(radii)), str(n_boxes)] + [f"{a!r} {b!r}" for a, b in thr] +
                            [" ".join(map(str, b)) + f" {v}" for b, v in zip(boxes, values)]))
    fin.write_bytes(occ.tobytes())
    r = subprocess.run([exe, str(par), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = fout.read_bytes()
    cells, isz, C, R = occ.size, int(np.prod(np.array(shape) + 1)), H * W * A, len(radii)
    assert len(raw) == 4 * cells + 4 * isz * R + C * R + cells
    got_edt = np.frombuffer(raw, np.float32, cells).reshape(shape)
    got_int = np.frombuffer(raw, np.int32, isz * R, 4 * cells).reshape((R,) + tuple(np.array(shape) + 1))
    got_goal = np.frombuffer(raw, np.uint8, C * R, 4 * cells + 4 * isz * R).reshape(R, A, H, W)
    got_occ = np.frombuffer(raw, np.uint8, cells, 4 * cells + 4 * isz * R + C * R).reshape(shape)

    want_occ = MR.apply_boxes(occ, boxes, values) if n_boxes else occ
    assert np.array_equal(got_occ != 0, want_occ != 0)
    want_edt = MR.edt(want_occ, res, maxdist)
    assert got_edt.tobytes() == want_edt.tobytes(), int((got_edt != want_edt).sum())
    assert np.array_equal(got_int, MR.integral(want_edt, radii, res))
    assert np.array_equal(got_goal, MR.goal_occupancy(want_edt, kmin, res, radii, WORLD[0], WORLD[1], gres, margin))
    if density > 0 and 0 < want_occ.mean() < 1 and min(shape) > 1:
        assert len(np.unique(want_edt)) > 2                       # the case is not vacuous


@pytest.fixture(scope="module")
def ref_world(tmp_path_factory):
    root = tmp_path_factory.mktemp("world")
    z = np.load(os.path.join(GOLDEN, "reference_maps.npz"))
    for name in z.files:
        path = root / name
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(z[name].tobytes())
    return str(root)


@pytest.mark.parametrize("name,world", [("simple_forest.bt", (-5, -5, 0, 5, 5, 2.5)), ("forest/forest1.bt", (-6, -6, 0, 6, 6, 2.5)),
                                        ("office.bt", (-10, -10, 0, 10, 10, 2.5))])
def test_occupancy_reader_marks_the_cells_where_the_distance_is_zero(ref_world, name, world):
    import lsc_planner_amd as L
    path = os.path.join(ref_world, name)
    occ, kmin, res = L.occupancy_from_bt(path, world[:3], world[3:])
    dist, kmin_d, res_d = L.edt_from_bt(path, world[:3], world[3:])
    assert occ.dtype == np.uint8 and occ.shape == dist.shape and np.array_equal(kmin, kmin_d) and res == res_d
    assert occ.any() and set(np.unique(occ)) <= {0, 1}
    assert np.array_equal(occ != 0, dist == 0)


def test_reference_edt_is_the_oracles_on_simple_forest(ref_world, oracle):
    import lsc_planner_amd as L
    world = (-5, -5, 0, 5, 5, 2.5)
    path = os.path.join(ref_world, "simple_forest.bt")
    res, leaves = oracle.bt_read(path)
    dm = oracle.DistMap(leaves, res, world[:3], world[3:])
    occ = np.zeros(dm.dist.shape, np.uint8)                      # the leaves on the field's grid, by hand
    for x, y, z, size in leaves:
        lo = np.maximum(np.array([x, y, z]) - dm.key_min, 0)
        hi = np.minimum(np.array([x, y, z]) + size - dm.key_min, occ.shape)
        if (lo < hi).all():
            occ[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    product_occ, kmin, _ = L.occupancy_from_bt(path, world[:3], world[3:])
    assert np.array_equal(kmin, dm.key_min) and np.array_equal(product_occ, occ)
    mine = MR.edt(occ, res, 1.0)
    assert mine.shape == dm.dist.shape and mine.tobytes() == dm.dist.tobytes()
    # ... and a shorter truncation, which the windows depend on
    assert MR.edt(occ, res, 0.35).tobytes() == oracle.DistMap(leaves, res, world[:3], world[3:], maxdist=0.35).dist.tobytes()
