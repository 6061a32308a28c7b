"""The obstacle stage's statements (csrc/lsc_obstacle_motion.hpp: obstacle_entry_build, obstacle_at, obstacle_walk_ok) without a GPU: compiled
for the host by the test itself, in a stand-alone program, and held to ObstacleSet.at (lsc_planner_amd/obstacles.py) and to the simulator's
ObstacleMotion::at (csrc/host/lsc_host.hpp) compiled into the same program.

straight and multisim_patrol take + - x / sqrt and comparisons only: the float32 states are the same bits on all three sides.  spin goes
through the platform's double sin / cos: within one float32 step (np.spacing) of ObstacleSet's float32 value, the bound
tests/test_obstacle_motion.py holds the C++ host and ObstacleSet to.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from lsc_planner_amd.obstacles import ObstacleSet
from obstacle_reference import SIM_OBSTACLES
from test_obstacle_motion import PATROL, SPIN, STRAIGHT

CSRC = os.path.join(ROOT, "lsc_planner_amd", "csrc")

MODEL = np.dtype([("kind", np.int32), ("n_points", np.int32), ("speed", np.float64), ("points", np.float64, (8, 3))])       # lsc_obstacle_model
OUT = np.dtype([("code", np.int32), ("walk_ok", np.int32), ("table", np.float32, 6), ("host", np.float32, 6)])

# a patrol with a repeated waypoint: a leg of no length, stepped over by the walk
PATROL_REPEAT = dict(PATROL, waypoints=[{"waypoint": [0, 0, 1]}, {"waypoint": [2, 0, 1]}, {"waypoint": [2, 0, 1]}, {"waypoint": [2, 1.5, 1.2]}])
OBSTACLES = [STRAIGHT, SPIN, PATROL, PATROL_REPEAT] + SIM_OBSTACLES
EXACT = [i for i, o in enumerate(OBSTACLES) if o["type"] != "spin"]
SPINS = [i for i, o in enumerate(OBSTACLES) if o["type"] == "spin"]

HOST_PROGRAM = r"""
// every model of the first file at every time of the second: the table's state (obstacle_entry_build + obstacle_at, rounded to float32 as the
// stage rounds it) and the simulator's (ObstacleMotion::at, built as Mission::initialize builds it), to the third file (MODEL / OUT of the test)
#include <cstdio>
#include <cstring>
#include <vector>
#include "lsc_obstacle_motion.hpp"
#include "host/lsc_host.hpp"
struct Out { int code, walk_ok; float table[6], host[6]; };
int main(int argc, char **argv)
{
    static_assert(sizeof(lsc_obstacle_model) == 208 && sizeof(Out) == 56, "the test's dtypes");
    if (argc != 4) return 2;
    FILE *fm = std::fopen(argv[1], "rb"), *ft = std::fopen(argv[2], "rb"), *out = std::fopen(argv[3], "wb");
    if (!fm || !ft || !out) return 2;
    std::vector<double> times;
    double t;
    while (std::fread(&t, sizeof(t), 1, ft) == 1) times.push_back(t);
    lsc_obstacle_model m;
    while (std::fread(&m, sizeof(m), 1, fm) == 1) {
        lsc::ObstacleEntry e;
        const int code = lsc::obstacle_entry_build(m.kind, m.n_points, m.speed, m.points, e);
        DynamicPlanning::ObstacleMotion h;
        if (!code) {
            h.kind = m.kind; h.speed = m.speed;
            for (int i = 0; i < m.n_points; i++) h.pts.push_back({m.points[i][0], m.points[i][1], m.points[i][2]});
            if (m.kind == 1) {                             // Mission::initialize: the axis normalised, the start relative to the axis position
                std::array<double, 3> &c = h.pts[0], &n = h.pts[1], &st = h.pts[2];
                const double nn = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                for (int k = 0; k < 3; k++) { n[k] /= nn; st[k] -= c[k]; }
            }
        }
        for (double tt : times) {
            Out o = {};
            o.code = code;
            o.walk_ok = !code && lsc::obstacle_walk_ok(e, tt);
            if (o.walk_ok) {
                double p[3], v[3];
                lsc::obstacle_at(e, tt, p, v);
                for (int k = 0; k < 3; k++) { o.table[k] = (float)p[k]; o.table[3 + k] = (float)v[k]; }
                h.at(tt, p, v);
                for (int k = 0; k < 3; k++) { o.host[k] = (float)p[k]; o.host[3 + k] = (float)v[k]; }
            }
            if (std::fwrite(&o, sizeof(o), 1, out) != 1) return 3;
        }
    }
    std::fclose(fm); std::fclose(ft); std::fclose(out);
    return 0;
}
"""


def models_of(obstacles):
    """lsc_obstacle_model records of mission obstacles (dicts), without ObstacleSet's checks."""
    m = np.zeros(len(obstacles), MODEL)
    for r, o in zip(m, obstacles):
        if o["type"] == "straight":
            kind, pts = 0, [o["start"], o["goal"]]
        elif o["type"] == "spin":
            kind, pts = 1, [o["axis_position"], o["axis_ori"], o["start"]]
        else:
            kind, pts = 2, [w["waypoint"] for w in o["waypoints"]]
        r["kind"], r["n_points"], r["speed"] = kind, len(pts), o["speed"]
        r["points"][:len(pts)] = pts
    return m


def _build(d, name, *flags):
    src, exe = d / "obstacle_motion_host.cpp", d / name
    src.write_text(HOST_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", *flags, "-I", CSRC, str(src), "-o", str(exe)])
    return exe


def _run(d, exe, models, times):
    fm, ft, fout = d / "models.bin", d / "times.bin", d / "out.bin"
    np.ascontiguousarray(models).tofile(fm)
    np.ascontiguousarray(times, np.float64).tofile(ft)
    subprocess.check_call([str(exe), str(fm), str(ft), str(fout)], timeout=60)
    out = np.fromfile(fout, OUT)
    assert len(out) == len(models) * len(times)
    return out.reshape(len(models), len(times))


@pytest.fixture(scope="session")
def host_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("obstacle_motion_rules")


@pytest.fixture(scope="session")
def host_motion(host_dir):
    """-> run(models, times) -> OUT [models][times] (no contraction: the reference's build has no fused multiply-add)"""
    exe = _build(host_dir, "obstacle_motion_host")
    return lambda models, times: _run(host_dir, exe, models, times)


def _times():
    s = ObstacleSet(OBSTACLES)
    t = [0.2 * k for k in range(301)]                                          # 0, 0.2 k for k to 300
    for i in EXACT:
        mo = s.motions[i]
        if hasattr(mo, "flight_time"):                                         # a straight's arrival, and one double step either side of it
            t += [mo.flight_time, np.nextafter(mo.flight_time, 0.0), np.nextafter(mo.flight_time, np.inf)]
        else:                                                                  # the 1st, 2nd and 40th period of a patrol
            t += [(n + f) * mo.period for n in (0, 1, 39) for f in (0.1, 0.45, 0.8)]
    return s, np.array(t, np.float64)


def test_states_equal_obstacleset_and_the_simulators_host(host_motion):
    s, times = _times()
    out = host_motion(models_of(OBSTACLES), times)
    assert not out["code"].any() and out["walk_ok"].all()
    ref = np.zeros((len(OBSTACLES), len(times), 6), np.float32)
    for j, t in enumerate(times):
        pos, vel = s.at(t)
        ref[:, j, :3], ref[:, j, 3:] = pos, vel
    # straight and patrol: the same bits as the simulator's C++ and as ObstacleSet
    for i in EXACT:
        assert np.array_equal(out["table"][i].view(np.int32), out["host"][i].view(np.int32)), OBSTACLES[i]["type"]
        differs = np.nonzero((out["table"][i].view(np.int32) != ref[i].view(np.int32)).any(axis=1))[0]
        assert len(differs) == 0, (OBSTACLES[i]["type"], times[differs][:5], out["table"][i][differs][:2], ref[i][differs][:2])
    # spin: one float32 step of ObstacleSet's float32 value
    for i in SPINS:
        for side in ("table", "host"):
            assert (np.abs(out[side][i].astype(np.float64) - ref[i].astype(np.float64)) <= np.spacing(np.abs(ref[i]))).all(), (i, side)
    # the walk took every leg of the patrols, the repeated waypoint's neighbours included, and the straight arrived
    assert (out["table"][EXACT[0], -3:, 3:] == 0).sum() >= 3 and len(np.unique(out["table"][3][:, 3:], axis=0)) == 3


def test_the_straights_arrival_is_the_hosts_comparison(host_motion):
    """t < flight_time strictly: one double step before the arrival the obstacle still flies, at it and after it it rests at the goal."""
    s = ObstacleSet([STRAIGHT])
    T = s.motions[0].flight_time
    out = host_motion(models_of([STRAIGHT]), [np.nextafter(T, 0.0), T, np.nextafter(T, np.inf)])[0]
    assert out["table"][0, 3:].any() and not out["table"][1:, 3:].any()
    assert np.array_equal(out["table"][1:, :3], np.tile(np.array(STRAIGHT["goal"], np.float32), (2, 1)))


def test_degenerate_models_are_refused_by_the_tables_own_check(host_motion):
    """The four inputs of test_degenerate_obstacles_are_refused, a point that is not finite, an unknown kind, nine waypoints."""
    bad = models_of([dict(PATROL, waypoints=[{"waypoint": [1, 1, 1]}]), dict(PATROL, waypoints=[{"waypoint": [1, 1, 1]}, {"waypoint": [1, 1, 1]}]),
                     dict(SPIN, start=[0.5, -0.5, 1.8]), dict(STRAIGHT, speed=0.0), dict(STRAIGHT, goal=[np.inf, 0, 0]), dict(STRAIGHT, speed=np.nan),
                     STRAIGHT, PATROL])
    bad["kind"][6] = 3
    bad["n_points"][7] = 9
    out = host_motion(bad, [0.0])
    # OBSTACLE_BAD_POINTS 2, _NO_DISTANCE 6, _ON_AXIS 5, _BAD_SPEED 4, _NOT_FINITE 3, _BAD_KIND 1
    assert list(out["code"][:, 0]) == [2, 6, 5, 4, 3, 3, 1, 2], out["code"][:, 0]


def test_the_walks_bound(host_motion):
    """A patrol tick is refused when time / shortest positive leg time exceeds 65 536; straights and spins have no walk."""
    s = ObstacleSet([PATROL_REPEAT])
    shortest = min(l.flight_time for l in s.motions[0].legs if l.flight_time > 0)
    out = host_motion(models_of([PATROL_REPEAT, STRAIGHT, SPIN]), [65536.0 * shortest, np.nextafter(65536.0 * shortest * (1 + 1e-15), np.inf), 1e12])
    assert list(out["walk_ok"][0]) == [1, 0, 0] and out["walk_ok"][1:].all()


def test_host_program_under_the_sanitizers(host_dir):
    """The same stand-alone program with -fsanitize=address,undefined (host code only): every model, every time, no report."""
    exe = _build(host_dir, "obstacle_motion_host_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    _, times = _times()
    out = _run(host_dir, exe, models_of(OBSTACLES), times)
    assert not out["code"].any()
