"""The flight record's host side (include/lsc_planner_amd.h: lsc_flight_weights, lsc_flight_row_bytes; csrc/lsc_flight.hpp), without a GPU.

The record kernel repeats multiply-adds only: the Bernstein weights and the segment of every record time are formed on the host, in the
reference's own expression (include/polynomial.hpp:22-24, 63-74).  Every comparison here is bitwise."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "lsc_planner_amd", "csrc")


def _weights_restated(dt, t, M):
    """nChoosek * pow(t, i) * pow(1 - t, n - i) at the local parameter of the time's segment (getStateFromControlPoints)."""
    m = int(t / dt)
    if m == M and t < M * dt + 1e-9:
        m = M - 1
    tl = t / dt - m
    return m, [[math.comb(n, i) * tl ** i * (1 - tl) ** (n - i) for i in range(n + 1)] for n in (5, 4, 3)]


@pytest.mark.parametrize("dt,segments", [(0.2, 5), (0.5, 4), (0.5, 5)])
def test_weights_are_the_reference_expression(dt, segments):
    import lsc_planner_amd as L
    horizon = segments * dt
    times = [t for t in (0.0, 0.1, 0.17, 0.45) if t <= horizon] + [horizon]
    w5, w4, w3, seg = L.flight_weights(dt, times, segments)
    for ti, t in enumerate(times):
        m, (r5, r4, r3) = _weights_restated(dt, t, segments)
        assert seg[ti] == m
        assert w5[ti].tolist() == r5 and w4[ti].tolist() == r4 and w3[ti].tolist() == r3, (t, w5[ti], r5)
    # exactly the horizon: the last segment at local parameter 1
    assert seg[-1] == segments - 1
    assert w5[-1].tolist() == [0, 0, 0, 0, 0, 1] and w4[-1].tolist() == [0, 0, 0, 0, 1] and w3[-1].tolist() == [0, 0, 0, 1]
    # a time in a later segment is not a time of the first one
    assert seg[times.index(0.45)] == int(0.45 / dt)


@pytest.mark.parametrize("dt,segments", [(0.2, 5), (0.5, 4)])
def test_weights_refuse_times_outside_the_horizon(dt, segments):
    import lsc_planner_amd as L
    from lsc_planner_amd import _lib
    lib = _lib.load_library(segments)
    horizon = segments * dt
    dp = ctypes.POINTER(ctypes.c_double)

    def rc(times):
        t = np.ascontiguousarray(times, np.float64)
        w5 = np.zeros((max(len(t), 1), 6))
        return lib.lsc_flight_weights(dt, t.ctypes.data_as(dp), len(t), w5.ctypes.data_as(dp), None, None, None)
    assert rc([0.0, horizon]) == 0
    assert rc([-1e-3]) == -1 and rc([0.0, -0.1]) == -1                   # LSC_EINVAL
    assert rc([horizon + dt]) == -1 and rc([horizon + 1e-6]) == -1
    assert rc([]) == -1 and rc([0.0] * 65) == -1 and rc([0.0] * 64) == 0
    with pytest.raises(L.LscError):
        L.flight_weights(dt, [horizon + dt], segments)


def test_row_bytes_is_the_layout_formula():
    from lsc_planner_amd import _lib
    lib = _lib.load_library()
    for N in (1, 2, 7, 64, 65, 257, 8192):
        for T in (1, 2, 3, 64):
            for what in range(8):
                b = 64
                if what & _lib.FLIGHT_SAFETY:
                    b += (8 + 4) * T * N
                if what & _lib.FLIGHT_SAMPLES:
                    b += 4 * 9 * T * N
                if what & _lib.FLIGHT_AGENTS:
                    b += (8 + 4 + 12) * N
                assert lib.lsc_flight_row_bytes(N, T, what) == (b + 63) // 64 * 64, (N, T, what)
    assert lib.lsc_flight_row_bytes(4, 1, 0) == 64
    assert lib.lsc_flight_row_bytes(0, 1, 7) == 0 and lib.lsc_flight_row_bytes(4, 0, 7) == 0 and lib.lsc_flight_row_bytes(4, 65, 7) == 0
    assert lib.lsc_flight_row_bytes(4, 1, 8) == 0
    assert ctypes.sizeof(_lib.LscFlightTick) == 64 and _lib.LscFlightTick.min_ratio.offset == 40
    assert ctypes.sizeof(_lib.LscFlightConfig) == 8 + 64 * 8 + 8


HOST_CHECK = r"""
// The record statements of lsc_flight.hpp against the plain loops they restate: getStateFromControlPoints of the host layer
// (csrc/host/lsc_host.hpp, include/polynomial.hpp:63-97) and savePlanningResult's pair loop (src/multi_sync_simulator.cpp:446-503,
// distBetweenAgents include/util.hpp:225-229), over a seeded table.  Exit status 0: every value is the same bits.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "host/lsc_host.hpp"
#include "lsc_flight.hpp"

using namespace DynamicPlanning;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform(double lo, double hi)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return lo + (hi - lo) * (double)(rng_state >> 11) / 9007199254740992.0;
}
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

int main()
{
    const int N = 5, M = lsc::M, NC = lsc::NC;
    const double dt = M == 5 ? 0.2 : 0.5;
    std::vector<double> times = {0.0, 0.1, 0.17, 0.45, M * dt};
    const int T = (int)times.size();
    std::vector<float> table((size_t)N * lsc::NV);
    std::vector<double> radius(N), downwash(N);
    for (int q = 0; q < N; q++) {
        radius[q] = uniform(0.1, 0.2);
        downwash[q] = uniform(1.0, 2.5);
        for (int k = 0; k < 3; k++) {
            float x = (float)uniform(-3, 3);
            for (int j = 0; j < lsc::SEGV; j++) { x += (float)uniform(-0.05, 0.08); table[(size_t)q * lsc::NV + k * lsc::SEGV + j] = x; }
        }
    }
    // agent 4 flies agent 3's plan with agent 3's size: every other agent has two partners at exactly the same ratio (the first stays)
    for (int j = 0; j < lsc::NV; j++) table[(size_t)4 * lsc::NV + j] = table[(size_t)3 * lsc::NV + j];
    radius[4] = radius[3]; downwash[4] = downwash[3];

    std::vector<double> w5((size_t)T * 6), w4((size_t)T * 5), w3((size_t)T * 4);
    std::vector<int> seg(T);
    for (int ti = 0; ti < T; ti++) {
        seg[ti] = lsc::flight_segment(times[ti], dt);
        if (seg[ti] < 0) { std::puts("a time inside the horizon was refused"); return 2; }
        const double tl = lsc::flight_local_time(times[ti], dt, seg[ti]);
        lsc::flight_bernstein(5, tl, w5.data() + ti * 6);
        lsc::flight_bernstein(4, tl, w4.data() + ti * 5);
        lsc::flight_bernstein(3, tl, w3.data() + ti * 4);
    }
    if (lsc::flight_segment(-0.25, dt) >= 0 || lsc::flight_segment(M * dt + dt, dt) >= 0) { std::puts("a time outside the horizon was accepted"); return 2; }
    const float dt_inv = (float)std::pow(dt, -1);

    std::vector<traj_t> trajs(N, traj_t(M, std::vector<point3d>(NC)));
    for (int q = 0; q < N; q++)
        for (int m = 0; m < M; m++)
            for (int i = 0; i < NC; i++)
                for (int k = 0; k < 3; k++) trajs[q][m][i](k) = table[(size_t)q * lsc::NV + k * lsc::SEGV + m * NC + i];

    int bad = 0, ties = 0;
    for (int ti = 0; ti < T; ti++) {
        std::vector<point3d> pos(N);
        for (int q = 0; q < N; q++) {
            const State s = getStateFromControlPoints(trajs[q], times[ti], M, 5, dt);
            pos[q] = s.position;
            float p[3];
            lsc::flight_position(table.data() + (size_t)q * lsc::NV, seg[ti], w5.data() + ti * 6, p);
            for (int k = 0; k < 3; k++) {
                const lsc::FlightAxisSample a = lsc::flight_axis_sample(table.data() + (size_t)q * lsc::NV + k * lsc::SEGV + seg[ti] * NC, w5.data() + ti * 6,
                                                                       w4.data() + ti * 5, w3.data() + ti * 4, dt_inv);
                if (!same(a.p, s.position(k)) || !same(a.v, s.velocity(k)) || !same(a.a, s.acceleration(k)) || !same(p[k], s.position(k))) {
                    std::printf("sample differs: time %g agent %d axis %d\n", times[ti], q, k);
                    bad++;
                }
            }
        }
        for (int qi = 0; qi < N; qi++) {
            // the reference's loop
            double ref = SP_INFINITY; int ref_q = -1;
            for (int qj = 0; qj < N; qj++) {
                if (qi == qj) continue;
                const double dw = (downwash[qi] * radius[qi] + downwash[qj] * radius[qj]) / (radius[qi] + radius[qj]);
                point3d delta = pos[qi] - pos[qj];
                delta(2) = delta.z() / dw;
                const double r = delta.norm() / (radius[qi] + radius[qj]);
                if (r < ref) { ref = r; ref_q = qj; }
            }
            // the record's statement, partners in increasing index, strict minimum
            double best = lsc::FLIGHT_NO_PARTNER; int best_q = -1;
            for (int qj = 0; qj < N; qj++) {
                if (qi == qj) continue;
                const double r = lsc::flight_pair_ratio(pos[qi].v, pos[qj].v, radius[qi], downwash[qi], radius[qj], downwash[qj]);
                if (r < best) { best = r; best_q = qj; }
            }
            if (!same(best, ref) || best_q != ref_q) { std::printf("pair differs: time %g agent %d: %.17g/%d vs %.17g/%d\n", times[ti], qi, best, best_q, ref, ref_q); bad++; }
        }
        {
            const double r3 = lsc::flight_pair_ratio(pos[0].v, pos[3].v, radius[0], downwash[0], radius[3], downwash[3]);
            const double r4 = lsc::flight_pair_ratio(pos[0].v, pos[4].v, radius[0], downwash[0], radius[4], downwash[4]);
            ties += same(r3, r4);
        }
    }
    // end point, moved, goal tests
    for (int q = 0; q < N; q++) {
        float e[3], e2[3];
        lsc::flight_end_point(table.data() + (size_t)q * lsc::NV, e);
        const point3d ref = trajs[q][M - 1][NC - 1];
        for (int k = 0; k < 3; k++) if (!same(e[k], ref(k))) { std::printf("end point differs: agent %d\n", q); bad++; }
        for (int k = 0; k < 3; k++) e2[k] = e[k];
        if (lsc::flight_moved(e, e2, 2) || !lsc::flight_moved(e, e2, 1)) { std::puts("moved: equal end points"); bad++; }
        e2[0] = e[0] + 1e-3f;
        const point3d a(e[0], e[1], e[2]), b(e2[0], e2[1], e2[2]);
        if (lsc::flight_moved(e, e2, 2) != ((a - b).norm() >= SP_EPSILON_FLOAT)) { std::puts("moved: shifted end point"); bad++; }
    }
    std::printf("checked %d agents x %d times, %d tied pairs, %d differences\n", N, T, ties, bad);
    if (ties != T) { std::puts("the table has no tied partners"); return 3; }
    return bad ? 1 : 0;
}
"""


@pytest.mark.parametrize("segments", [5, 4])
def test_record_statements_equal_the_plain_loops(tmp_path, segments):
    """A stand-alone program of its own (never loaded into Python), built with the address and undefined-behaviour sanitizers."""
    src = tmp_path / "flight_host_check.cpp"
    src.write_text(HOST_CHECK)
    exe = tmp_path / "flight_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           f"-DLSC_SEGMENTS={segments}", "-I", CSRC, str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 differences" in r.stdout, r.stdout
