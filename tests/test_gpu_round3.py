"""-m gpu: round-3 additions.
  * lsc_dump_qp: the QP failure export of TrajOptimizer::solve (log/QPmodel.lp, src/traj_optimizer.cpp:99-153) -- the product's
    dump of the very scene the reference dumped, read back and compared with the reference's file number by number."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from harness import fly, start_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


def test_qp_dump_of_the_reference_scene_equals_the_reference_dump(L, tmp_path):
    """The reference's log/QPmodel.lp is the model CPLEX failed on (agent 3 of multi_random_10agents_1 at tick 1, z = 0.7).  The
    same scene through the C ABI: the agent's plan fails (status 1, like the reference), lsc_dump_qp writes its QP, and that file
    holds the reference file's numbers: 546 rows in the same order with the same names, senses, coefficients and right-hand
    sides, the same objective (quadratic, linear, constant) and the same bounds."""
    from lp_parse import parse_lp
    lp = json.load(open(os.path.join(GOLDEN, "qpmodel_lp.json")))
    sc = lp["scene"]
    starts = np.array(sc["starts_xy_z07"], np.float32)
    N, a = len(starts), sc["agent"]
    lin = np.zeros(90)
    for k, v in lp["lin"].items():
        lin[int(k)] = v
    goal = starts.copy()
    goal[:, :2] *= -0.5
    goal[a] = (-lin / 2)[[29, 59, 89]].astype(np.float32)          # the goal the reference's objective was built for
    ms = L.Mission(starts, goal, np.asarray(sc["world"][:3], np.float32), np.asarray(sc["world"][3:], np.float32),
                   np.full(N, sc["radius"]), np.full(N, sc["downwash"]), np.tile(sc["max_vel"], (N, 1)).astype(float),
                   np.tile(sc["max_acc"], (N, 1)).astype(float), np.full(N, sc["nominal_velocity"]))
    pl = L.SwarmPlanner(ms)
    with pytest.raises(L.LscError):
        pl.dump_qp(a, tmp_path / "early.lp")                         # no tick yet
    state, traj = start_inputs(ms, pl.SEGV)
    g = pl.plan(state, goal, traj)
    assert g["status"][a] == 1                                       # infeasible, as CPLEX found
    path = tmp_path / "QPmodel.lp"
    pl.dump_qp(a, path)
    pl.close()
    P = parse_lp(open(path, encoding="latin-1").read())
    assert len(P["rows"]) == len(lp["rows"]) == 546
    for R, Q in zip(lp["rows"], P["rows"]):
        assert R["name"] == Q["name"] and R["sense"] == Q["sense"], R["name"]
        a1 = np.zeros(90); a1[R["idx"]] = R["val"]
        a2 = np.zeros(90); a2[Q["idx"]] = Q["val"]
        assert np.abs(a1 - a2).max() <= 1e-12 * max(1.0, np.abs(a1).max()), R["name"]
        assert abs(R["rhs"] - Q["rhs"]) <= 1e-13 * max(1.0, abs(R["rhs"])), R["name"]
    def dense(quad):
        M = np.zeros((90, 90))
        for i, j, v in quad:
            M[i, j] += v
            if i != j:
                M[j, i] += v
        return M
    assert np.abs(dense(lp["quad"]) - dense(P["quad"])).max() <= 1e-9 * np.abs(dense(lp["quad"])).max()
    l2 = np.zeros(90)
    for k, v in P["lin"].items():
        l2[int(k)] = v
    assert np.abs(lin - l2).max() <= 1e-13
    assert abs(P["const"] - 5.58195613498786) <= 1e-12
    for i in range(90):
        lo, hi = lp["bounds"][str(i)]
        assert P["bounds"][i] == [lo, hi] or (lo is not None and abs(P["bounds"][i][0] - lo) < 1e-14 and abs(P["bounds"][i][1] - hi) < 1e-14), i


def test_kernel_statuses_and_costs_against_highs_verdicts(L):
    """The kernel against the INDEPENDENT solver, no oracle in between: 32 ticks of eight dense seeded soak missions
    (tests/golden/qp_pin_ticks.npz, made by tests/golden/make_qp_pin_ticks.py in the build container) hold, per agent, HiGHS's
    verdict on the agent's QP -- infeasible (151 of them, each with a phase-1 certificate: the minimal uniform violation of
    the rows is strictly positive) or optimal with a cost (369).  Same inputs through the C ABI: status 1 exactly where HiGHS
    certifies infeasibility, status 0 and HiGHS's cost elsewhere."""
    from tolerances import COST_ATOL, COST_RTOL
    Z = np.load(os.path.join(GOLDEN, "qp_pin_ticks.npz"))
    n_inf = n_opt = 0
    for t in range(int(Z["count"])):
        g = lambda k: Z[f"t{t}_{k}"]
        ms = L.Mission(g("start"), g("goal"), g("world_min"), g("world_max"), g("radius"), g("downwash"), g("max_vel"), g("max_acc"),
                       g("nominal_velocity"))
        pl = L.SwarmPlanner(ms)
        pl.planner_seq = int(g("tick")) - 1                       # plan() advances it: the tick's own planner_seq
        r = pl.plan(g("state"), g("goal"), g("traj"))
        pl.close()
        v, c = g("verdict"), g("cost")
        known = v >= 0
        assert np.array_equal(r["status"][known], (v[known] == 1).astype(np.int32)), (t, r["status"], v)
        opt = v == 0
        assert (np.abs(r["cost"][opt] - c[opt]) <= COST_RTOL * np.abs(c[opt]) + COST_ATOL).all(), (t, r["cost"][opt], c[opt])
        ub = v == 2                                                 # HiGHS stopped short: its cost is an upper bound (a few 1e-6 relative)
        assert (r["cost"][ub] <= c[ub] + COST_ATOL).all() and (r["cost"][ub] >= c[ub] * (1 - 1e-5) - COST_ATOL).all(), (t, r["cost"][ub], c[ub])
        n_inf += int((v == 1).sum()); n_opt += int(opt.sum() + ub.sum())
    assert n_inf >= 140 and n_opt >= 300, (n_inf, n_opt)


@pytest.mark.parametrize("seed,which,cfg,agent,highs_cost",
                         [(5023, 3, dict(planner_mode="bvc", n_constraint_segments=2), 2, 1.3618641918561454),
                          (4800332, 2, dict(planner_mode="bvc", slack_mode="dynamical_limit"), 2, 1860.235625116953),
                          (6800157, 2, dict(planner_mode="bvc", slack_mode="dynamical_limit"), 0, 4258.793418172383),      # (the oracle was 3.6e-6 off here until round 4)
                          (6800522, 2, dict(planner_mode="bvc", slack_mode="dynamical_limit"), 0, 16.849414817360),
                          (7301082, 2, dict(planner_mode="bvc", slack_mode="dynamical_limit"), 3, 3523.9260890555174)])      # (a face of optima: the value decides)
def test_fuzz_found_instance_through_the_kernel_against_highs(L, seed, which, cfg, agent, highs_cost):
    """tests/golden/fuzz_found_5023.npz: the alternate-mode QP (BVC, two constraint segments) on which the oracle used to give
    up and HiGHS found the optimum 1.3618641918561454; fuzz_found_4800332.npz (round 4): BVC with the dynamical-limit slack at
    |f| = 1860, where the oracle's plan is the one 6.7e-5 m from HiGHS's (tests/test_oracle_pins.py re-derives both optima when
    HiGHS is importable).  The current kernel on the recorded inputs, against those numbers directly."""
    Z = np.load(os.path.join(GOLDEN, "fuzz_found_%d.npz" % seed))
    assert int(Z["which"]) == which
    ms = L.Mission(Z["state"][:, :3].copy(), Z["goal"], Z["wmin"], Z["wmax"], Z["radius"], Z["dw"], Z["vmax"], Z["amax"], Z["vnom"])
    pl = L.SwarmPlanner(ms, L.PlannerConfig(**cfg))
    pl.planner_seq = int(Z["tick"]) - 1
    r = pl.plan(Z["state"], Z["goal"], Z["traj"])
    pl.close()
    assert (r["status"] == 0).all() and np.array_equal(r["status"], Z["gstatus"])
    assert abs(r["cost"][agent] - highs_cost) <= 5e-8 * highs_cost
    if seed == 4800332:
        assert np.abs(r["traj"][agent] - Z["gtraj"][agent]).max() <= 5e-6      # (the recorded plan is 1.2e-7 m from HiGHS's)


def _safety_reference(traj, times, dt, radius, downwash):
    """MultiSyncSimulator::savePlanningResult's pair loop (src/multi_sync_simulator.cpp:446-503) with octomap's float arithmetic."""
    from math import comb
    N = traj.shape[0]
    ratio = np.full((len(times), N), np.inf)
    partner = np.full((len(times), N), -1, np.int32)
    for ti, t in enumerate(times):
        m = min(int(t / dt), 4)
        tl = t / dt - m
        w = [comb(5, i) * pow(tl, i) * pow(1 - tl, 5 - i) for i in range(6)]
        pos = np.zeros((N, 3), np.float32)
        for q in range(N):
            for k in range(3):
                x = 0.0
                for i in range(6):
                    x += float(traj[q, k, 6 * m + i]) * w[i]
                pos[q, k] = np.float32(x)
        for qi in range(N):
            for qj in range(N):
                if qi == qj:
                    continue
                ra, rb = radius[qi], radius[qj]
                dw = (downwash[qi] * ra + downwash[qj] * rb) / (ra + rb)
                d = pos[qi] - pos[qj]
                d[2] = np.float32(float(d[2]) / dw)
                n2 = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                r = np.sqrt(float(n2)) / (ra + rb)
                if r < ratio[ti, qi]:
                    ratio[ti, qi], partner[ti, qi] = r, qj
    return ratio, partner


def test_safety_ratio_accounting_equals_the_reference_pair_loop():
    import lsc_planner_amd as L
    from lsc_planner_amd.planner import PlannerConfig
    ms = L.random_swarm(48, world=(-3, -3, 0, 3, 3, 2.5), seed=31)
    ms.radius[:] = np.random.default_rng(3).uniform(0.1, 0.2, 48)
    ms.downwash[:] = np.random.default_rng(4).uniform(1.0, 2.5, 48)
    pl = L.SwarmPlanner(ms, PlannerConfig(goal_mode="static"))
    times = [0.0, 0.1, 0.17]

    def accounted(tick, state, traj, outs):
        ratio, partner, mn = pl.safety_ratio(times)
        ref_ratio, ref_partner = _safety_reference(outs[0]["traj"], times, 0.2, ms.radius, ms.downwash)
        assert np.array_equal(ratio, ref_ratio)
        assert np.array_equal(partner, ref_partner)
        assert mn == ref_ratio.min()
    fly(pl, ms, 4, each_tick=accounted)
    pl.close()


def test_sweep_with_float32_margins_is_the_rounded_double_sweep():
    import torch
    import lsc_planner_amd as L
    from lsc_planner_amd.planner import PlannerConfig
    ms = L.circle_swap(24, 4.0)
    pl = L.SwarmPlanner(ms, PlannerConfig(goal_mode="static"))
    dev = torch.device("cuda", 0)
    state = torch.zeros((24, 9), dtype=torch.float32, device=dev)
    state[:, :3] = torch.from_numpy(ms.start).to(dev)
    state[:, 3:6] = 0.3
    prev = torch.zeros((24, 90), dtype=torch.float32, device=dev)
    n64 = torch.empty((24, 23, 5, 3), dtype=torch.float32, device=dev)
    n32 = torch.empty_like(n64)
    d64 = torch.empty((24, 23, 5, 6), dtype=torch.float64, device=dev)
    d32 = torch.empty((24, 23, 5, 6), dtype=torch.float32, device=dev)
    pl.sweep_device(state, prev, 1, n64, d64)
    pl.sweep_device(state, prev, 1, n32, d32)
    torch.cuda.synchronize()
    assert torch.equal(n64, n32)
    assert torch.equal(d64.to(torch.float32), d32)
    pl.close()


def test_plans_do_not_depend_on_what_the_lds_held_before():
    """The parity cases once more through the poison build of the plan, goal and general kernels (make poison: every byte of the
    workgroup's LDS is 0xff at entry).  A read of LDS that was never written -- harmless while the previous kernel left numbers there -- fails them."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "lsc_planner_amd", "liblsc_hip_poison.so")
    if not os.path.exists(lib):
        pytest.skip("liblsc_hip_poison.so not built (make -C lsc_planner_amd/csrc poison)")
    env = dict(os.environ, LSC_HIP_LIB=lib)
    # (test_gpu_highs_variants.py: the corridor, planar, four-segment and throughput-build QPs against HiGHS's verdicts, through every solver path,
    #  and the obs family's QPs through the three plan kernels of a context with dynamic obstacles; its obs_m4 cases take LSC_HIP_LIB_M4 below)
    files = [os.path.join(root, "tests", f) for f in ("test_gpu_parity.py", "test_gpu_edges.py", "test_gpu_goal.py", "test_gpu_modes.py",
                                                      "test_gpu_highs_variants.py")]
    # ... and the M = 4 instantiation through ITS poison build (round 5: `make poison_m4`, LSC_HIP_LIB_M4): its twisted factorisation has
    # sweeps of different lengths and its unmasked loads rest on the same "S.K is zero outside the band" invariant
    lib4 = os.path.join(root, "lsc_planner_amd", "liblsc_hip_m4_poison.so")
    if os.path.exists(lib4):
        env["LSC_HIP_LIB_M4"] = lib4
        files.append(os.path.join(root, "tests", "test_gpu_round4.py") + "::test_four_segments_the_reference_s_cpp_defaults")
        files.append(os.path.join(root, "tests", "test_gpu_round4.py") + "::test_four_segments_in_the_forest_and_in_the_alternate_modes")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu"] + files, env=env, cwd=root, capture_output=True, text=True,
                       timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:]
