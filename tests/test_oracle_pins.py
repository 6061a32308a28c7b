"""Pins of the oracle's QP optimum and of its infeasible verdict against an independent solver (HiGHS, tests/highs_qp.py).

CPLEX -- what the reference calls (src/traj_optimizer.cpp:76-153) -- is absent, and no reference fixture holds an optimum.
What can be pinned without it:
  1. the reference's OWN fixture log/QPmodel.lp, read by HiGHS's own LP-file reader: same dimensions as our parse of it,
     and infeasible (the file is written when CPLEX fails, src/traj_optimizer.cpp:100-102);
  2. the optimum of a strictly convex QP is unique and infeasibility is a property of the rows, so for >1000 QPs the
     oracle assembles on golden ticks and on seeded soak missions (sparse and dense: hundreds of infeasible ones),
     HiGHS's active-set QP solver must return the oracle's cost to <= 1e-7 relative (never a better feasible point;
     where HiGHS itself stops short -- <1 % of instances -- the oracle's point is checked to be feasible and better), and
     for every status-1 verdict a phase-1 LP must have a strictly positive minimal violation.
The kernel is compared with the oracle on the same kind of QPs in tests/test_gpu_soak.py, so the chain
kernel == oracle == HiGHS closes on cost and on the feasibility verdict.
"""
import json
import os

import numpy as np
import pytest

import highs_qp as H
from conftest import GOLDEN, golden_mission

pytestmark = pytest.mark.skipif(not H.available(), reason="scipy's bundled HiGHS is not importable")

REF_LP = os.path.join(GOLDEN, "QPmodel.lp")          # the reference's log/QPmodel.lp, byte for byte (tests/golden/make_reference_data_golden.py)
COST_RTOL = 1e-7
COST_ATOL = 1e-8          # costs go to zero when an agent hovers at its goal (same floor as tests/test_gpu_parity.py)


def _agent_qp(O, prm, ms, a, state, goal, obs_trajs, normal, d):
    """QP of agent a in the reference's row order, from one oracle tick's inputs and its LSC dump."""
    others = [j for j in range(ms.qn) if j != a]
    return O.qp_assemble(prm, state[a], goal[a], float(ms.nominal_velocity[a]), ms.max_vel[a], ms.max_acc[a], obs_trajs[others],
                         normal[a], d[a])


def _check_against_highs(qp, status, cost):
    """One QP: oracle verdict (status, cost) against HiGHS.  Returns 'opt' / 'inf'."""
    A, lo, hi = H.rows_of(qp)
    if status == 0:
        ms_, x, obj, viol = H.solve_oracle_qp(qp)
        if ms_ in ("Solve error", "Time limit reached"):
            return "gave_up"                                 # HiGHS's active-set code abandons a few degenerate instances
        assert ms_ == "Optimal", ms_
        assert viol <= 1e-7, viol                            # the point HiGHS calls optimal satisfies the ORIGINAL rows
        tol = COST_RTOL * abs(cost) + COST_ATOL
        # the direction that could expose the oracle: an independent solver must never find a better feasible point
        assert obj >= cost - tol, (obj, cost)
        if obj <= cost + tol:
            return "opt"
        # HiGHS's "optimum" is WORSE than the oracle's (its active-set code stops ~1e-6 short on a few instances).  That
        # says nothing against the oracle provided the oracle's own point really is feasible: re-solve in double and check
        # it against the original rows.
        st, xo, co, _, _ = qp.solve()
        assert st == 0 and co == cost
        vo = max(np.max(lo - A @ xo), np.max(A @ xo - hi), np.max(qp.lo - xo), np.max(xo - qp.hi))
        # (+ 1e-7: near the goal the cost goes to 1e-3 and HiGHS's shortfall stays ~1e-8 absolute -- seen once the oracle finished its optimum exactly, round 5)
        assert vo <= 1e-9 and obj - cost <= 1e-5 * abs(cost) + 1e-7, (vo, obj, cost)
        return "highs_short"
    ms_, t = H.min_violation(A, lo, hi, qp.lo, qp.hi)
    assert ms_ == "Optimal" and t > 1e-7, (ms_, t)          # the rows cannot all hold: certificate of infeasibility
    ms_, _, _, _ = H.solve_oracle_qp(qp)
    assert ms_ in ("Infeasible", "Solve error", "Time limit reached"), ms_
    return "inf"


def test_highs_reads_the_reference_fixture_itself_and_finds_it_infeasible():
    """No parser of ours in between: HiGHS reads log/QPmodel.lp verbatim."""
    lp = json.load(open(os.path.join(GOLDEN, "qpmodel_lp.json")))
    status, rows, cols, hnz = H.read_lp_file(REF_LP)
    assert (rows, cols) == (len(lp["rows"]), 90) == (546, 90)
    assert hnz == len({(min(i, j), max(i, j)) for i, j, _ in lp["quad"]})      # same quadratic objective entries as our parse
    assert status == "Infeasible"
    pin = json.load(open(os.path.join(GOLDEN, "qp_pins.json")))
    assert pin["reference_lp"]["highs_status"] == status and pin["reference_lp"]["rows"] == rows


def test_parsed_fixture_is_infeasible_for_highs_and_for_the_oracle(oracle):
    """The same instance through our parse (tests/golden/qpmodel_lp.json, travels to the GPU box): HiGHS's verdict, the
    oracle's verdict and the recorded verdict of HiGHS on the reference file agree."""
    from test_oracle_qp import _scene_qp
    lp = json.load(open(os.path.join(GOLDEN, "qpmodel_lp.json")))
    qp, _ = _scene_qp(oracle, lp)
    st, x, cost, it, kkt = qp.solve()
    assert st == 1
    assert _check_against_highs(qp, st, cost) == "inf"
    A, lo, hi = H.rows_of(qp)
    _, t = H.min_violation(A, lo, hi, qp.lo, qp.hi)
    assert abs(t - 0.0385092) < 1e-6                         # the LP-minimal uniform violation
    pin = json.load(open(os.path.join(GOLDEN, "qp_pins.json")))
    assert pin["reference_lp"]["highs_status"] == "Infeasible"


def test_every_agent_of_the_golden_ticks_vs_highs(oracle, ticks):
    """All agents of all committed snapshots (56 QPs), not a sample."""
    n = 0
    for name, keep in (("multi_simple4", (1, 2, 3, 20)), ("multi_circle20", (1, 15))):
        ms = golden_mission(ticks, name)
        prm = oracle.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True)
        for tick in keep:
            g = lambda k: ticks[f"{name}/tick{tick}/{k}"]
            state, prev = g("state"), g("prev")
            obs = np.array([oracle.shift_traj(p) for p in prev]) if tick >= 2 else \
                np.array([oracle.const_vel_traj(state[j, :3], state[j, 3:6]) for j in range(ms.qn)])
            for a in range(ms.qn):
                qp = _agent_qp(oracle, prm, ms, a, state, ms.goal, obs, g("normal"), g("d"))
                st, x, cost, it, kkt = qp.solve()
                assert st == 0 and abs(cost - g("cost")[a]) <= 1e-9 * abs(cost)
                _check_against_highs(qp, st, cost)
                n += 1
    assert n == 56


@pytest.mark.parametrize("dense", [False, True])
def test_soak_qps_optimum_and_infeasibility_vs_highs(oracle, dense):
    """Seeded random missions like tests/test_gpu_soak.py (dense = packed so tightly that many QPs are infeasible):
    the QPs of every tick through HiGHS.  > 1000 QPs in total, > 100 certified-infeasible ones in the dense run."""
    import lsc_planner_amd as L
    from lsc_planner_amd.planner import next_state_host
    rng = np.random.default_rng(777 + int(dense))
    n_opt = n_inf = n_gave_up = 0
    for trial in range(8 if dense else 6):
        n = int(rng.integers(10, 22)) if dense else int(rng.integers(4, 24))
        side = float(rng.uniform(0.9, 1.3)) if dense else float(rng.uniform(2.5, 5.0))
        ms = L.random_swarm(n, world=(-side, -side, 0, side, side, 2.5), seed=int(rng.integers(1, 1 << 30)),
                            min_sep=0.33 if dense else 0.5, shrink=0.15 if dense else 0.4)
        if trial % 3 == 0:
            ms.radius[:] = rng.uniform(0.1, 0.25, n)
            ms.downwash[:] = rng.uniform(1.0, 2.5, n)
            ms.max_vel[:] = rng.uniform(0.6, 1.5, (n, 1))
            ms.max_acc[:] = rng.uniform(1.0, 3.0, (n, 1))
        prm = oracle.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True)
        sw = oracle.Swarm(prm, ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
        state = np.zeros((n, 9), np.float32)
        state[:, :3] = ms.start
        traj = np.zeros((n, 3, 30), np.float32)
        for tick in range(1, 21 if dense else 9):
            o = sw.tick(state, ms.goal, traj, tick, want_lsc=True, nthreads=8)
            obs = np.array([oracle.shift_traj(p) for p in traj]) if tick >= 2 else \
                np.array([oracle.const_vel_traj(state[j, :3], state[j, 3:6]) for j in range(n)])
            for a in range(n):
                if dense and o["status"][a] == 0 and (a + tick) % 4:
                    continue        # dense run: EVERY infeasible verdict is certified, the feasible ones are sampled (1 in 4)
                qp = _agent_qp(oracle, prm, ms, a, state, ms.goal, obs, o["normal"], o["d"])
                kind = _check_against_highs(qp, int(o["status"][a]), float(o["cost"][a]))
                n_opt += kind == "opt"
                n_inf += kind == "inf"
                n_gave_up += kind in ("gave_up", "highs_short")
            traj = o["traj"]
            state = next_state_host(traj)
    assert n_opt + n_inf >= 500
    assert (n_inf > 100) == dense, (n_opt, n_inf)
    print(f"dense={dense}: {n_opt} optimal, {n_inf} infeasible, {n_gave_up} without a HiGHS verdict")
    assert n_gave_up <= 0.01 * (n_opt + n_inf), n_gave_up      # no verdict from HiGHS is not a disagreement, but must stay rare


@pytest.mark.parametrize("mode", ["bvc", "collision_constraint", "dynamical_limit", "reset"])
def test_alternate_mode_qps_vs_highs(oracle, mode):
    """the QPs of the alternate modes (BVC rows without the stop-at-horizon equalities; slack variables on the
    collision rows / on the dynamic limits; the slack rows a disturbance leaves behind) as the oracle assembles and solves
    them, against HiGHS with the slack variables as ordinary variables."""
    import lsc_planner_amd as L
    from lsc_planner_amd.planner import next_state_host
    O = oracle
    # slack modes with mode/planner = bvc: in LSC mode the reference fixes SlackMode to none (src/traj_planner.cpp:445-448)
    md = {"bvc": O.make_modes(planner="bvc"), "collision_constraint": O.make_modes(planner="bvc", slack="collision_constraint"),
          "dynamical_limit": O.make_modes(planner="bvc", slack="dynamical_limit"), "reset": O.make_modes(reset_threshold=0.15)}[mode]
    ms = L.circle_swap(8, 1.2, world=(-5, -5, 0, 5, 5, 2.5))
    N = ms.qn
    prm = O.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True)
    sw = O.SwarmEx(prm, md, ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
    state = np.zeros((N, 9), np.float32)
    state[:, :3] = ms.start
    traj = np.zeros((N, 3, 30), np.float32)
    checked = slack_vars = 0
    for tick in range(1, 13):
        if mode == "reset" and tick in (5, 9):
            state[tick % N, :3] += np.float32([0.25, -0.2, 0.05])          # a gust moves one agent off its plan
        own = sw.disturbance_update(state, traj, tick)
        o = sw.tick(state, ms.goal, traj, tick, want_lsc=True, nthreads=4)
        for a in range(N):
            others = [j for j in range(N) if j != a]
            obs = []
            for j in others:
                if mode in ("bvc", "collision_constraint", "dynamical_limit") or sw.slack_set[a, j] and np.linalg.norm(
                        (O.shift_traj(traj[j]) if tick >= 2 else O.const_vel_traj(state[j, :3], state[j, 3:6]))[:, 0] - state[j, :3]) > 0.15:
                    obs.append(np.repeat(state[j, :3, None], 30, axis=1))
                else:
                    obs.append(O.shift_traj(traj[j]) if tick >= 2 else O.const_vel_traj(state[j, :3], state[j, 3:6]))
            qp = O.qp_assemble_ex(prm, md, state[a], ms.goal[a], float(ms.nominal_velocity[a]), ms.max_vel[a], ms.max_acc[a],
                                  np.array(obs, np.float32), o["normal"][a], o["d"][a], slack_flags=sw.slack_set[a, others])
            st, x, cost, it, kkt = qp.solve()
            assert st == o["status"][a] and (st != 0 or abs(cost - o["cost"][a]) <= 1e-9 * abs(cost) + 1e-12), (tick, a)
            kind = _check_against_highs(qp, st, cost)
            checked += kind in ("opt", "inf")
            slack_vars = max(slack_vars, qp.nv - 90)
        traj = o["traj"]
        state = next_state_host(traj)
    assert checked >= 90
    assert slack_vars == {"bvc": 0, "collision_constraint": 35, "dynamical_limit": 10, "reset": 35}[mode]


# (3400814: found by round 3's large-count run, tools/fuzz_round.sh -- a gust case where the ORACLE stops 7.7e-9 relative above the
#  optimum with its plan 1.7e-4 m from HiGHS's, while the kernel's recorded plan is within 1.2e-5 m of it: the fuzzer compares plans
#  against the oracle and flagged the kernel)
# (4800332: round 4's run of tests/fuzz_modes.py -- BVC with the dynamical-limit slack, |f| = 1860: the oracle stops 1.2e-8 relative above the optimum
#  with its plan 6.7e-5 m from HiGHS's, the kernel's recorded plan is 1.2e-7 m from it; same answer from round 3's kernel)
@pytest.mark.parametrize("seed,agent,highs_cost", [(5023, 2, 1.3618641918561454), (5059, 6, 106.74117597754659),
                                                   (3400814, 2, 837.1755490814921), (4800332, 2, 1860.235625116953)])
def test_instances_on_which_the_oracle_used_to_give_up(oracle, seed, agent, highs_cost):
    """Found by tests/test_gpu_fuzz.py: alternate-mode QPs close to a degenerate optimum, where the oracle's normal equations
    lose definiteness.  It used to answer "infeasible"; HiGHS (cost recorded here, re-derived when HiGHS is importable) and the
    kernel (cost and plan in the fixture, produced on an MI355X) agree on the optimum.  Inputs: tests/golden/fuzz_found_*.npz
    (the tick's states, previous plans, persistent slack set and the seeded agents of the fuzzer)."""
    O = oracle
    Z = np.load(os.path.join(GOLDEN, "fuzz_found_%d.npz" % seed))
    modes = [dict(planner="bvc"), dict(planner="bvc", slack="collision_constraint"), dict(planner="bvc", slack="dynamical_limit"),      # (MODES of tests/fuzz_modes.py)
             dict(planner="bvc", n_constraint_segments=2), dict(reset_threshold=0.15)]
    mk = modes[int(Z["which"])]
    md = O.make_modes(**mk)
    state, traj, goal, tick = Z["state"], Z["traj"], Z["goal"], int(Z["tick"])
    n = len(state)
    prm = O.make_params(world_min=Z["wmin"], world_max=Z["wmax"], obs_f32=True)
    sw = O.SwarmEx(prm, md, Z["radius"], Z["dw"], Z["vmax"], Z["amax"], Z["vnom"])
    sw.slack_set[:] = Z["slack"]
    sw.stale[:] = Z["stale"]
    o = sw.tick(state, goal, traj, tick, want_lsc=True, nthreads=2)
    assert (o["status"] == 0).all() and np.array_equal(o["status"], Z["gstatus"])
    assert abs(o["cost"][agent] - highs_cost) <= 1e-7 * highs_cost
    assert abs(Z["gcost"][agent] - highs_cost) <= 1e-8 * highs_cost           # the kernel's answer on the same inputs
    assert (np.abs(o["cost"] - Z["gcost"]) <= 1e-6 * np.abs(Z["gcost"])).all()
    if H.available():
        others = [j for j in range(n) if j != agent]
        bvc = mk.get("planner") == "bvc"
        obs = []
        for j in others:
            pred = O.shift_traj(traj[j]) if tick >= 2 else O.const_vel_traj(state[j, :3], state[j, 3:6])
            moved = sw.slack_set[agent, j] and np.linalg.norm(pred[:, 0] - state[j, :3]) > 0.15
            obs.append(np.repeat(state[j, :3, None], 30, axis=1) if (bvc or moved) else pred)
        qp = O.qp_assemble_ex(prm, md, state[agent], goal[agent], float(Z["vnom"][agent]), Z["vmax"][agent], Z["amax"][agent],
                              np.array(obs, np.float32), o["normal"][agent], o["d"][agent], slack_flags=sw.slack_set[agent, others])
        verdict, xh, cost = H.solve_oracle_qp(qp)[:3]
        assert verdict == "Optimal" and abs(cost - highs_cost) <= 1e-8 * highs_cost
        if seed in (3400814, 4800332):          # both plans at the optimum (until round 4 only the kernel's was: see the test below)
            xh = np.asarray(xh)[:90].reshape(3, 30)
            assert np.abs(xh - Z["gtraj"][agent]).max() <= 2e-5 and np.abs(xh - o["traj"][agent]).max() <= 2e-5


@pytest.mark.parametrize("seed,agent,highs_cost", [(6800157, 0, 4258.793418172383), (6800522, 0, 16.849414817360), (7301082, 3, 3523.9260890555174)])
def test_instances_that_found_the_cancellation_in_the_oracle(oracle, seed, agent, highs_cost):
    """Round 4, tests/fuzz_modes.py: BVC with the dynamical-limit slack (penalty 1e5).  On 6800157 the oracle used to end 3.6e-6 relative
    above the optimum -- outside the 1e-6 of the tolerance table it is the yardstick of --, on 6800522 5.8e-7 above with its plan
    1.2e-4 m away, while HiGHS and the kernel (recorded on an MI355X) agreed to 2e-8.  Cause, found with these two: the oracle formed
    the Newton right-hand side as  -rd - Z'G'((z rp - s z) / s),  two sums that each carry the multipliers z and cancel them between
    each other; with z in the 1e10s close to a degenerate optimum the difference had no digits left, the multipliers wandered, and the
    Newton-step test ended the run on damped steps.  Formed as  -(Hy y + gy) - Z'G'(z rp / s)  (what the kernel has always done) and
    with a quadruple-precision assembly / LDL' of K for the iterations whose double-precision K is no longer positive definite (instead
    of a diagonal shift), the oracle reaches the same optimum as HiGHS and the kernel -- here and on every earlier "the oracle's plan is
    the distant one" fixture (3400814, 4800332, m4_4602619), which were this defect, not flat optima.
    7301082 is what the corrected solver then met: a slack-mode QP whose optima form a face.  The value is final after eleven iterations
    (HiGHS, kernel and this solver: 3523.9260890), but the iterates drift along the face, the Newton step never gets small and the
    multipliers of the degenerate rows have no limit, so neither convergence test fires -- the run ended "infeasible" at the iteration
    cap.  The solver now also stops when it is feasible, complementary to 1e-7 and the objective has not moved by 1e-9 for three
    iterations in a row; the plans of such a QP are not comparable (and are not compared above |f| = 1e3)."""
    O = oracle
    Z = np.load(os.path.join(GOLDEN, "fuzz_found_%d.npz" % seed))
    assert int(Z["which"]) == 2
    mk = dict(planner="bvc", slack="dynamical_limit")
    md = O.make_modes(**mk)
    state, traj, goal, tick = Z["state"], Z["traj"], Z["goal"], int(Z["tick"])
    n = len(state)
    prm = O.make_params(world_min=Z["wmin"], world_max=Z["wmax"], obs_f32=True)
    sw = O.SwarmEx(prm, md, Z["radius"], Z["dw"], Z["vmax"], Z["amax"], Z["vnom"])
    sw.slack_set[:] = Z["slack"]
    sw.stale[:] = Z["stale"]
    o = sw.tick(state, goal, traj, tick, want_lsc=True, nthreads=2)
    assert (o["status"] == 0).all() and np.array_equal(o["status"], Z["gstatus"])
    assert abs(Z["gcost"][agent] - highs_cost) <= 5e-8 * highs_cost                       # the kernel's answer on the same inputs
    assert abs(o["cost"][agent] - highs_cost) <= 5e-8 * highs_cost                        # ... and now the oracle's
    assert abs(o["cost"][agent] - Z["gcost"][agent]) <= 1e-9 * highs_cost                 # (HiGHS is the loosest of the three)
    assert (np.abs(o["cost"] - Z["gcost"]) <= 1e-6 * np.abs(Z["gcost"])).all()
    others = [j for j in range(n) if j != agent]
    assert np.abs(o["traj"] - Z["gtraj"])[others if seed == 7301082 else slice(None)].max() <= 5e-6
    if H.available():
        obs = [np.repeat(state[j, :3, None], 30, axis=1) for j in others]                 # BVC: obstacles at their current positions
        qp = O.qp_assemble_ex(prm, md, state[agent], goal[agent], float(Z["vnom"][agent]), Z["vmax"][agent], Z["amax"][agent],
                              np.array(obs, np.float32), o["normal"][agent], o["d"][agent], slack_flags=sw.slack_set[agent, others])
        verdict, xh, cost = H.solve_oracle_qp(qp)[:3]
        assert verdict == "Optimal" and abs(cost - highs_cost) <= 1e-8 * highs_cost
