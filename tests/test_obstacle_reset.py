"""CPU: dynamic obstacles under the disturbance reset -- the two rules of csrc/lsc_rules.hpp on the host against their float64 restatement
(tests/obstacle_reset_reference.py), and the scene "pushed hover" flown by the composed reference alone: what the GPU tests of
tests/test_gpu_obstacle_reset.py rest on."""
import os
import subprocess
from math import comb

import numpy as np
import pytest

from obstacle_reset_reference import (HOVER_DOWNWASH, HOVER_RADIUS, PUSHED_AGENT, PUSHED_BY, PUSHED_MAX_ACC, PUSHED_THRESHOLD, PUSHED_TICK,
                                      PUSHED_TICKS, ObstacleResetSwarm, fly_reference, hover_mission, hover_states, obstacle_size,
                                      uncertainty_segments)
from tolerances import FUZZ_PLAN_COMPARED_BELOW_COST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(v):
    return f"{np.array([v], np.float64).view(np.uint64)[0]:x}"


@pytest.mark.parametrize("m,dt", [(5, 0.2), (4, 0.5)])
def test_size_and_margin_rules_of_the_header_on_the_host(tmp_path, m, dt):
    """rule_uncertainty_segments, rule_obstacle_size and rule_slack_obstacle_margin, compiled for the host (tests/native/
    obstacle_size_check.cpp, M = 5 at dt 0.2 and M = 4 at dt 0.5), against the Python doubles bit for bit: horizons 0, 1.0 and M dt,
    max_acc 0 and seeded values, size prediction on and off."""
    src = os.path.join(ROOT, "tests", "native", "obstacle_size_check.cpp")
    exe = str(tmp_path / f"obstacle_size_check_m{m}")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-O2", "-std=c++17", f"-DLSC_SEGMENTS={m}", "-o", exe, src])
    rng = np.random.default_rng(20261021)
    cases = []
    for h in (0.0, 1.0, m * dt):
        for a in [0.0] + list(rng.uniform(0.05, 6.0, 12)):
            for flag in (1, 0):
                cases.append((float(np.float32(rng.uniform(0.05, 0.5))), float(a), dt, h, float(rng.uniform(0.05, 0.4)), flag))
    text = "\n".join(" ".join(_hex(v) for v in c[:5]) + f" {c[5]}" for c in cases) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(cases)
    grew = 0
    for (r_o, a, dt_, h, r_a, flag), line in zip(cases, out):
        words = line.split()
        M_u = uncertainty_segments(h, dt_)
        assert int(words[0]) == M_u and M_u == round(h / dt_), (h, dt_, words[0])
        got = np.array([int(w, 16) for w in words[1:]], np.uint64).view(np.float64).reshape(2, m, 6)
        size = np.array([[obstacle_size(r_o, a, dt_, M_u, flag, s, i) for i in range(6)] for s in range(m)])
        assert np.array_equal(got[0].view(np.uint64), size.view(np.uint64)), (r_o, a, h, flag)
        assert np.array_equal(got[1].view(np.uint64), (size + r_a).view(np.uint64)), (r_o, a, h, flag)
        if not flag or a == 0.0 or M_u == 0:
            assert (size == r_o).all()
        else:
            grew += 1
            # the control points ARE the degree-5 Bernstein form of r_o + 0.5 a (dt (s + t))^2 on every growing segment, and rest behind it
            for s in range(m):
                for t in (0.0, 0.3, 1.0):
                    val = sum(comb(5, i) * t ** i * (1 - t) ** (5 - i) * size[s, i] for i in range(6))
                    assert abs(val - (r_o + 0.5 * a * (dt_ * (min(s, M_u) + (t if s < M_u else 0.0))) ** 2)) < 1e-12, (s, t)
    assert grew >= 20


@pytest.fixture(scope="module")
def pushed_hover(oracle):
    ms = hover_mission()
    ref = ObstacleResetSwarm(oracle, ms, HOVER_RADIUS, HOVER_DOWNWASH, PUSHED_MAX_ACC, reset_threshold=PUSHED_THRESHOLD)
    return fly_reference(ref, ms, PUSHED_TICKS, hover_states, {PUSHED_TICK: (PUSHED_AGENT, PUSHED_BY)}, variants=("half", "no_growth"),
                         variant_ticks={PUSHED_TICK})


def test_pushed_hover_is_what_the_gpu_tests_need(pushed_hover):
    """The reference alone on "pushed hover" (hover's 8 agents and three spheres, max_acc (1.0, 0.5, 2.0), size prediction on, horizon 1.0,
    reset_threshold 0.15, agent 2 moved +0.3 m in x in front of tick 12, 20 ticks): no infeasible agent-tick, agent 2 flagged at tick 12
    and nobody before, every agent through the alternate QP from tick 12 on, agent 2's plan of tick 12 more than 1 cm from the plan with
    the half-separation margins and from the plan with full margins without growth, every cost below FUZZ_PLAN_COMPARED_BELOW_COST."""
    fl = pushed_hover
    status = np.stack([t["status"] for t in fl])
    assert status.shape == (PUSHED_TICKS, 8) and (status == 0).all(), np.argwhere(status != 0)
    for j, t in enumerate(fl, 1):
        if j < PUSHED_TICK:
            assert not t["own"].any() and not t["ever"].any() and not t["alt"].any(), j
        else:
            assert t["alt"].all() and t["ever"][PUSHED_AGENT] and t["ever"].sum() == 1, j
    t12 = fl[PUSHED_TICK - 1]
    assert list(np.flatnonzero(t12["own"])) == [PUSHED_AGENT]
    q = PUSHED_AGENT
    d_half = float(np.abs(t12["traj"][q] - t12["traj_half"][q]).max())
    d_flat = float(np.abs(t12["traj"][q] - t12["traj_no_growth"][q]).max())
    n_alt = int(sum(t["alt"].sum() for t in fl))
    n_slack = int(sum((t["slack_min"] < -1e-6).sum() for t in fl))
    print(f"alternate-QP agent-ticks {n_alt}, with a slack variable below -1e-6: {n_slack}; tick 12, agent 2: {d_half:.4f} m from the "
          f"half-separation plan, {d_flat:.4f} m from the plan without growth")
    assert t12["status_half"][q] == 0 and t12["status_no_growth"][q] == 0
    assert d_half > 0.01 and d_flat > 0.01, (d_half, d_flat)
    assert n_alt == 8 * (PUSHED_TICKS - PUSHED_TICK + 1)
    assert max(float(t["cost"].max()) for t in fl) < FUZZ_PLAN_COMPARED_BELOW_COST


def test_generated_scenes_are_telling(oracle):
    """The two scenes the GPU tests fly beside "pushed hover", on the reference alone: at most a quarter of the agent-ticks infeasible, and
    a sphere's full-margin row moves a plan by more than 1 mm (scene_is_telling)."""
    from obstacle_reset_reference import (CROWD_AGENT, CROWD_MAX_ACC, CROWD_PUSH_TICK, CROWD_TICKS, M4_DT, M4_PUSH_TICK, M4_TICKS, crowd_scene,
                                          scene_is_telling)
    with oracle.segments(4):
        ms = hover_mission()
        ref = ObstacleResetSwarm(oracle, ms, HOVER_RADIUS, HOVER_DOWNWASH, PUSHED_MAX_ACC, reset_threshold=PUSHED_THRESHOLD, dt=M4_DT)
        fl = fly_reference(ref, ms, M4_TICKS, lambda j: hover_states(j, dt=M4_DT), {M4_PUSH_TICK: (PUSHED_AGENT, PUSHED_BY)}, dt=M4_DT,
                           variants=("half",))
        print("M = 4 hover: a full-margin row moves a plan by", scene_is_telling(fl), "m; infeasible agent-ticks",
              int(sum((t["status"] != 0).sum() for t in fl)))
        assert fl[M4_PUSH_TICK - 1]["own"][PUSHED_AGENT] and not fl[M4_PUSH_TICK - 2]["ever"].any()
    ms, rad, dw, states_of = crowd_scene()
    ref = ObstacleResetSwarm(oracle, ms, rad, dw, CROWD_MAX_ACC, reset_threshold=PUSHED_THRESHOLD)
    fl = fly_reference(ref, ms, CROWD_TICKS, states_of, {CROWD_PUSH_TICK: (CROWD_AGENT, PUSHED_BY)}, variants=("half",))
    print("crowd: a full-margin row moves a plan by", scene_is_telling(fl), "m; infeasible agent-ticks",
          int(sum((t["status"] != 0).sum() for t in fl)))
    assert fl[CROWD_PUSH_TICK - 1]["own"][CROWD_AGENT] and not fl[CROWD_PUSH_TICK - 2]["ever"].any()
