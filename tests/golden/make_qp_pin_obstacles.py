"""HiGHS verdicts on the QPs of swarms that plan against dynamic obstacles -- the obs family of tests/pin_variants.py --, for replay THROUGH
THE KERNEL on the GPU box (tests/test_gpu_highs_variants.py) and through the composed reference anywhere (tests/test_oracle_pin_variants.py).

Every mission (pin_variants.OBS_SCENES / OBS_PARAMS) is flown closed-loop on the CPU: lsc_planner_amd/obstacles.py::ObstacleSet moves the
obstacles from the agents' float32 states, tests/obstacle_reference.py::ObstacleSwarm plans.  Every tick from 1 is recorded -- the
stale-trajectory rule has a history -- with the agents' states, the previous plans, the obstacles' float32 [K][6] states and, per agent,
HiGHS's verdict, cost, point and x_ok, and whether a row of an obstacle is active at HiGHS's point.  On the ticks of `rows_ticks` the composed
reference's rows (normals float32, margins float64, the other agents by index and then the obstacles) are recorded too.

Run in the build container (SciPy's bundled HiGHS):  python tests/golden/make_qp_pin_obstacles.py
Writes tests/golden/qp_pin_obstacles.npz.  The scenes' speeds and seeds were picked until the REFERENCE SOLVERS ALONE (HiGHS and the composed
reference, no kernel) met pin_variants.OBS_CONDITIONS; this script asserts them, and both test files assert them again on the arrays.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import highs_qp as H  # noqa: E402
import pin_variants as PV  # noqa: E402


def rows_ticks_of(hist):
    """Ticks whose rows are recorded: the first two (constant-velocity and shifted predictions of the agents), the first with an infeasible
    agent, and the last."""
    first = [t for t, (_, _, o) in enumerate(hist, 1) if (o["status"] == 1).any()][:1]
    return sorted({1, min(2, len(hist)), len(hist)} | set(first))


def record(out, fam, i, name, ms, obstacles, prm, hist):
    """Verdicts of every tick of one flown mission into `out`; prints the counts."""
    from lsc_planner_amd.obstacles import ObstacleSet
    from oracle import oracle as O
    key = f"{fam}{i}_"
    S = ObstacleSet(obstacles, n_agents=ms.qn)
    for k in PV.MISSION_KEYS:
        out[key + k] = getattr(ms, k)
    T = len(hist)
    out[key + "kept"] = np.arange(1, T + 1, dtype=np.int32)
    out[key + "states"] = np.array([h[0] for h in hist])
    out[key + "trajs"] = np.array([h[1] for h in hist])
    out[key + "obstacles"] = np.array([h[2]["obs"] for h in hist], np.float32)
    out[key + "obs_radius"], out[key + "obs_downwash"] = S.radius, S.downwash
    out[key + "ostatus"] = out[key + "ostatus_kept"] = np.array([h[2]["status"] for h in hist], np.int32)
    rt = rows_ticks_of(hist)
    out[key + "rows_ticks"] = np.asarray(rt, np.int32)
    out[key + "normal"] = np.array([hist[t - 1][2]["normal"] for t in rt])
    out[key + "d"] = np.array([hist[t - 1][2]["d"] for t in rt])
    V, C, X, OK, ACT = [], [], [], [], []
    for tick, (state, traj, o) in enumerate(hist, 1):
        act = np.zeros(ms.qn, bool)
        v, c, x, ok = PV.tick_verdicts(O, H, fam, prm, ms, state, traj, tick, o, active=act)
        V.append(v); C.append(c); X.append(x); OK.append(ok); ACT.append(act)
        agree = bool(((v < 0) | (np.minimum(v, 1) == o["status"]) | (v == 2)).all())
        print(f"{name} (n {ms.qn}, K {len(S)}) tick {tick}: infeasible {int((v == 1).sum())} optimal {int((v == 0).sum())} upper bounds {int((v == 2).sum())}"
              f" none {int((v < 0).sum())} x far {int((((v == 0) | (v == 2)) & ~ok).sum())} obstacle rows active {int(act.sum())}  reference agrees {agree}", flush=True)
    out[key + "verdict"], out[key + "cost"], out[key + "x"] = np.array(V), np.array(C), np.array(X)
    out[key + "xok"], out[key + "obs_active"] = np.array(OK), np.array(ACT)
    out[key + "judged"] = np.ones((T, ms.qn), bool)


def main():
    from oracle import oracle as O
    out = {}
    for fam in PV.OBS_FAMILIES:
        with O.segments(PV.family_params(fam)[0]):
            for i, name in enumerate(PV.OBS_SCENES[fam]):
                ms, obstacles, ticks = PV.obs_scene(name)
                prm, hist = PV.fly(O, fam, ms, ticks, obstacles=obstacles)
                record(out, fam, i, name, ms, obstacles, prm, hist)
        out[fam + "_count"] = np.int32(len(PV.OBS_SCENES[fam]))
    out["solver"] = np.array("HiGHS " + H.version() + " (scipy.optimize._highspy)")
    path = os.path.join(HERE, PV.FILES["obs"])
    np.savez_compressed(path, **out)
    Z = np.load(path)
    for fam in PV.OBS_FAMILIES:
        print(f"{fam}: (certified infeasible, optimal, no verdict, optimal with x far, blocked) = {PV.counts(Z, fam)}")
    got = PV.obs_conditions(Z)
    print("conditions:", got)
    print(f"{path}: {os.path.getsize(path)} bytes", flush=True)
    PV.assert_obs_conditions(got)
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
