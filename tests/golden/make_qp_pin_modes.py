"""HiGHS verdicts on the QPs of the alternate planner modes -- the modes family of tests/pin_variants.py --, for replay THROUGH THE KERNEL on
the GPU box (tests/test_gpu_highs_variants.py) and through the oracle anywhere (tests/test_oracle_pin_variants.py).

Every scene (pin_variants.MODES_SCENES / MODES_PARAMS) is flown closed-loop on the CPU by the oracle of the alternate modes
(oracle/lsc_oracle_modes.c through O.SwarmEx: the disturbance checks, then the tick); the scene's events push agents together, give them
velocities beyond their limit or move them off their plans.  Every tick from 1 is recorded -- an infeasible agent keeps the last plan its
context solved, and the reset's slack set only grows -- with the agents' states, the previous plans and, per agent, HiGHS's verdict (the
slack variables are ordinary variables of the QP), cost, point and x_ok, and whether a slack variable is positive at HiGHS's point
(pin_variants.slack_is_positive).  On the ticks of `rows_ticks` the oracle's rows (normals float32, margins float64) are recorded too.

Run in the build container (SciPy's bundled HiGHS):  python tests/golden/make_qp_pin_modes.py [scene ...]
Writes tests/golden/qp_pin_modes.npz (with scene names: flies and judges those alone, prints their counts and writes nothing).  The scenes'
pushes, seeds and tick counts were picked until the REFERENCE SOLVERS ALONE (HiGHS and the oracle, no kernel) met
pin_variants.MODES_CONDITIONS; this script asserts them, and both test files assert them again on the arrays.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import highs_qp as H  # noqa: E402
import pin_variants as PV  # noqa: E402


def rows_ticks_of(name, hist):
    """Ticks whose rows are recorded: the first two (constant-velocity and shifted predictions), the first with an infeasible agent, the
    first with an event, and the last; of the 64-agent crowd the first alone (its rows are 63 per agent)."""
    if name == "crowd":
        return [1]
    first = [t for t, (_, _, o) in enumerate(hist, 1) if (o["status"] == 1).any()][:1]
    event = sorted(PV.MODES_PARAMS[name]["events"])[:1]
    return sorted({1, min(2, len(hist)), len(hist)} | set(first) | set(event))


def record(out, fam, i, name, ms, prm, md, hist):
    """Verdicts of every tick of one flown scene into `out`; prints the counts."""
    from oracle import oracle as O
    key = f"{fam}{i}_"
    for k in PV.MISSION_KEYS:
        out[key + k] = getattr(ms, k)
    T = len(hist)
    out[key + "kept"] = np.arange(1, T + 1, dtype=np.int32)
    out[key + "states"] = np.array([h[0] for h in hist])
    out[key + "trajs"] = np.array([h[1] for h in hist])
    out[key + "ostatus"] = out[key + "ostatus_kept"] = np.array([h[2]["status"] for h in hist], np.int32)
    out[key + "slack_set"] = np.array([h[2]["slack_set"] for h in hist], np.uint8)
    rt = rows_ticks_of(name, hist)
    out[key + "rows_ticks"] = np.asarray(rt, np.int32)
    out[key + "normal"] = np.array([hist[t - 1][2]["normal"] for t in rt])
    out[key + "d"] = np.array([hist[t - 1][2]["d"] for t in rt])
    V, C, X, OK, SL = [], [], [], [], []
    for tick, (state, traj, o) in enumerate(hist, 1):
        sl = np.zeros(ms.qn, bool)
        v, c, x, ok = PV.modes_tick_verdicts(O, H, fam, name, prm, md, ms, state, traj, tick, o, slack=sl)
        V.append(v); C.append(c); X.append(x); OK.append(ok); SL.append(sl)
        opt = (v == 0) | (v == 2)
        agree = bool(((v < 0) | (np.minimum(v, 1) == o["status"]) | (v == 2)).all())
        print(f"{name} (n {ms.qn}) tick {tick}: infeasible {int((v == 1).sum())} optimal {int((v == 0).sum())} upper bounds {int((v == 2).sum())}"
              f" none {int((v < 0).sum())} x far {int((opt & ~ok).sum())} |f| >= 1e3 {int((opt & (np.abs(c) >= PV.LARGE_COST)).sum())}"
              f" slack positive {int((opt & sl).sum())} in slack sets {int(o['slack_set'].sum())}  oracle agrees {agree}", flush=True)
    out[key + "verdict"], out[key + "cost"], out[key + "x"] = np.array(V), np.array(C), np.array(X)
    out[key + "xok"], out[key + "slack"] = np.array(OK), np.array(SL)
    out[key + "judged"] = np.ones((T, ms.qn), bool)


def main(only):
    from oracle import oracle as O
    out = {}
    for fam in PV.MODES_FAMILIES:
        with O.segments(PV.family_params(fam)[0]):
            for i, name in enumerate(PV.MODES_SCENES[fam]):
                if only and name not in only:
                    continue
                ms, prm, md, hist = PV.fly_modes(O, fam, name)
                record(out, fam, i, name, ms, prm, md, hist)
        out[fam + "_count"] = np.int32(len(PV.MODES_SCENES[fam]))
    if only:
        for fam in PV.MODES_FAMILIES:
            for i, name in enumerate(PV.MODES_SCENES[fam]):
                if name in only:
                    v, ok = out[f"{fam}{i}_verdict"], out[f"{fam}{i}_xok"]
                    opt = (v == 0) | (v == 2)
                    print(name, "judged", v.size, "infeasible", int((v == 1).sum()), "optimal", int(opt.sum()), "none", int((v < 0).sum()), "x far", int((opt & ~ok).sum()),
                          "large", int((opt & (np.abs(out[f"{fam}{i}_cost"]) >= PV.LARGE_COST)).sum()), "slack", int((opt & out[f"{fam}{i}_slack"]).sum()))
        return
    out["solver"] = np.array("HiGHS " + H.version() + " (scipy.optimize._highspy)")
    path = os.path.join(HERE, PV.FILES["modes"])
    np.savez_compressed(path, **out)
    Z = np.load(path)
    for fam in PV.MODES_FAMILIES:
        print(f"{fam}: (certified infeasible, optimal, no verdict, optimal with x far, blocked) = {PV.counts(Z, fam)}")
    got = PV.modes_conditions(Z)
    print("conditions:", got)
    print(f"{path}: {os.path.getsize(path)} bytes", flush=True)
    PV.assert_modes_conditions(got)
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1:])
