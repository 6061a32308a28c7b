"""HiGHS verdicts on the QP variants the 90-variable empty-map pins (make_qp_pin_ticks.py) never reach, for replay THROUGH THE KERNEL on the
GPU box (tests/test_gpu_highs_variants.py) and through the oracle anywhere (tests/test_oracle_pin_variants.py).  Four families
(tests/pin_variants.py): corridor QPs on the forest map, the planar 60-variable QP, the four-segment 72-variable QP, and one tick of the
320-agent swarm that the throughput build plans.  Per kept agent: HiGHS's verdict, its cost, its point rounded to float32 in the traj layout
and whether that point and the oracle's plan agree to TRAJ_ATOL / 2 (x_ok).

Run in the build container (SciPy's bundled HiGHS):  python tests/golden/make_qp_pin_variants.py [family ...]
Writes tests/golden/qp_pin_variants.npz (planar, m4), qp_pin_corridor.npz (the corridor family records every tick of its missions -- the boxes
have a history -- and would not fit the size limit of a committed file next to the others) and qp_pin_tp.npz.  The missions are seeded; the
seeds and densities below were picked until the REFERENCE SOLVERS ALONE (HiGHS and the oracle, no kernel) met the conditions that both test
files assert: per family at least 10 certified-infeasible and 60 optimal agent-ticks, at most 10 % without a verdict, x_ok false for at most
5 % of the optimal ones.  The QP rows come from the oracle's assembly, which log/QPmodel.lp pins.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import highs_qp as H  # noqa: E402
import pin_variants as PV  # noqa: E402

# corridor: (agents, half side of the world, seed, ticks flown, ticks kept besides those on which an agent first turns infeasible)
#   min_clearance 0.25 lets a few seeds start so close to a trunk that their first box is blocked (status 4 at tick 1): those agents are
#   infeasible on every later tick.  The third mission holds an agent that is infeasible for five ticks and then recovers.
CORRIDOR = [(24, 2.0, 11, 14, (2, 8, 14)), (36, 2.5, 12, 5, (2, 5)), (36, 2.5, 13, 6, (2, 6))]
# planar, m4: (agents, half side, seed); the first tick that holds an infeasible QP and ticks 8 and 14 are kept, as make_qp_pin_ticks.py does.
#   planar: a 3-D swarm (separation scaled by the downwash in z) put into the plane z = world_z_2d = 1.0: some agents start inside another's
#   collision model, a third to a half of the QPs are infeasible.
#   m4: with half-second segments a swarm of uniform agents this dense has no infeasible QP at all (two seconds to stop in); the agents are the
#   mixed ones of make_qp_pin_ticks.py (radius 0.1-0.25, downwash 1-2.5, v_max 0.6-1.5, a_max 1-3).  The last mission's infeasible QP is
#   feasible again on the second tick.
PLANAR = [(14, 1.5, 101), (20, 1.9, 102), (16, 1.6, 103), (18, 1.8, 104)]
M4 = [(16, 1.2, 204), (20, 1.4, 213), (12, 1.0, 214), (14, 1.0, 217)]
TP = dict(n=320, world=(-12, -12, 0, 12, 12, 3), seed=9, tick=6, subset=40, subset_seed=2026)


def _swarm(fam, n, side, seed):
    import lsc_planner_amd as L
    from oracle import oracle as O
    if fam == "corridor":
        w = (-side, -side, 0, side, side, 2.5)
        dm, _ = PV.forest_distmap(O, w[:3], w[3:])
        return L.random_swarm(n, world=w, seed=seed, min_sep=0.31, shrink=0.15, edt=dm.dist, edt_key_min=dm.key_min, min_clearance=0.25), dm
    ms = L.random_swarm(n, world=(-side, -side, 0, side, side, 2.5), seed=seed, min_sep=0.31, shrink=0.15)
    if fam == "planar":
        ms.start[:, 2] = ms.goal[:, 2] = 1.0
    if fam == "m4":
        rng = np.random.default_rng(seed)
        ms.radius[:] = rng.uniform(0.1, 0.25, n)
        ms.downwash[:] = rng.uniform(1.0, 2.5, n)
        ms.max_vel[:] = rng.uniform(0.6, 1.5, (n, 1))
        ms.max_acc[:] = rng.uniform(1.0, 3.0, (n, 1))
    return ms, None


def _record(out, fam, i, ms, prm, hist, kept, agents=None):
    """Verdicts of the kept ticks of one flown mission into `out`; prints the counts."""
    from oracle import oracle as O
    key = f"{fam}{i}_"
    for name in PV.MISSION_KEYS:
        out[key + name] = getattr(ms, name)
    out[key + "kept"] = np.asarray(kept, np.int32)
    if fam == "corridor":                       # every tick: inputs, the oracle's boxes and statuses
        out[key + "states"] = np.array([h[0] for h in hist])
        out[key + "trajs"] = np.array([h[1] for h in hist])
        out[key + "sfc"] = np.array([h[2]["sfc"] for h in hist])
        out[key + "ostatus"] = np.array([h[2]["status"] for h in hist], np.int32)
    else:
        out[key + "states"] = np.array([hist[t - 1][0] for t in kept])
        out[key + "trajs"] = np.array([hist[t - 1][1] for t in kept])
    V, C, X, OK, J = [], [], [], [], []
    for tick in kept:
        state, traj, o = hist[tick - 1]
        ag = None if agents is None else agents(o)
        v, c, x, ok = PV.tick_verdicts(O, H, fam, prm, ms, state, traj, tick, o, agents=ag)
        judged = o["status"] != 4
        if ag is not None:
            judged &= np.isin(np.arange(ms.qn), ag)
        V.append(v); C.append(c); X.append(x); OK.append(ok); J.append(judged)
        opt = (v == 0) | (v == 2)
        agree = bool(((v < 0) | (np.minimum(v, 1) == o["status"]) | (v == 2)).all())
        print(f"{fam} mission {i} (n {ms.qn}) tick {tick}: infeasible {int((v == 1).sum())} optimal {int((v == 0).sum())} upper bounds {int((v == 2).sum())}"
              f" none {int(((v < 0) & judged).sum())} blocked {int((o['status'] == 4).sum())} x far {int((opt & ~ok).sum())}  oracle agrees {agree}", flush=True)
    out[key + "verdict"], out[key + "cost"], out[key + "x"] = np.array(V), np.array(C), np.array(X)
    out[key + "xok"], out[key + "judged"] = np.array(OK), np.array(J)
    out[key + "ostatus_kept"] = np.array([hist[t - 1][2]["status"] for t in kept], np.int32)


def _first_infeasible_ticks(hist):
    """Ticks on which some agent is infeasible that was not on the tick before."""
    ticks, before = [], np.zeros(len(hist[0][0]), bool)
    for t, (_, _, o) in enumerate(hist, 1):
        now = o["status"] == 1
        if (now & ~before).any():
            ticks.append(t)
        before = now
    return ticks


def make(fam, out):
    from oracle import oracle as O
    M = PV.family_params(fam)[0]
    with O.segments(M):
        if fam == "corridor":
            for i, (n, side, seed, T, keep) in enumerate(CORRIDOR):
                ms, dm = _swarm(fam, n, side, seed)
                prm, hist = PV.fly(O, fam, ms, T, dm)
                kept = sorted(set(keep) | set(_first_infeasible_ticks(hist)))
                _record(out, fam, i, ms, prm, hist, kept)
            out[fam + "_count"] = np.int32(len(CORRIDOR))
        elif fam in ("planar", "m4"):
            specs = PLANAR if fam == "planar" else M4
            for i, (n, side, seed) in enumerate(specs):
                ms, _ = _swarm(fam, n, side, seed)
                prm, hist = PV.fly(O, fam, ms, 14)
                first = [t for t, (_, _, o) in enumerate(hist, 1) if (o["status"] == 1).any()][:1]
                _record(out, fam, i, ms, prm, hist, sorted(set(first) | {8, 14}))
            out[fam + "_count"] = np.int32(len(specs))
        else:
            import lsc_planner_amd as L
            ms = L.random_swarm(TP["n"], world=TP["world"], seed=TP["seed"])
            prm, hist = PV.fly(O, fam, ms, TP["tick"])
            subset = np.random.default_rng(TP["subset_seed"]).choice(TP["n"], TP["subset"], replace=False)
            _record(out, fam, 0, ms, prm, hist, [TP["tick"]], agents=lambda o: sorted(set(subset.tolist()) | set(np.flatnonzero(o["status"] == 1).tolist())))
            out[fam + "_count"] = np.int32(1)


def main(families):
    files = {}
    for fam in families:
        files.setdefault(PV.FILES[fam], []).append(fam)
    for fname, fams in files.items():
        if set(fams) != {f for f, n in PV.FILES.items() if n == fname}:
            raise SystemExit(f"{fname} holds {sorted(f for f, n in PV.FILES.items() if n == fname)}: make them together")
        out = {}
        for fam in fams:
            make(fam, out)
        out["solver"] = np.array("HiGHS " + H.version() + " (scipy.optimize._highspy)")
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **out)
        Z = np.load(path)
        for fam in fams:
            print(f"{fam}: (certified infeasible, optimal, no verdict, optimal with x far, blocked) = {PV.counts(Z, fam)}")
        print(f"{fname}: {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or ["corridor", "planar", "m4", "tp"])
