"""-m gpu: the kernel against the INDEPENDENT solver on the QP variants, no oracle in between.

tests/golden/make_qp_pin_variants.py recorded, for four families of QPs the 90-variable empty-map pins of tests/test_gpu_round3.py never reach
(tests/pin_variants.py: corridor QPs on the forest map, the planar 60-variable QP, the four-segment 72-variable QP, one tick of the 320-agent
swarm the throughput build plans), the inputs of the ticks and what HiGHS says about every agent's QP.  The same inputs through the C ABI:
status 1 exactly where HiGHS certifies infeasibility, status 0 and HiGHS's cost elsewhere, and -- where HiGHS's point and the oracle's plan
agree to half the plan tolerance (x_ok) -- HiGHS's plan.  Every family goes through every way an agent's QP gets solved, and each case
proves that its way was the one taken:

    active_set      the default: the dual active-set solve (the interior point takes what it hands over)
    interior_point  the interior point alone
    hand_over       the active-set solve runs, then every agent is handed to the interior point (test mode of the library)
    second_pass     max_rows_per_cp = 1: agents with more rows than the LDS pass holds are planned with their rows in HBM (lsc_plan_spill_kernel)
    tp              more agents than the GPU has CUs: the 256-lane throughput build
    m4              liblsc_hip_m4.so

The obs family (tests/golden/make_qp_pin_obstacles.py: crossing spheres, chasers and a walker in pursuit, a crowd of 54 spheres, and the
crossing once more with half-second segments) holds the plan kernels of a context with dynamic obstacles -- lsc_plan_obs_kernel<0>, <1> and
lsc_plan_spill_obs_kernel -- to the same verdicts: every recorded tick is replayed in order on one context per path, because an infeasible
agent keeps the last plan it solved.

Plan tolerances (tests/tolerances.py): TRAJ_ATOL for the active-set path (under its LSC_SOLVER-proof name), the interior point's 1e-4 m
wherever the interior point is sent agents on purpose, FUZZ_TRAJ_ATOL_HALF_SECOND with half-second segments.
"""
import numpy as np
import pytest

import pin_variants as PV
from tolerances import ACTIVE_SET_TRAJ_ATOL, COST_ATOL, COST_RTOL, FUZZ_TRAJ_ATOL_HALF_SECOND, INTERIOR_POINT_TRAJ_ATOL

pytestmark = pytest.mark.gpu

PATHS = {"active_set": dict(solver="active_set"), "interior_point": dict(solver="interior_point"), "hand_over": dict(solver="hand_over"),
         "second_pass": dict(solver="active_set", max_rows_per_cp=1)}


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


@pytest.fixture(scope="module")
def forest_bt(tmp_path_factory):
    from maputil import forest_leaves, write_bt
    path = str(tmp_path_factory.mktemp("map") / "forest.bt")
    write_bt(path, *forest_leaves())
    return path


def _traj_atol(fam, path):
    if fam in ("m4", "obs_m4"):
        return FUZZ_TRAJ_ATOL_HALF_SECOND
    return ACTIVE_SET_TRAJ_ATOL if path == "active_set" else INTERIOR_POINT_TRAJ_ATOL


class _Tally:
    """What a replay saw, for the proof that its path was taken and for the counts."""

    def __init__(self):
        self.n_inf = self.n_opt = self.replans = self.solved = self.handed = self.spilled = 0
        self.worst_cost = self.worst_plan = 0.0

    def planner(self, L, ms, fam, path, extra=None):
        pl = L.SwarmPlanner(ms, L.PlannerConfig(**PV.family_params(fam)[3], **PATHS[path], **(extra or {})))
        pl.iterations_total(reset=True)
        return pl

    def after_tick(self, pl, r, kept):
        self.replans += int(np.isin(r["status"], (0, 1)).sum())           # agents whose QP was solved: neither a blocked seed nor an error
        if kept and pl.cfg.max_rows_per_cp:
            # the LDS pass leaves an agent to the pass with its rows in HBM when the agent has more rows than lsc_row_capacity says
            # (its fullest control-point bucket then holds more than max_rows_per_cp of them)
            over = pl.row_counts() > pl.row_capacity()[0]
            assert (pl.bucket_max()[over] > pl.cfg.max_rows_per_cp).all()
            self.spilled += int(over.sum())

    def done(self, pl):
        st = pl.solver_stats()
        self.solved += st["solved"]; self.handed += st["handed_over"]
        pl.close()

    def check(self, Z, fam, i, k, tick, r, atol):
        """One kept tick's results against the file."""
        key = f"{fam}{i}_"
        v, c, x, x_ok, ost = Z[key + "verdict"][k], Z[key + "cost"][k], Z[key + "x"][k], Z[key + "xok"][k], Z[key + "ostatus_kept"][k]
        where = (fam, i, tick)
        blocked = ost == 4                                          # no QP, no verdict: the status itself is the recorded one
        assert np.array_equal(r["status"] == 4, blocked), (where, r["status"], ost)
        known = v >= 0
        assert np.array_equal(r["status"][known], (v[known] == 1).astype(np.int32)), (where, r["status"], v)
        opt = v == 0
        err = np.abs(r["cost"][opt] - c[opt]) / (COST_RTOL * np.abs(c[opt]) + COST_ATOL)
        ub = v == 2                                                 # HiGHS stopped short: its cost is an upper bound (a few 1e-6 relative)
        far = np.abs(r["traj"][:, :x.shape[1]].astype(np.float64) - x).reshape(len(v), -1).max(1)[opt & x_ok | ub & x_ok]
        self.worst_cost = max(self.worst_cost, float(err.max()) if err.size else 0.0)
        self.worst_plan = max(self.worst_plan, float(far.max()) if far.size else 0.0)
        print(f"{where}: cost error / bound {err.max() if err.size else 0.0:.3g}, plan {far.max() if far.size else 0.0:.3g} m (bound {atol:g})")
        assert (err <= 1.0).all(), ("cost", where, r["cost"][opt], c[opt])
        assert (r["cost"][ub] <= c[ub] + COST_ATOL).all() and (r["cost"][ub] >= c[ub] * (1 - 1e-5) - COST_ATOL).all(), (where, r["cost"][ub], c[ub])
        assert (far <= atol).all(), ("plan", where, far)
        self.n_inf += int((v == 1).sum()); self.n_opt += int(opt.sum() + ub.sum())


def replay(L, fam, path, bt, extra=None):
    """Every mission of a family through one path (bt: the forest map as an octomap file); returns the tally."""
    Z = PV.load(fam)
    T = _Tally()
    atol = _traj_atol(fam, path)
    for i in range(PV.missions_of(Z, fam)):
        ms = PV.mission(Z, fam, i)
        kept = PV.kept_ticks(Z, fam, i)
        key = f"{fam}{i}_"
        if fam == "corridor":
            # one context over every recorded tick: the boxes have a history
            pl = T.planner(L, ms, fam, path, extra)
            pl.load_octomap(bt)                     # (the library's own reader and distance transform: tests/test_oracle_pin_variants.py holds them to the oracle's on these worlds)
            at = {tick: k for k, tick in kept}
            for tick in range(1, len(Z[key + "states"]) + 1):
                state, traj = PV.tick_inputs(Z, fam, i, None, tick)
                r = pl.plan(state, ms.goal, traj)
                assert np.array_equal(r["sfc"], Z[key + "sfc"][tick - 1]), (i, tick)
                assert np.array_equal(r["status"] == 4, Z[key + "ostatus"][tick - 1] == 4), (i, tick)
                T.after_tick(pl, r, tick in at)
                if tick in at:
                    T.check(Z, fam, i, at[tick], tick, r, atol)
            T.done(pl)
        else:
            for k, tick in kept:
                state, traj = PV.tick_inputs(Z, fam, i, k, tick)
                pl = T.planner(L, ms, fam, path, extra)
                if fam == "m4":
                    assert pl.M == 4 and pl.L.lsc_segments() == 4
                if fam == "tp":
                    lds, thr = pl.row_capacity()
                    assert 0 < thr < lds                            # default capacities: this shard takes the throughput build
                pl.planner_seq = tick - 1                           # plan() advances it: the tick's own planner_seq
                r = pl.plan(state, ms.goal, traj)
                T.after_tick(pl, r, True)
                T.check(Z, fam, i, k, tick, r, atol)
                T.done(pl)
    return T


# (tp: the throughput build has two instantiations of its own, one per solver)
CASES = [(fam, path) for fam in ("corridor", "planar", "m4") for path in PATHS] + [("tp", "active_set"), ("tp", "interior_point")]


@pytest.mark.parametrize("fam,path", CASES)
def test_kernel_against_highs_verdicts(L, forest_bt, fam, path):
    T = replay(L, fam, path, forest_bt)
    print(f"{fam} / {path}: worst cost error / bound {T.worst_cost:.3g}, worst plan distance {T.worst_plan:.3g} m")
    assert (T.n_inf, T.n_opt) == PV.COUNTS[fam][:2]
    if path == "active_set":
        assert T.solved > 0, vars(T)
    elif path == "hand_over":
        assert T.solved == 0 and T.handed == T.replans > 0, vars(T)
    elif path == "second_pass":
        assert T.spilled > 0, vars(T)


def test_an_interior_point_that_stops_early_fails_the_pins(L, forest_bt, capsys):
    """The tolerances bind: gap_tolerance = 1e-5 is a supported setting that lets the interior point stop at a relative duality gap of 1e-5
    instead of 1e-9.  Its verdicts stay right and its boxes are the same, but its costs or plans are no longer HiGHS's: the corridor replay
    fails in the cost or the plan assertion -- and nowhere earlier."""
    with pytest.raises(AssertionError, match=r"^\('(cost|plan)'"):
        replay(L, "corridor", "interior_point", forest_bt, extra=dict(gap_tolerance=1e-5))
    print(capsys.readouterr().out[-400:])


# ------------------------------------------------------------------------------------------------ the obs family: dynamic obstacles
# (second_pass as tests/test_gpu_obstacles.py::test_second_pass_with_rows_in_hbm: one row per control point in LDS and no pruning)
OBS_PATHS = dict(PATHS, second_pass=dict(solver="active_set", max_rows_per_cp=1, prune=False))


def replay_obs(L, fam, path, extra=None):
    """Every mission of an obs family through one path: every recorded tick in order on ONE context, the obstacles' recorded states
    host-fed.  Returns the tally; T.peak13 says whether an active-set solve asked for a thirteenth row, T.notes holds the contexts' notes."""
    Z = PV.load(fam)
    T = _Tally()
    T.peak13, T.notes = False, {}
    atol = _traj_atol(fam, path)
    for i, name in enumerate(PV.OBS_SCENES[fam]):
        ms = PV.mission(Z, fam, i)
        key = f"{fam}{i}_"
        pl = L.SwarmPlanner(ms, L.PlannerConfig(**PV.family_params(fam)[3], **OBS_PATHS[path], **(extra or {})))
        pl.iterations_total(reset=True)
        if fam == "obs_m4":
            assert pl.M == 4 and pl.L.lsc_segments() == 4
        pl.set_obstacles(Z[key + "obs_radius"], Z[key + "obs_downwash"])
        T.notes[name] = pl.note()
        if path == "active_set":
            assert (pl.working_set_peaks() == 0).all()                 # (the first call switches the counter on)
        rows_at = {int(t): r for r, t in enumerate(Z[key + "rows_ticks"])}
        last_ok = np.zeros_like(Z[key + "trajs"][0])                    # a context's plans start at zero, as TrajOptimizer::trajectory does
        for k, tick in PV.kept_ticks(Z, fam, i):
            state, traj = PV.tick_inputs(Z, fam, i, k, tick)
            pv = Z[key + "obstacles"][k]
            pl.obstacle_states(pv[:, :3], pv[:, 3:])
            r = pl.plan(state, ms.goal, traj, want_constraints=tick in rows_at)
            T.after_tick(pl, r, True)
            T.check(Z, fam, i, k, tick, r, atol)
            # an infeasible agent keeps the last plan THIS context returned with status 0 for it, bit for bit
            bad = r["status"] == 1
            assert np.array_equal(r["traj"][bad], last_ok[bad]), ("stale", name, tick, np.flatnonzero(bad))
            last_ok[r["status"] == 0] = r["traj"][r["status"] == 0]
            if tick in rows_at:
                # the composed reference's rows, in the product's order: the other agents by index, then the obstacles
                assert np.array_equal(r["normal"], Z[key + "normal"][rows_at[tick]]), ("normal", name, tick)
                assert np.array_equal(r["d"], Z[key + "d"][rows_at[tick]]), ("d", name, tick)
            if path == "active_set":
                T.peak13 = T.peak13 or bool((pl.working_set_peaks() == 13).any())
        T.done(pl)
    return T


# (the four-segment mission goes through the active-set solve and the second pass)
OBS_CASES = [("obs", path) for path in OBS_PATHS] + [("obs_m4", "active_set"), ("obs_m4", "second_pass")]


@pytest.mark.parametrize("fam,path", OBS_CASES)
def test_obstacle_kernels_against_highs_verdicts(L, fam, path):
    Z = PV.load(fam)
    assert PV.counts(Z, fam) == PV.COUNTS[fam]
    got = PV.obs_conditions(Z)
    assert got == PV.OBS_COUNTS
    PV.assert_obs_conditions(got)
    T = replay_obs(L, fam, path)
    print(f"{fam} / {path}: certified infeasible {T.n_inf}, optimal {T.n_opt}, handed over {T.handed}, solved by the active set {T.solved}, spilled {T.spilled}, "
          f"worst cost error / bound {T.worst_cost:.3g}, worst plan distance {T.worst_plan:.3g} m")
    assert (T.n_inf, T.n_opt) == PV.COUNTS[fam][:2]
    if path == "active_set":
        assert T.solved > 0, vars(T)
        if fam == "obs":
            assert T.handed > 0 and T.peak13, vars(T)
    elif path == "hand_over":
        assert T.solved == 0 and T.handed == T.replans > 0, vars(T)
    elif path == "second_pass":
        assert T.spilled > 0, vars(T)
    if fam == "obs":
        # (lsc_set_obstacles' remark: the build goes by N - 1 + K; the "lsc build:" remark of lsc_set_agents speaks of the agents alone)
        assert "dynamic obstacles: K = 54, 65 per agent, generic pass (more than 64 obstacles)" in T.notes["crowd"], T.notes
        assert "dynamic obstacles: K = 3, 10 per agent, one wave per segment" in T.notes["crossing"], T.notes
        assert "dynamic obstacles: K = 4, 11 per agent, one wave per segment" in T.notes["pursuit"], T.notes
