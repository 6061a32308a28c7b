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

The modes family (tests/golden/make_qp_pin_modes.py: BVC, BVC with two constrained segments, BVC with either slack mode, the disturbance
reset in LSC mode with gusts, a 64-agent crowd, a planar world, and a slack mode and the reset with half-second segments) holds the OTHER QP
solver of the library -- the dense interior point of csrc/lsc_general.hpp -- to the same verdicts, through every way it is reached:
folded into the plan kernel, a launch of lsc_general_kernel, lsc_general_batch_kernel, both builds of general_agent (every row array in LDS /
the last ones in HBM), the warm start alone and the cold start behind a failed warm attempt, and the M = 4 library.

Plan tolerances (tests/tolerances.py): TRAJ_ATOL for the active-set path (under its LSC_SOLVER-proof name), the interior point's 1e-4 m
wherever the interior point is sent agents on purpose, FUZZ_TRAJ_ATOL_HALF_SECOND with half-second segments.
"""
import os
import subprocess
import sys

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
    if fam in ("m4", "obs_m4", "modes_m4"):
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


# ------------------------------------------------------------------------------------------------ the modes family: the alternate planner modes
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDOVER_ENV = "LSC_GENERAL_HANDOVER"
FOLDED, LAUNCHED, BATCHED = 1, 2, 3                  # lsc_general_info's last_launch


def _modes_context(L, fam, name, monkeypatch, hold=False):
    """(mission, context) of a scene; hold: created with LSC_GENERAL_HANDOVER set, i.e. held to the two-launch hand-over."""
    from harness import held_planner
    Z = PV.load(fam)
    ms = PV.mission(Z, fam, PV.MODES_SCENES[fam].index(name))
    pl = held_planner(L, ms, lambda: L.PlannerConfig(**PV.modes_scene_params(fam, name)[3], solver="active_set"), monkeypatch, HANDOVER_ENV, hold)
    pl.iterations_total(reset=True)
    if fam == "modes_m4":
        assert pl.M == 4 and pl.L.lsc_segments() == 4
    return ms, pl


class _ModesTally(_Tally):
    """... and the stale-plan rule, the recorded rows and the path proofs of a modes replay."""

    def __init__(self):
        super().__init__()
        self.launches = {}                              # scene: the set of lsc_general_info's last_launch over its ticks
        self.lds = self.generic = 0                     # agent-ticks solved by general_agent<true> / <false> (from the kept obstacles)
        self.warm_alone = self.cold_after_warm = self.cold_first = 0
        self.last_ok = {}

    def first_plans(self, Z, fam, i, name):
        last = np.zeros_like(Z[f"{fam}{i}_trajs"][0])         # a context's plans start at zero, as TrajOptimizer::trajectory does
        if PV.modes_scene_params(fam, name)[5]:
            last[:, 2] = np.float32(1.0)                # (in the plane, world_z_2d, in a planar world: lsc_set_agents)
        self.last_ok[name] = last

    def after_modes_tick(self, Z, fam, i, name, k, tick, r, rows_at=None):
        self.check(Z, fam, i, k, tick, r, _traj_atol(fam, "modes"))
        key = f"{fam}{i}_"
        # an infeasible agent keeps the last plan THIS context returned with status 0 for it, bit for bit
        bad, last = r["status"] == 1, self.last_ok[name]
        assert np.array_equal(r["traj"][bad], last[bad]), ("stale", name, tick, np.flatnonzero(bad))
        last[r["status"] == 0] = r["traj"][r["status"] == 0]
        if rows_at and tick in rows_at:
            assert np.array_equal(r["normal"], Z[key + "normal"][rows_at[tick]]), ("normal", name, tick)
            assert np.array_equal(r["d"], Z[key + "d"][rows_at[tick]]), ("d", name, tick)

    def builds(self, pl, general):
        """Which build of general_agent solved the agents of the last tick (`general`: the solver planned them): an agent's row count
        (collision rows and group sign rows: at most 27 + M per kept obstacle) bounds its kept obstacles from below, N - 1 from above."""
        if not general:
            return
        bound = pl.general_info()[0]
        rows = pl.row_counts()
        per = 6 * pl.M - 3 + pl.M                       # (every control point but the first three carries a row, every segment a sign row)
        kept_least = -(-rows // per)
        assert (kept_least <= pl.N - 1).all(), (rows, pl.N)
        if pl.N - 1 <= bound:
            self.lds += pl.N                            # (whatever the agents keep)
        else:
            self.generic += int((kept_least > bound).sum())


def _flagged(Z, fam, i, k):
    """Whether the general solver plans the scene's agents on kept tick k: always in BVC, from the first disturbance on under the reset."""
    name = PV.MODES_SCENES[fam][i]
    return "reset_threshold" not in PV.MODES_PARAMS[name]["cfg"] or bool(Z[f"{fam}{i}_slack_set"][k].any())


def replay_modes(L, fam, names, monkeypatch, hold=False, profile=False):
    """The named scenes of a modes family, each on ONE context over every recorded tick in order.  Returns the tally."""
    Z = PV.load(fam)
    T = _ModesTally()
    for name in names:
        i = PV.MODES_SCENES[fam].index(name)
        key = f"{fam}{i}_"
        ms, pl = _modes_context(L, fam, name, monkeypatch, hold)
        if profile:
            pl.phase_profile(1)
        T.first_plans(Z, fam, i, name)
        T.launches[name] = set()
        rows_at = {} if profile else {int(t): r for r, t in enumerate(Z[key + "rows_ticks"])}
        seen = np.zeros((pl.N, 16), np.int64)
        for k, tick in PV.kept_ticks(Z, fam, i):
            state, traj = PV.tick_inputs(Z, fam, i, k, tick)
            r = pl.plan(state, ms.goal, traj, want_constraints=tick in rows_at)
            T.after_tick(pl, r, True)
            T.after_modes_tick(Z, fam, i, name, k, tick, r, rows_at)
            general = _flagged(Z, fam, i, k)
            T.launches[name].add((general, pl.general_info()[1]))
            T.builds(pl, general)
            if profile:
                # columns 13 and 15 of lsc_general_profile: the agent's solves and its cold starts
                now = pl.general_profile()
                solves, cold = (now - seen)[:, 13], (now - seen)[:, 15]
                seen = now
                assert (solves == (1 if general else 0)).all() and (cold <= solves).all(), (name, tick, solves, cold)
                if tick >= 2:                       # (the warm start is tried from the second tick on)
                    T.warm_alone += int(((solves == 1) & (cold == 0)).sum())
                    T.cold_after_warm += int((cold == 1).sum())
                else:
                    T.cold_first += int((cold == 1).sum())
        T.done(pl)
    return T


SMALL = {"modes": ("bvc", "bvc_ncs2", "collision", "dynlimit", "reset", "planar"), "modes_m4": ("m4_collision", "m4_reset")}
RESETS = {"modes": ("reset",), "modes_m4": ("m4_reset",)}


def _assert_modes_fixture():
    Z = PV.load("modes")
    for fam in PV.MODES_FAMILIES:
        assert PV.counts(Z, fam) == PV.COUNTS[fam]
    got = PV.modes_conditions(Z)
    assert got == PV.MODES_COUNTS
    PV.assert_modes_conditions(got)


def _scene_counts(fam, names):
    got = PV.MODES_COUNTS
    return sum(got[n][1] for n in names), sum(got[n][2] for n in names)


@pytest.mark.parametrize("fam", PV.MODES_FAMILIES)
def test_general_solver_against_highs_verdicts(L, monkeypatch, fam):
    """Every small scene on a default context: BVC and the slack modes send every agent to a launch of lsc_general_kernel; the reset's
    context folds the hand-over into the plan kernel, on every tick."""
    _assert_modes_fixture()
    T = replay_modes(L, fam, SMALL[fam], monkeypatch)
    print(f"{fam} / default: certified infeasible {T.n_inf}, optimal {T.n_opt}, worst cost error / bound {T.worst_cost:.3g}, worst plan distance {T.worst_plan:.3g} m")
    assert (T.n_inf, T.n_opt) == _scene_counts(fam, SMALL[fam])
    for name in SMALL[fam]:
        want = {(False, FOLDED), (True, FOLDED)} if name in RESETS[fam] else {(True, LAUNCHED)}
        assert T.launches[name] == want, (name, T.launches)
    assert T.lds > 0 and T.generic == 0, vars(T)               # swarms of 8: every row array in LDS


@pytest.mark.parametrize("fam", PV.MODES_FAMILIES)
def test_general_solver_behind_the_plan_kernel_against_highs_verdicts(L, monkeypatch, fam):
    """The reset's scene on a context held to the two-launch hand-over: lsc_general_kernel on the flagged ticks, no launch on the others."""
    T = replay_modes(L, fam, RESETS[fam], monkeypatch, hold=True)
    print(f"{fam} / two launches: certified infeasible {T.n_inf}, optimal {T.n_opt}, worst cost error / bound {T.worst_cost:.3g}, worst plan distance {T.worst_plan:.3g} m")
    assert (T.n_inf, T.n_opt) == _scene_counts(fam, RESETS[fam])
    assert T.launches[RESETS[fam][0]] == {(False, 0), (True, LAUNCHED)}, T.launches


@pytest.mark.parametrize("fam", PV.MODES_FAMILIES)
def test_general_batch_kernel_against_highs_verdicts(L, monkeypatch, fam):
    """The family's small 3-D scenes as one mission list through replan_tick_batch (lsc_general_batch_kernel behind the batched plan
    launch): every mission's verdicts.  A scene that has run out of ticks leaves the list."""
    from lsc_planner_amd.planner import replan_tick_batch
    Z = PV.load(fam)
    names = [n for n in SMALL[fam] if not PV.modes_scene_params(fam, n)[5]]       # (one planar class per launch: the planar scene stays out)
    T = _ModesTally()
    ctx = {}
    for name in names:
        ctx[name] = _modes_context(L, fam, name, monkeypatch)
        T.first_plans(Z, fam, PV.MODES_SCENES[fam].index(name), name)
        T.launches[name] = set()
    for tick in range(1, max(PV.MODES_PARAMS[n]["ticks"] for n in names) + 1):
        live = [n for n in names if tick <= PV.MODES_PARAMS[n]["ticks"]]
        idx = [PV.MODES_SCENES[fam].index(n) for n in live]
        ins = [PV.tick_inputs(Z, fam, i, tick - 1, tick) for i in idx]
        outs = replan_tick_batch([ctx[n][1] for n in live], [s for s, _ in ins], [ctx[n][0].goal for n in live], [t for _, t in ins], [tick] * len(live))
        anyone = any(_flagged(Z, fam, i, tick - 1) for i in idx)
        for n, i, (traj, cost, status, iters) in zip(live, idx, outs):
            pl = ctx[n][1]
            r = dict(traj=traj, cost=cost, status=status, iters=iters)
            T.after_tick(pl, r, True)
            T.after_modes_tick(Z, fam, i, n, tick - 1, tick, r)
            T.launches[n].add(pl.general_info()[1])
            assert pl.general_info()[1] == (BATCHED if anyone else 0), (n, tick)
    for n in names:
        T.done(ctx[n][1])
    print(f"{fam} / batch: certified infeasible {T.n_inf}, optimal {T.n_opt}, worst cost error / bound {T.worst_cost:.3g}, worst plan distance {T.worst_plan:.3g} m")
    assert (T.n_inf, T.n_opt) == _scene_counts(fam, names)
    assert all(BATCHED in T.launches[n] for n in names), T.launches


def test_generic_pointer_build_against_highs_verdicts(L, monkeypatch):
    """The 64-agent crowd under DYNAMICALLIMIT's slack: no row pruning, all 63 obstacles kept -- more than the 50 whose row arrays fit in
    LDS behind the solver's state at M = 5 --, so every agent is solved by general_agent<false>, its last arrays in the HBM workspace."""
    T = replay_modes(L, "modes", ("crowd",), monkeypatch)
    print(f"modes / crowd: certified infeasible {T.n_inf}, optimal {T.n_opt}, worst cost error / bound {T.worst_cost:.3g}, worst plan distance {T.worst_plan:.3g} m")
    assert (T.n_inf, T.n_opt) == _scene_counts("modes", ("crowd",))
    assert T.launches["crowd"] == {(True, LAUNCHED)}
    assert T.generic == 64 * PV.MODES_PARAMS["crowd"]["ticks"] and T.lds == 0, vars(T)


def test_lds_bound_of_the_general_solver(L):
    """lsc_general_info's bound: a swarm of up to 51 agents has every agent's row arrays in LDS whatever it keeps; from 52 agents on the
    bound is 50 kept obstacles (M = 5: the take sizes of general_agent against the 160 KB of LDS less the solver's state)."""
    for n, want in ((8, 7), (51, 50), (52, 50), (64, 50)):
        ms = L.circle_swap(n, 3.0, world=(-5, -5, 0, 5, 5, 2.5))
        pl = L.SwarmPlanner(ms, L.PlannerConfig(planner_mode="bvc"))
        assert pl.general_info() == (want, 0), (n, pl.general_info())
        pl.close()


def test_warm_and_cold_starts_of_the_general_solver(L, monkeypatch):
    """Columns 13 and 15 of lsc_general_profile (the instrumented kernels): over the M = 5 scenes the warm attempt decides agent-ticks on
    its own, and the cold start runs behind a failed warm attempt -- the verdicts hold on this path too.  (On the MI355X: 303 agent-ticks
    decided by the warm attempt, 81 by the cold start behind it, 32 cold starts on tick 1.)"""
    T = replay_modes(L, "modes", ("bvc", "bvc_ncs2", "collision", "dynlimit", "reset"), monkeypatch, profile=True)
    print(f"modes / profiled: warm start alone {T.warm_alone}, cold start behind a failed warm attempt {T.cold_after_warm}, cold start on the first tick {T.cold_first}, "
          f"worst cost error / bound {T.worst_cost:.3g}, worst plan distance {T.worst_plan:.3g} m")
    assert T.warm_alone > 0 and T.cold_first > 0, vars(T)
    assert T.cold_after_warm > 0, vars(T)


def test_modes_through_the_lds_poison_libraries():
    """The modes cases once more through the libraries whose kernels start with their LDS full of 0xff bytes."""
    lib = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_poison.so")
    lib4 = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_m4_poison.so")
    assert os.path.exists(lib) and os.path.exists(lib4), "the poison libraries are not built (make -C lsc_planner_amd/csrc poison poison_m4)"
    env = dict(os.environ, LSC_HIP_LIB=lib, LSC_HIP_LIB_M4=lib4)
    env.pop(HANDOVER_ENV, None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "general_solver or general_batch or generic_pointer"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
