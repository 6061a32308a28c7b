"""The HiGHS pins of the QP variants (tests/pin_variants.py: corridor, planar, four-segment and throughput-swarm QPs), oracle side.

tests/golden/make_qp_pin_variants.py recorded, per agent of the kept ticks, what HiGHS says about the agent's QP.  Here
  * the recorded counts are the ones the generator printed and meet the conditions the fixtures were made for;
  * the oracle on the recorded inputs gives status 1 exactly where the file certifies infeasibility and the recorded cost elsewhere -- to
    the bound of tests/test_oracle_pins.py --, and in the corridor family its boxes are the recorded ones bit for bit on every tick;
  * with HiGHS importable, the verdicts of one mission per family are derived again.
The obs family (dynamic obstacles; tests/golden/make_qp_pin_obstacles.py) has its own tests at the end: the composed reference of
tests/obstacle_reference.py stands where the oracle's Swarm stands for the others, and ObstacleSet gives back the recorded obstacle states.
The modes family (the alternate planner modes; tests/golden/make_qp_pin_modes.py) follows them: the oracle of the alternate modes
(O.SwarmEx) over every recorded tick in order, and a stated sample of its QPs through HiGHS once more.
The kernel replays the same files in tests/test_gpu_highs_variants.py.
"""
import os

import numpy as np
import pytest

import highs_qp as H
import pin_variants as PV
from test_oracle_pins import COST_ATOL, COST_RTOL

FAMILIES = ("corridor", "planar", "m4", "tp")


@pytest.mark.parametrize("fam", FAMILIES)
def test_recorded_counts_are_the_generator_s_and_meet_the_conditions(fam):
    Z = PV.load(fam)
    n_inf, n_opt, n_none, n_far, n_blocked = got = PV.counts(Z, fam)
    print(fam, got)
    assert got == PV.COUNTS[fam]
    if fam != "tp":
        assert n_inf >= 10 and n_opt >= 60
    assert n_none <= 0.10 * (n_inf + n_opt + n_none)
    assert n_far <= 0.05 * n_opt
    for i in range(PV.missions_of(Z, fam)):
        # a blocked seed (status 4) has no QP and no verdict
        assert (Z[f"{fam}{i}_verdict"][Z[f"{fam}{i}_ostatus_kept"] == 4] == -1).all()


def _replay(O, Z, fam, i):
    """The oracle over the recorded inputs of mission i: [(kept index, tick, state, previous plans, result)] of the kept ticks."""
    ms = PV.mission(Z, fam, i)
    dm = PV.forest_distmap(O, ms.world_min, ms.world_max)[0] if fam == "corridor" else None
    prm, sw = PV.oracle_swarm(O, fam, ms, dm)
    kept = PV.kept_ticks(Z, fam, i)
    out = []
    if fam == "corridor":
        # one swarm over every tick: the boxes of a tick grow out of the boxes of the tick before
        at = {tick: k for k, tick in kept}
        for tick in range(1, len(Z[f"{fam}{i}_states"]) + 1):
            state, traj = PV.tick_inputs(Z, fam, i, None, tick)
            o = sw.tick(state, ms.goal, traj, tick, want_lsc=True, nthreads=8)
            assert np.array_equal(o["sfc"], Z[f"{fam}{i}_sfc"][tick - 1]), (i, tick)
            assert np.array_equal(o["status"], Z[f"{fam}{i}_ostatus"][tick - 1]), (i, tick)
            if tick in at:
                out.append((at[tick], tick, state, traj, o))
    else:
        for k, tick in kept:
            state, traj = PV.tick_inputs(Z, fam, i, k, tick)
            out.append((k, tick, state, traj, sw.tick(state, ms.goal, traj, tick, want_lsc=True, nthreads=8)))
    return ms, prm, out


@pytest.mark.parametrize("fam", FAMILIES)
def test_oracle_on_the_recorded_inputs_vs_the_recorded_verdicts(oracle, fam):
    O = oracle
    Z = PV.load(fam)
    n_inf = n_opt = 0
    with O.segments(PV.family_params(fam)[0]):
        for i in range(PV.missions_of(Z, fam)):
            ms, prm, ticks = _replay(O, Z, fam, i)
            for k, tick, state, traj, o in ticks:
                v, c = Z[f"{fam}{i}_verdict"][k], Z[f"{fam}{i}_cost"][k]
                assert np.array_equal(o["status"], Z[f"{fam}{i}_ostatus_kept"][k]), (i, tick)
                known = v >= 0
                assert np.array_equal(o["status"][known], (v[known] == 1).astype(np.int32)), (i, tick, o["status"], v)
                opt = v == 0
                assert (np.abs(o["cost"][opt] - c[opt]) <= COST_RTOL * np.abs(c[opt]) + COST_ATOL).all(), (i, tick)
                ub = v == 2             # HiGHS stopped short: its cost is an upper bound (a few 1e-6 relative), as in tests/test_gpu_round3.py
                assert (o["cost"][ub] <= c[ub] + COST_ATOL).all() and (o["cost"][ub] >= c[ub] * (1 - 1e-5) - COST_ATOL).all(), (i, tick)
                n_inf += int((v == 1).sum()); n_opt += int(opt.sum() + ub.sum())
    assert (n_inf, n_opt) == PV.COUNTS[fam][:2]


@pytest.mark.skipif(not H.available(), reason="scipy's bundled HiGHS is not importable")
@pytest.mark.parametrize("fam,i", [("corridor", 0), ("planar", 0), ("m4", 2), ("tp", 0)])
def test_verdicts_derived_again_with_highs(oracle, fam, i):
    """One mission per family through HiGHS once more: the verdicts, costs, points and x_ok flags of the file.  (tp: a QP of the 320-agent
    swarm has 8 600 rows and takes HiGHS most of a second; eight of the recorded agents are derived again.)"""
    O = oracle
    Z = PV.load(fam)
    with O.segments(PV.family_params(fam)[0]):
        ms, prm, ticks = _replay(O, Z, fam, i)
        for k, tick, state, traj, o in ticks:
            ag = np.flatnonzero(Z[f"{fam}{i}_judged"][k])
            if fam == "tp":
                ag = ag[::5]
                assert len(ag) == 8
            v, c, x, ok = PV.tick_verdicts(O, H, fam, prm, ms, state, traj, tick, o, agents=ag)
            assert np.array_equal(v[ag], Z[f"{fam}{i}_verdict"][k][ag]), (tick, v, Z[f"{fam}{i}_verdict"][k])
            assert np.allclose(c[ag], Z[f"{fam}{i}_cost"][k][ag], rtol=1e-9, atol=1e-12), tick
            assert np.abs(x[ag] - Z[f"{fam}{i}_x"][k][ag]).max() <= 1e-6, tick
            assert np.array_equal(ok[ag], Z[f"{fam}{i}_xok"][k][ag]), tick


def test_the_library_s_distance_field_of_the_corridor_worlds_is_the_oracle_s(oracle, tmp_path):
    """The GPU replay hands the forest map to the library as an octomap file (no oracle there): its reader and distance transform -- host
    code -- give the oracle's field on the worlds of the corridor missions, bit for bit."""
    from lsc_planner_amd.planner import edt_from_bt
    from maputil import forest_leaves, write_bt
    bt = str(tmp_path / "forest.bt")
    leaves, res = forest_leaves()
    write_bt(bt, leaves, res)
    Z = PV.load("corridor")
    for i in range(PV.missions_of(Z, "corridor")):
        ms = PV.mission(Z, "corridor", i)
        dm, _ = PV.forest_distmap(oracle, ms.world_min, ms.world_max)
        dist, key_min, r = edt_from_bt(bt, ms.world_min, ms.world_max)
        assert r == res and np.array_equal(key_min, dm.key_min) and np.array_equal(dist, dm.dist), i


# ------------------------------------------------------------------------------------------------ the obs family: dynamic obstacles
OBS_MISSIONS = [(fam, i) for fam in PV.OBS_FAMILIES for i in range(len(PV.OBS_SCENES[fam]))]


def test_obs_recorded_counts_are_the_generator_s_and_meet_the_conditions():
    Z = PV.load("obs")
    for fam in PV.OBS_FAMILIES:
        assert PV.missions_of(Z, fam) == len(PV.OBS_SCENES[fam])
        assert PV.counts(Z, fam) == PV.COUNTS[fam], (fam, PV.counts(Z, fam))
        for i, name in enumerate(PV.OBS_SCENES[fam]):
            ms, obstacles, ticks = PV.obs_scene(name)
            n, K = ms.qn, len(obstacles)
            assert 8 <= n <= 12 and ticks <= 40 and Z[f"{fam}{i}_states"].shape == (ticks, n, 9) and Z[f"{fam}{i}_obstacles"].shape == (ticks, K, 6)
            assert Z[f"{fam}{i}_obstacles"].dtype == np.float32 and Z[f"{fam}{i}_judged"].all()          # every tick from 1, every agent judged
            assert (n - 1 + K > 64) == (name == "crowd")
            for k in PV.MISSION_KEYS:
                assert np.array_equal(Z[f"{fam}{i}_{k}"], getattr(ms, k)), (name, k)
    got = PV.obs_conditions(Z)
    print(got)
    assert got == PV.OBS_COUNTS
    PV.assert_obs_conditions(got)
    # the crowd's obstacles are close ones: every agent has an obstacle within a metre on the first tick
    crowd = PV.OBS_SCENES["obs"].index("crowd")
    gap = np.linalg.norm(Z[f"obs{crowd}_states"][0][:, None, :3] - Z[f"obs{crowd}_obstacles"][0][None, :, :3], axis=2)
    assert (gap.min(axis=1) < 1.0).all(), gap.min(axis=1)


def _obs_replay(O, Z, fam, i):
    """The composed reference over the recorded inputs of mission i, every tick in order on one swarm: [(tick, state, plans, result)]."""
    from obstacle_reference import ObstacleSwarm
    ms = PV.mission(Z, fam, i)
    key = f"{fam}{i}_"
    ref = ObstacleSwarm(O, ms, Z[key + "obs_radius"], Z[key + "obs_downwash"], dt=PV.family_params(fam)[1])
    out = []
    for k, tick in PV.kept_ticks(Z, fam, i):
        assert tick == k + 1
        state, traj = PV.tick_inputs(Z, fam, i, k, tick)
        pv = Z[key + "obstacles"][k]
        o = ref.tick(state, ms.goal, traj, tick, pv[:, :3], pv[:, 3:])
        o["obs"] = pv
        out.append((tick, state, traj, o))
    return ms, ref.prm, out


@pytest.mark.parametrize("fam,i", OBS_MISSIONS)
def test_composed_reference_on_the_recorded_inputs_vs_the_recorded_verdicts(oracle, fam, i):
    """tests/obstacle_reference.py's tick on the recorded inputs: status 1 exactly where HiGHS certifies infeasibility, HiGHS's cost
    elsewhere, HiGHS's plan where x_ok, the recorded rows bit for bit, and for an infeasible agent the last plan it solved."""
    from tolerances import ACTIVE_SET_TRAJ_ATOL
    O = oracle
    Z = PV.load(fam)
    key = f"{fam}{i}_"
    with O.segments(PV.family_params(fam)[0]):
        ms, prm, ticks = _obs_replay(O, Z, fam, i)
        rows_at = {int(t): r for r, t in enumerate(Z[key + "rows_ticks"])}
        last_ok = np.zeros_like(Z[key + "trajs"][0])
        for tick, state, traj, o in ticks:
            k = tick - 1
            v, c, x, x_ok = Z[key + "verdict"][k], Z[key + "cost"][k], Z[key + "x"][k], Z[key + "xok"][k]
            assert np.array_equal(o["status"], Z[key + "ostatus"][k]), (tick, o["status"])
            assert (v >= 0).all() and np.array_equal(o["status"], (v == 1).astype(np.int32)), (tick, o["status"], v)
            opt = v == 0
            assert (np.abs(o["cost"][opt] - c[opt]) <= COST_RTOL * np.abs(c[opt]) + COST_ATOL).all(), tick
            ub = v == 2
            assert (o["cost"][ub] <= c[ub] + COST_ATOL).all() and (o["cost"][ub] >= c[ub] * (1 - 1e-5) - COST_ATOL).all(), tick
            near = (opt | ub) & x_ok
            assert np.abs(o["traj"][near].astype(np.float64) - x[near]).max(initial=0.0) <= ACTIVE_SET_TRAJ_ATOL, tick
            bad = o["status"] == 1
            assert np.array_equal(o["traj"][bad], last_ok[bad]), tick
            last_ok[~bad] = o["traj"][~bad]
            if tick in rows_at:
                assert np.array_equal(o["normal"], Z[key + "normal"][rows_at[tick]]) and np.array_equal(o["d"], Z[key + "d"][rows_at[tick]]), tick
            if k + 1 < len(ticks):
                # the record is a closed loop: the next tick's previous plans are this tick's plans
                assert np.array_equal(Z[key + "trajs"][k + 1], o["traj"]), tick
        assert len(rows_at) >= 3


@pytest.mark.skipif(not H.available(), reason="scipy's bundled HiGHS is not importable")
def test_obs_verdicts_derived_again_with_highs(oracle):
    """The pursuit mission through HiGHS once more: verdicts, costs, points, x_ok flags and active obstacle rows of the file."""
    O = oracle
    fam, i = "obs", PV.OBS_SCENES["obs"].index("pursuit")
    Z = PV.load(fam)
    key = f"{fam}{i}_"
    with O.segments(PV.family_params(fam)[0]):
        ms, prm, ticks = _obs_replay(O, Z, fam, i)
        for tick, state, traj, o in ticks:
            k = tick - 1
            act = np.zeros(ms.qn, bool)
            v, c, x, ok = PV.tick_verdicts(O, H, fam, prm, ms, state, traj, tick, o, active=act)
            assert np.array_equal(v, Z[key + "verdict"][k]), (tick, v, Z[key + "verdict"][k])
            assert np.allclose(c, Z[key + "cost"][k], rtol=1e-9, atol=1e-12), tick
            assert np.abs(x - Z[key + "x"][k]).max() <= 1e-6, tick
            assert np.array_equal(ok, Z[key + "xok"][k]) and np.array_equal(act, Z[key + "obs_active"][k]), tick


@pytest.mark.parametrize("fam,i", OBS_MISSIONS)
def test_obstacle_set_gives_back_the_recorded_obstacle_states(fam, i):
    """lsc_planner_amd/obstacles.py::ObstacleSet, stepped from the recorded agent states, returns the recorded obstacle states bit for bit
    (tests/test_obstacle_reactive.py holds ObstacleSet to the device's motion stage through its host twin)."""
    from lsc_planner_amd.obstacles import ObstacleSet
    Z = PV.load(fam)
    key = f"{fam}{i}_"
    ms, obstacles, ticks = PV.obs_scene(PV.OBS_SCENES[fam][i])
    S = ObstacleSet(obstacles, n_agents=ms.qn)
    assert np.array_equal(S.radius, Z[key + "obs_radius"]) and np.array_equal(S.downwash, Z[key + "obs_downwash"])
    dt = PV.family_params(fam)[1]
    for tick in range(1, ticks + 1):
        pos, vel = S.at(dt * tick, Z[key + "states"][tick - 1][:, :3])
        got = np.concatenate([pos, vel], axis=1)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), Z[key + "obstacles"][tick - 1].view(np.int32)), tick
    if PV.OBS_SCENES[fam][i] == "pursuit":
        kinds = [o["type"] for o in obstacles]
        assert kinds.count("chasing") >= 2 and kinds.count("gaussian") == 1 and len({o["target"] for o in obstacles if o["type"] == "chasing"}) >= 2
        assert all(o["max_vel"] > ms.max_vel.max() for o in obstacles if o["type"] == "chasing")
        assert any(n > 0 for mo in S.motions for n in getattr(mo, "counts", {}).values())


# ------------------------------------------------------------------------------------------------ the modes family: the alternate planner modes
MODES_MISSIONS = [(fam, i) for fam in PV.MODES_FAMILIES for i in range(len(PV.MODES_SCENES[fam]))]


def test_modes_recorded_counts_are_the_generator_s_and_meet_the_conditions():
    from lsc_planner_amd.planner import next_state_host
    Z = PV.load("modes")
    for fam in PV.MODES_FAMILIES:
        assert PV.missions_of(Z, fam) == len(PV.MODES_SCENES[fam])
        assert PV.counts(Z, fam) == PV.COUNTS[fam], (fam, PV.counts(Z, fam))
        M, dt = PV.family_params(fam)[:2]
        for i, name in enumerate(PV.MODES_SCENES[fam]):
            key = f"{fam}{i}_"
            ms, events, ticks = PV.modes_scene(name)
            n = ms.qn
            assert (n == 64) == (name == "crowd") and (n == 64 or n <= 16) and ticks <= 16
            assert Z[key + "states"].shape == (ticks, n, 9) and Z[key + "trajs"].shape == (ticks, n, 3, 6 * M) and Z[key + "judged"].all()
            for k in PV.MISSION_KEYS:
                assert np.array_equal(Z[key + k], getattr(ms, k)), (name, k)
            # the record is a closed loop: a tick's state is the state the plans of the tick before lead to, with the tick's events
            for t in range(1, ticks):
                state = next_state_host(Z[key + "trajs"][t], dt=dt)
                PV.apply_events(state, events.get(t + 1, ()))
                assert np.array_equal(state, Z[key + "states"][t]), (name, t + 1)
            grown = Z[key + "slack_set"].reshape(ticks, -1).sum(axis=1)
            if "reset_threshold" in PV.MODES_PARAMS[name]["cfg"]:
                # unflagged ticks (nobody in a slack set: plan_agent plans the swarm), flagged ones, and ticks after the set has grown again
                assert grown[0] == 0 and (np.diff(grown) >= 0).all() and (np.diff(grown) > 0).sum() >= 2 and grown[-1] == grown[-2], (name, grown)
            else:
                assert not grown.any()
    got = PV.modes_conditions(Z)
    print(got)
    assert got == PV.MODES_COUNTS
    PV.assert_modes_conditions(got)
    assert os.path.getsize(os.path.join(PV.GOLDEN, PV.FILES["modes"])) <= os.path.getsize(os.path.join(PV.GOLDEN, PV.FILES["obs"]))


_MODES_REPLAYS = {}


def _modes_replay(O, Z, fam, i):
    """The oracle of the alternate modes over the recorded inputs of mission i, every tick in order on one swarm (computed once per
    mission and shared): (mission, params, modes, [(tick, state, plans, result)])."""
    if (fam, i) not in _MODES_REPLAYS:
        name = PV.MODES_SCENES[fam][i]
        ms = PV.mission(Z, fam, i)
        with O.segments(PV.family_params(fam)[0]):
            prm, md, sw = PV.modes_swarm(O, fam, name, ms)
            out = []
            for k, tick in PV.kept_ticks(Z, fam, i):
                assert tick == k + 1
                state, traj = PV.tick_inputs(Z, fam, i, k, tick)
                out.append((tick, state, traj, PV.modes_tick(sw, ms, state, traj, tick)))
        _MODES_REPLAYS[fam, i] = (ms, prm, md, out)
    return _MODES_REPLAYS[fam, i]


@pytest.mark.parametrize("fam,i", MODES_MISSIONS)
def test_oracle_of_the_modes_on_the_recorded_inputs_vs_the_recorded_verdicts(oracle, fam, i):
    """O.SwarmEx on the recorded inputs: status 1 exactly where HiGHS certifies infeasibility, HiGHS's cost elsewhere, HiGHS's plan where
    x_ok, the recorded rows and slack sets bit for bit, and for an infeasible agent the last plan it solved."""
    # (cost: the table's bound, the one the kernel is held to -- not this file's 1e-7, which was made for the LSC oracle and its exact finish:
    #  the oracle of the modes ends as an interior point, and on the half-second reset's sixth tick it stops 9.8e-7 relative above HiGHS)
    from tolerances import COST_ATOL, COST_RTOL, INTERIOR_POINT_TRAJ_ATOL
    O = oracle
    Z = PV.load(fam)
    key = f"{fam}{i}_"
    ms, prm, md, ticks = _modes_replay(O, Z, fam, i)
    rows_at = {int(t): r for r, t in enumerate(Z[key + "rows_ticks"])}
    last_ok = np.zeros_like(Z[key + "trajs"][0])
    if PV.modes_scene_params(fam, PV.MODES_SCENES[fam][i])[5]:
        last_ok[:, 2] = np.float32(prm.world_z_2d)             # (a planar agent's first plan lies in the plane: pin_variants.modes_swarm)
    for tick, state, traj, o in ticks:
        k = tick - 1
        v, c, x, x_ok = Z[key + "verdict"][k], Z[key + "cost"][k], Z[key + "x"][k], Z[key + "xok"][k]
        assert np.array_equal(o["status"], Z[key + "ostatus"][k]), (tick, o["status"])
        known = v >= 0
        assert np.array_equal(o["status"][known], (v[known] == 1).astype(np.int32)), (tick, o["status"], v)
        assert np.array_equal(o["slack_set"], Z[key + "slack_set"][k]), tick
        opt = v == 0
        assert (np.abs(o["cost"][opt] - c[opt]) <= COST_RTOL * np.abs(c[opt]) + COST_ATOL).all(), tick
        ub = v == 2
        assert (o["cost"][ub] <= c[ub] + COST_ATOL).all() and (o["cost"][ub] >= c[ub] * (1 - 1e-5) - COST_ATOL).all(), tick
        near = (opt | ub) & x_ok
        assert np.abs(o["traj"][near][:, :x.shape[1]].astype(np.float64) - x[near]).max(initial=0.0) <= INTERIOR_POINT_TRAJ_ATOL, tick
        bad = o["status"] == 1
        assert np.array_equal(o["traj"][bad], last_ok[bad]), tick
        last_ok[~bad] = o["traj"][~bad]
        if tick in rows_at:
            assert np.array_equal(o["normal"], Z[key + "normal"][rows_at[tick]]) and np.array_equal(o["d"], Z[key + "d"][rows_at[tick]]), tick
        if k + 1 < len(ticks):
            assert np.array_equal(Z[key + "trajs"][k + 1], o["traj"]), tick
    assert len(rows_at) >= (1 if ms.qn == 64 else 3)


# What goes through HiGHS once more -- about a minute of CPU time in all: the dynamical-limit scene whole (the objectives above 1e3), the
# reset's gust ticks, the tick on which the half-second scenes are pushed, and every sixteenth agent of the crowd's second tick with the
# agent that was given a velocity beyond its limit (a QP of the crowd has 2 000 rows and takes HiGHS a second).
MODES_SAMPLE = {"dynlimit": (None, None), "reset": ((5, 9, 12), None), "m4_collision": ((3,), None), "m4_reset": ((3, 6), None),
                "crowd": ((2,), (0, 7, 16, 32, 48))}


@pytest.mark.skipif(not H.available(), reason="scipy's bundled HiGHS is not importable")
@pytest.mark.parametrize("name", sorted(MODES_SAMPLE))
def test_modes_verdicts_derived_again_with_highs(oracle, name):
    O = oracle
    fam = next(f for f in PV.MODES_FAMILIES if name in PV.MODES_SCENES[f])
    i = PV.MODES_SCENES[fam].index(name)
    Z = PV.load(fam)
    key = f"{fam}{i}_"
    only_ticks, ag = MODES_SAMPLE[name]
    ms, prm, md, ticks = _modes_replay(O, Z, fam, i)
    with O.segments(PV.family_params(fam)[0]):
        for tick, state, traj, o in ticks:
            if only_ticks is not None and tick not in only_ticks:
                continue
            k = tick - 1
            ag_ = np.arange(ms.qn) if ag is None else np.asarray(ag)
            sl = np.zeros(ms.qn, bool)
            v, c, x, ok = PV.modes_tick_verdicts(O, H, fam, name, prm, md, ms, state, traj, tick, o, agents=ag_, slack=sl)
            assert np.array_equal(v[ag_], Z[key + "verdict"][k][ag_]), (tick, v, Z[key + "verdict"][k])
            assert np.allclose(c[ag_], Z[key + "cost"][k][ag_], rtol=1e-9, atol=1e-12), tick
            assert np.abs(x[ag_] - Z[key + "x"][k][ag_]).max() <= 1e-6, tick
            assert np.array_equal(ok[ag_], Z[key + "xok"][k][ag_]) and np.array_equal(sl[ag_], Z[key + "slack"][k][ag_]), tick
