"""-m gpu: dynamic obstacles under the disturbance reset (lsc_set_obstacles_ex on a context with reset_threshold > 0: the ALT + OBS
instantiations of plan_agent, general_agent<., true>) against the composed reference of tests/obstacle_reset_reference.py, every tick.

Statuses and planned goals exactly; rows (normals, margins) bit for bit -- of every agent on every tick: the plan kernel dumps them for a
swarm nobody is flagged in, the alternate-mode solver for a flagged one --; cost within COST_RTOL / COST_ATOL; plans within
INTERIOR_POINT_TRAJ_ATOL for the agents the alternate-mode solver planned (a dense interior point) and within TRAJ_ATOL for the rest.
Each case proves its path through lsc_general_info and the note.  The scenes' own conditions are held on the reference alone, without a GPU,
by tests/test_obstacle_reset.py.
"""
import numpy as np
import pytest

from harness import assert_lockstep, assert_tick_matches, held_planner, same_bits, start_inputs
from obstacle_reset_reference import (CROWD_AGENT, CROWD_MAX_ACC, CROWD_PUSH_TICK, CROWD_TICKS, HOVER_DOWNWASH, HOVER_RADIUS, M4_DT, M4_PUSH_TICK,
                                      M4_TICKS, PUSHED_AGENT, PUSHED_BY, PUSHED_MAX_ACC, PUSHED_THRESHOLD, PUSHED_TICK, PUSHED_TICKS,
                                      ObstacleResetSwarm, crowd_scene, hover_mission, hover_states)
from tolerances import COST_ATOL, INTERIOR_POINT_TRAJ_ATOL, TRAJ_ATOL

pytestmark = pytest.mark.gpu

EINVAL = -1
FOLDED, LAUNCHED = 1, 2                  # lsc_general_info's last_launch


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


def _fly(pl, ref, ms, ticks, states_of, gusts, each_tick=None, dt=0.2, plan_atol=TRAJ_ATOL):
    """Closed loop on the context's own plans, every tick against the reference on the same inputs.  each_tick(tick, state, traj, pos, vel,
    g, r) sees what was compared.  Returns the reference's results."""
    from lsc_planner_amd.planner import next_state_host
    state, traj = start_inputs(ms, pl.SEGV)
    seen = []
    for tick in range(1, ticks + 1):
        if tick in gusts:
            q, off = gusts[tick]
            state[q, :3] += np.asarray(off, np.float32)
        pos, vel = states_of(tick)
        pl.obstacle_states(pos, vel)
        g = pl.plan(state, ms.goal, traj, want_constraints=True)
        r = ref.tick(state, ms.goal, traj, tick, pos, vel)
        assert g["normal"].shape == r["normal"].shape and g["d"].shape == r["d"].shape, tick
        assert np.array_equal(pl.last_goals(), r["goal"]), tick
        alt = r["alt"]
        assert_tick_matches(g, r, tick, rows="bits", cost_atol=COST_ATOL, traj_atol=INTERIOR_POINT_TRAJ_ATOL, traj_mask=alt)
        assert_tick_matches(g, r, tick, rows=False, cost_atol=COST_ATOL, traj_atol=plan_atol, traj_mask=~alt)
        if each_tick:
            each_tick(tick, state, traj, pos, vel, g, r)
        ok = r["status"] == 0
        ref.stale[ok] = g["traj"][ok]                  # (the optimiser's last good plan is the context's own)
        seen.append(r)
        traj = g["traj"]
        state = next_state_host(traj, dt=dt)
    return seen


def _pushed_hover_reference(oracle, ms, **kw):
    kw.setdefault("reset_threshold", PUSHED_THRESHOLD)
    return ObstacleResetSwarm(oracle, ms, HOVER_RADIUS, HOVER_DOWNWASH, kw.pop("max_acc", PUSHED_MAX_ACC), **kw)


GUST = {PUSHED_TICK: (PUSHED_AGENT, PUSHED_BY)}


def test_pushed_hover_default_solver_folds_the_hand_over(L, oracle):
    """Pushed hover, the default solver.  Ticks 1-11 run undisturbed through lsc_plan_alt_obs_kernel: bit-identical to a twin context with
    reset_threshold 0 (lsc_plan_obs_kernel), no status 6 left behind.  From tick 12 on every agent is planned by the alternate-mode
    solver inside the plan kernel (the folded hand-over), the spheres' rows of agent 2 with the full predicted size."""
    ms = hover_mission()
    pl = L.SwarmPlanner(ms, L.PlannerConfig(reset_threshold=PUSHED_THRESHOLD))
    twin = L.SwarmPlanner(ms, L.PlannerConfig(reset_threshold=0.0))
    pl.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH, max_acc=PUSHED_MAX_ACC)
    twin.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH)
    assert "dynamic obstacles: K = 3, 10 per agent, one wave per segment" in pl.note(), pl.note()
    lds_bound = pl.general_info()[0]
    assert lds_bound >= 10, lds_bound                   # (every row array of 7 agents + 3 spheres in LDS: general_agent<true>)
    ref = _pushed_hover_reference(oracle, ms)

    def each(tick, state, traj, pos, vel, g, r):
        assert pl.general_info()[1] == FOLDED, tick      # (the kernel that can fold: the ALT build)
        assert r["alt"].all() == (tick >= PUSHED_TICK) and r["alt"].any() == (tick >= PUSHED_TICK), tick
        if tick < PUSHED_TICK:
            twin.obstacle_states(pos, vel)
            t = twin.plan(state, ms.goal, traj, want_constraints=True)
            assert_lockstep(pl, twin, tick, (g, t), eq=same_bits, keys=("traj", "cost", "status", "iters", "normal", "d"))
        else:
            # agent 2's margins against the spheres are the size table + its radius, not the half separation
            d = g["d"][PUSHED_AGENT, 7:]
            assert np.array_equal(d, ref.size + float(ms.radius[PUSHED_AGENT])), tick
            assert (pl.row_counts() > 0).all(), tick

    seen = _fly(pl, ref, ms, PUSHED_TICKS, hover_states, GUST, each)
    assert all((r["status"] == 0).all() for r in seen)
    pl.close(); twin.close()


def test_pushed_hover_through_the_general_kernel_and_the_interior_point(L, oracle, monkeypatch):
    """The same with LSC_GENERAL_HANDOVER -- lsc_general_obs_kernel itself solves the flagged swarm in a launch behind the plan kernel -- and
    with solver = interior_point in the plan kernel."""
    ms = hover_mission()
    pl = held_planner(L, ms, lambda: L.PlannerConfig(reset_threshold=PUSHED_THRESHOLD, solver="interior_point"), monkeypatch,
                      "LSC_GENERAL_HANDOVER", True)
    pl.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH, max_acc=PUSHED_MAX_ACC)
    ref = _pushed_hover_reference(oracle, ms)

    def each(tick, state, traj, pos, vel, g, r):
        assert pl.general_info()[1] == (LAUNCHED if tick >= PUSHED_TICK else 0), (tick, pl.general_info())

    seen = _fly(pl, ref, ms, PUSHED_TICKS, hover_states, GUST, each)
    assert all((r["status"] == 0).all() for r in seen)
    pl.close()


def test_no_size_prediction_and_no_acceleration_are_the_radius(L, oracle):
    """size_prediction = False and max_acc = 0: both equal the reference with sizes r_o, and each other bit for bit."""
    ms = hover_mission()
    cfg = lambda: L.PlannerConfig(reset_threshold=PUSHED_THRESHOLD)
    off, still = L.SwarmPlanner(ms, cfg()), L.SwarmPlanner(ms, cfg())
    off.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH, max_acc=PUSHED_MAX_ACC, size_prediction=False)
    still.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH, max_acc=0.0)
    ref = _pushed_hover_reference(oracle, ms, size_prediction=False)
    r_o = HOVER_RADIUS.astype(np.float32).astype(np.float64)
    assert np.array_equal(ref.size, np.broadcast_to(r_o[:, None, None], ref.size.shape))
    assert np.array_equal(_pushed_hover_reference(oracle, ms, max_acc=0.0).size, ref.size)

    def each(tick, state, traj, pos, vel, g, r):
        still.obstacle_states(pos, vel)
        s = still.plan(state, ms.goal, traj, want_constraints=True)
        assert_lockstep(off, still, tick, (g, s), eq=same_bits, keys=("traj", "cost", "status", "iters", "normal", "d"))

    _fly(off, ref, ms, PUSHED_TICKS, hover_states, GUST, each)
    off.close(); still.close()


def test_four_segment_library(L, oracle):
    """The M = 4 library (dt 0.5, horizon 2.0, uncertainty horizon 1.0: M_u = 2): the hover circle, 8 ticks, the push in front of tick 4."""
    ms = hover_mission()
    pl = L.SwarmPlanner(ms, L.PlannerConfig(dt=M4_DT, horizon=2.0, reset_threshold=PUSHED_THRESHOLD))
    assert pl.M == 4
    pl.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH, max_acc=PUSHED_MAX_ACC, uncertainty_horizon=1.0)
    with oracle.segments(4):
        ref = _pushed_hover_reference(oracle, ms, dt=M4_DT)
        assert ref.size.shape == (3, 4, 6) and (ref.size[:, 2:] == ref.size[:, 2:3, :1]).all() and (ref.size[:, 1, 0] < ref.size[:, 2, 0]).all()

        def each(tick, state, traj, pos, vel, g, r):
            assert pl.general_info()[1] == FOLDED and r["alt"].all() == (tick >= M4_PUSH_TICK), tick

        _fly(pl, ref, ms, M4_TICKS, lambda j: hover_states(j, dt=M4_DT), {M4_PUSH_TICK: (PUSHED_AGENT, PUSHED_BY)}, each, dt=M4_DT)
    pl.close()


def test_more_kept_obstacles_than_the_lds_bound(L, oracle):
    """The obs family's crowd (12 agents, 54 spheres: 65 obstacles per agent), pruning off, max_acc 1.0, agent 0 pushed in front of tick 3,
    5 ticks: every flagged agent keeps all 65 obstacles, more than lsc_general_info's LDS bound, so general_agent<false, true> runs -- in a
    launch of its own (the context has a second pass, which does not fold)."""
    ms, rad, dw, states_of = crowd_scene()
    pl = L.SwarmPlanner(ms, L.PlannerConfig(reset_threshold=PUSHED_THRESHOLD, prune=False))
    pl.set_obstacles(rad, dw, max_acc=CROWD_MAX_ACC)
    assert "dynamic obstacles: K = 54, 65 per agent, generic pass (more than 64 obstacles)" in pl.note(), pl.note()
    lds_bound = pl.general_info()[0]
    assert 0 < lds_bound < 65, lds_bound
    ref = ObstacleResetSwarm(oracle, ms, rad, dw, CROWD_MAX_ACC, reset_threshold=PUSHED_THRESHOLD)

    def each(tick, state, traj, pos, vel, g, r):
        if tick >= CROWD_PUSH_TICK:
            assert pl.general_info()[1] in (FOLDED, LAUNCHED), tick
            # 27 rows per kept obstacle + M per obstacle of the slack set: everybody keeps all 65
            assert (pl.row_counts() >= 27 * 65).all() and (pl.row_counts() > 27 * lds_bound + 5 * lds_bound).all(), (tick, pl.row_counts())

    seen = _fly(pl, ref, ms, CROWD_TICKS, states_of, {CROWD_PUSH_TICK: (CROWD_AGENT, PUSHED_BY)}, each)
    assert sum(int((r["status"] != 0).sum()) for r in seen) * 4 <= CROWD_TICKS * ms.qn
    pl.close()


def _refused(L, call, *words):
    with pytest.raises(L.LscError) as e:
        call()
    msg = str(e.value)
    assert f"lsc error {EINVAL}:" in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def test_refusals_of_the_new_call_name_their_cause(L):
    """lsc_set_obstacles_ex refuses, naming the obstacle, a max_acc that is negative or not finite and a horizon that is negative, not
    finite or longer than the plan's; it refuses what lsc_set_obstacles refuses; the context stays usable, and lsc_set_obstacles on a
    context with reset_threshold > 0 is still refused."""
    ms = hover_mission()
    rad, dw, acc = HOVER_RADIUS, HOVER_DOWNWASH, PUSHED_MAX_ACC
    pl = L.SwarmPlanner(ms, L.PlannerConfig(reset_threshold=PUSHED_THRESHOLD))
    ex = "lsc_set_obstacles_ex"
    _refused(L, lambda: pl.set_obstacles(rad, dw, max_acc=[1.0, -0.5, 2.0]), ex, "max_acc of obstacle 1")
    _refused(L, lambda: pl.set_obstacles(rad, dw, max_acc=[1.0, 0.5, np.inf]), ex, "max_acc of obstacle 2")
    _refused(L, lambda: pl.set_obstacles(rad, dw, max_acc=[np.nan, 0.5, 1.0]), ex, "max_acc of obstacle 0")
    _refused(L, lambda: pl.set_obstacles(rad, dw, max_acc=acc, uncertainty_horizon=-0.2), ex, "uncertainty_horizon", "obstacle 0")
    _refused(L, lambda: pl.set_obstacles(rad, dw, max_acc=acc, uncertainty_horizon=np.nan), ex, "uncertainty_horizon", "obstacle 0")
    _refused(L, lambda: pl.set_obstacles(rad, dw, max_acc=acc, uncertainty_horizon=np.inf), ex, "uncertainty_horizon", "obstacle 0")
    _refused(L, lambda: pl.set_obstacles(rad, dw, max_acc=acc, uncertainty_horizon=1.2), ex, "uncertainty_horizon", "M = 5", "obstacle 0")
    _refused(L, lambda: pl.set_obstacles(rad, dw, max_acc=acc, uncertainty_horizon=1e300), ex, "uncertainty_horizon", "M = 5")
    _refused(L, lambda: pl.set_obstacles([0.2, 0.0, 0.1], dw, max_acc=acc), ex, "radius of obstacle 1")
    _refused(L, lambda: pl.set_obstacles(np.full(65, 0.2), np.ones(65), max_acc=1.0), ex, "K = 65")
    _refused(L, lambda: pl.set_obstacles(rad, dw), "lsc_set_obstacles:", "reset_threshold > 0", "lsc_set_obstacles_ex")
    for kw, word in ((dict(planner_mode="bvc"), "bvc"), (dict(slack_mode="dynamical_limit", planner_mode="bvc"), "slack mode"),
                     (dict(world_dimension=2), "world_dimension 2")):
        p = L.SwarmPlanner(ms, L.PlannerConfig(reset_threshold=PUSHED_THRESHOLD, **kw))
        _refused(L, lambda: p.set_obstacles(rad, dw, max_acc=acc), ex, "dynamic obstacles are not built for this context", word)
        p.close()
    pl.phase_profile(1)
    _refused(L, lambda: pl.set_obstacles(rad, dw, max_acc=acc), ex, "lsc_phase_profile")
    pl.phase_profile(0)
    # the longest horizon that is served: M dt
    pl.set_obstacles(rad, dw, max_acc=acc, uncertainty_horizon=1.0)
    state, traj = start_inputs(ms, pl.SEGV)
    pos, vel = hover_states(1)
    pl.obstacle_states(pos, vel)
    first = pl.plan(state, ms.goal, traj)
    assert (first["status"] == 0).all()
    _refused(L, lambda: pl.set_obstacles(rad, dw, max_acc=-acc), ex, "max_acc of obstacle 0")
    _refused(L, lambda: pl.phase_profile(1), "lsc_phase_profile", "dynamic obstacles")
    _refused(L, lambda: pl.dump_qp(0, "/dev/null"), "lsc_dump_qp", "dynamic obstacles")
    pl.set_shard(0, 4)
    _refused(L, lambda: pl.plan(state, ms.goal, traj), "shard is not the whole swarm")
    pl.set_shard(0, 8)
    # the refused calls changed nothing: the same tick, the same bits
    pl.planner_seq = 0
    pl.obstacle_states(pos, vel)
    again = pl.plan(state, ms.goal, traj)
    assert same_bits(again["traj"], first["traj"]) and same_bits(again["cost"], first["cost"])
    pl.close()


def test_k_ticks_per_call_with_models_are_the_per_tick_loop(L):
    """Pushed hover with the spheres as straight motion models on the device: fly() in batches of 4 with the push between two calls (in front
    of tick 13) against one fused tick per call with the same push.  Plans, states, costs, statuses and iterations after every batch, the
    rows every agent carried (they count the slack rows the `ever` flags on the device decide) and the obstacle track, bit for bit."""
    from lsc_planner_amd.obstacles import ObstacleSet
    from test_gpu_obstacle_motion import HOVER_MODELS, TRACK_TIMES, Loop
    ms, ticks, push_tick = hover_mission(), 20, 13

    def context():
        pl = L.SwarmPlanner(ms, L.PlannerConfig(reset_threshold=PUSHED_THRESHOLD))
        pl.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH, max_acc=PUSHED_MAX_ACC)
        pl.set_obstacle_motion(ObstacleSet(HOVER_MODELS))
        pl.obstacle_clock(0.2, 0.2, 0.2)
        return pl

    def push(lp):
        lp.states[lp.flown & 1][PUSHED_AGENT, :3] += lp.torch.tensor(PUSHED_BY, dtype=lp.torch.float32, device=lp.states[0].device)

    a, b = context(), context()
    a.flight_begin(TRACK_TIMES[0.2], ticks)
    la, lb = Loop(a, ms), Loop(b, ms)
    states_b, rows_before = [], None
    for first in range(1, ticks + 1, 4):
        if first == push_tick:
            push(la); push(lb)
        la.fly(4)
        for _ in range(4):
            lb.tick()
            states_b.append(np.concatenate(b.obstacle_states_read(), axis=1))
        ra, rb = la.results(), lb.results()
        for k in ("state", "traj", "cost", "status", "iters"):
            assert same_bits(ra[k], rb[k]), (first, k)
        assert (ra["status"] == 0).all(), (first, ra["status"])
        assert same_bits(a.row_counts(), b.row_counts()), first
        assert a.general_info()[1] == FOLDED and b.general_info()[1] == FOLDED, first
        if first + 4 == push_tick:
            rows_before = a.row_counts().copy()
    # the push changed the QPs' shape: group sign rows of the slack set exist from then on
    assert rows_before is not None and (a.row_counts() != rows_before).any()
    track = a.flight_obstacles_read(0, ticks)
    assert same_bits(track["pos_vel"], np.stack(states_b))
    log = a.flight_read(0, ticks)
    assert same_bits(log["status"][-1], ra["status"]) and same_bits(log["cost"][-1], ra["cost"])
    a.flight_end()
    a.close(); b.close()


def _sim(tmp, name, doc, *args):
    import json
    import os
    import subprocess
    sim = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsc_planner_amd", "lsc_sim")
    assert os.path.exists(sim), "lsc_sim not built"
    out = tmp / name
    out.mkdir()
    mp = out / "m.json"
    mp.write_text(json.dumps(doc))
    r = subprocess.run([sim, "--mission", str(mp), "--csv", str(out), "--quiet", "--max-iter", "120"] + list(args), capture_output=True, text=True, timeout=120)
    return r, out / "result_LSC_3agents.csv"


def test_simulator_flies_obstacles_at_the_default_threshold(tmp_path):
    """lsc_sim on the three-agent mission with its two obstacles, --obs-size-prediction true at the default reset_threshold: exit 0, and the
    CSV carries the obstacle cells.  The same with --obstacles-on-device --device-loop 5: the CSV is the same text cell for cell,
    planning_time (a wall clock) apart.  (Without the flag the mission still ends with exit status 2 at the default threshold:
    tests/test_gpu_obstacles.py.)"""
    import csv
    from obstacle_reference import sim_mission_doc
    doc = sim_mission_doc()
    assert all("max_acc" in o for o in doc["obstacles"])
    r, f = _sim(tmp_path, "host", doc, "--obs-size-prediction", "true")
    assert r.returncode == 0, r.stderr[-2000:]
    rows = list(csv.reader(open(f)))
    hdr_a, hdr_o = "id,t,px,py,pz,vx,vy,vz,ax,ay,az,planning_time,qp_cost,planning_report,size", "obs_id,t,px,py,pz,size"
    assert ",".join(rows[0]) == ",".join([hdr_a] * 3 + [hdr_o] * 2)
    assert all(len(row) == 57 for row in rows[1:]) and len(rows) > 20
    r2, f2 = _sim(tmp_path, "device", doc, "--obs-size-prediction", "true", "--obstacles-on-device", "--device-loop", "5")
    assert r2.returncode == 0, r2.stderr[-2000:]
    rows2 = list(csv.reader(open(f2)))
    strip = lambda rs: [[c for i, c in enumerate(row) if not (i < 45 and i % 15 == 11)] for row in rs]      # (11: planning_time)
    assert strip(rows) == strip(rows2)
