"""-m gpu: the goal stage (csrc/lsc_mission.hip; lsc_mission_open / lsc_mission_set_state / lsc_set_goal_rule) -- patrol missions, GOBACK and
the right-hand goal rule as the first launch of a tick.

The reference leg of every closed loop is a per-tick loop on a context WITHOUT a mission state whose goal table the test rewrites between
ticks with the numpy restatement of src/traj_planner.cpp:477-538 (tests/patrol_reference.py): what a caller had to do before the stage
existed.  A context with a mission state must give that leg's plans, states, costs, statuses and tables bit for bit, however many ticks a
call flies.  Every statement about how many swaps happened is made on the reference leg.

Not tested here: the refusal of a communicator of several ranks (it needs several processes; the condition is the one line next to the
shard's in mission_tick_ok, csrc/lsc_abi.cpp)."""
import csv
import subprocess

import numpy as np
import pytest

import patrol_reference as R
from harness import circle
from test_gpu_flight import SIM, RESULT_TIME_COLUMN, SUMMARY_TIME_COLUMNS, Dev, _figures, _forest
from test_gpu_sim import _write_mission

pytestmark = pytest.mark.gpu

F = np.float32
OUTPUTS = ("traj", "state", "cost", "status", "iters")


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    return L


# ------------------------------------------------------------------------------------------------ the two legs
def reference_leg(L, ms, cfg, ticks, state_of=lambda tick: R.PATROL, rule=None, bt=None, setup=None, start=None, goal=None):
    """Per-tick loop without a mission state: rows[j] = tick j + 1 (inputs, outputs, the tables the host kept, unmet against the desired
    goals, the goal table the tick was handed)."""
    import torch
    d = Dev(L, ms, cfg, bt)
    t = R.Tables(ms, start, goal)
    rows = []
    try:
        if setup:
            setup(d.pl)
        for tick in range(1, ticks + 1):
            before = d.snapshot()
            pos, vel = before["state"][:, :3], before["state"][:, 3:6]
            swapped = t.step(state_of(tick), pos, cfg.goal_threshold)
            table = t.desired if rule is None else R.rule_goals(pos, vel, t.desired, tick, goal_threshold=cfg.goal_threshold, **rule)
            d.goal.copy_(torch.from_numpy(np.ascontiguousarray(table, F)))
            d.tick()
            after = d.snapshot()
            rows.append(dict(out={k: after[k] for k in OUTPUTS}, pos=pos.copy(), desired=t.desired.copy(), start=t.start.copy(), legs=t.legs.copy(),
                             swapped=swapped.copy(), table=np.array(table, F), unmet=int(R.unmet(pos, t.desired, cfg.goal_threshold).sum())))
    finally:
        d.close()
    return rows


def assert_is_row(d, row, what):
    """the device leg after its last call against the reference leg's row of that tick: outputs and tables"""
    snap = d.snapshot()
    for k in OUTPUTS:
        assert np.array_equal(snap[k], row["out"][k]), f"{what}: {k} differs"
    m = d.pl.mission_read()
    for k in ("desired", "start", "legs"):
        assert np.array_equal(m[k], row[k]), f"{what}: {k} {m[k].tolist()} != {row[k].tolist()}"


def mission_leg(L, ms, cfg, rows, calls, log=False, state_of=lambda tick: R.PATROL, bt=None, setup=None, start=None, goal=None, what=""):
    """A context with a mission state flies `calls` (ticks per lsc_fly_device call); after every call it must be the reference leg's row."""
    names = {R.GOTO: "goto", R.PATROL: "patrol", R.GOBACK: "goback"}
    d = Dev(L, ms, cfg, bt)
    try:
        if setup:
            setup(d.pl)
        d.pl.mission_open(start, goal, state=names[state_of(1)])
        d.goal.fill_(float("nan"))                  # (the ticks' goal argument is ignored while the state is open)
        if log:
            d.pl.flight_begin([0.0, 0.1], sum(calls), samples=False, safety=False, agents=False)
        for k in calls:
            for tick in range(d.seq + 1, d.seq + k + 1):
                assert state_of(tick) == state_of(d.seq + 1), "a call flies one planner state"
            d.pl.mission_state(names[state_of(d.seq + 1)])
            d.fly(k)
            assert_is_row(d, rows[d.seq - 1], f"{what} after tick {d.seq} ({k} per call)")
        if log:
            s = d.pl.flight_read(0, d.seq)["summary"]
            assert s["planner_seq"].tolist() == list(range(1, d.seq + 1))
            assert s["unmet"].tolist() == [r["unmet"] for r in rows[:d.seq]], what
            d.pl.flight_end()
    finally:
        d.close()


def chunks(ticks, k):
    return [k] * (ticks // k) + ([ticks % k] if ticks % k else [])


# ------------------------------------------------------------------------------------------------ 1. closed loop, lockstep
TICKS = 60
_legs = {}


def patrol_leg(L, n, goal_mode):
    if (n, goal_mode) not in _legs:
        ms = R.one_agent_mission() if n == 1 else R.two_agent_mission()
        cfg = L.PlannerConfig(goal_mode=goal_mode)
        _legs[n, goal_mode] = (ms, cfg, reference_leg(L, ms, cfg, TICKS))
    return _legs[n, goal_mode]


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("goal_mode", ["static", "prior_based"])
@pytest.mark.parametrize("n", [1, 2])
def test_patrol_flown_k_ticks_per_call_is_the_host_rewritten_loop(L, n, goal_mode, log):
    ms, cfg, rows = patrol_leg(L, n, goal_mode)
    swaps = [[j + 1 for j, r in enumerate(rows) if r["swapped"][q]] for q in range(n)]
    assert min(len(s) for s in swaps) >= 2, swaps                   # (on the reference leg)
    if n == 2:
        assert not set(swaps[0]) & set(swaps[1]), swaps
    for k in (1, 7, TICKS):
        mission_leg(L, ms, cfg, rows, chunks(TICKS, k), log=log, what=f"N={n} {goal_mode}")


# ------------------------------------------------------------------------------------------------ 2. one stage tick at the kernel's edges
@pytest.mark.parametrize("n", [64, 65, 256, 257])
def test_one_stage_tick_swaps_exactly_the_agents_inside_the_threshold(L, n):
    thr = 0.125
    radius = max(8.0, 0.7 * n / (2 * np.pi))
    ms = circle(L, n, radius)
    cfg = L.PlannerConfig(goal_threshold=thr)
    pos = (np.round(ms.start.astype(np.float64) * 64) / 64).astype(F)            # multiples of 1/64: the offsets below are exact in float32
    state = np.zeros((n, 9), F); state[:, :3] = pos
    traj = np.zeros((n, 3, 30), F)
    near = sorted(set(range(0, n, 3)) | {0, n - 1})
    goal = np.array(ms.goal, F)
    inside = [True, False, True, False, True, False]                          # exactly at the threshold (and beyond it): no swap
    expect = np.zeros(n, bool)
    for i, q in enumerate(near):
        p, g = pos[q], pos[q].copy()
        if i % 6 == 0:
            g[0] = p[0] + F(0.0625)
        elif i % 6 == 1:
            g[0] = p[0] + F(thr)                                              # exactly the threshold away along x
        elif i % 6 == 2:
            g[0] = np.nextafter(F(p[0] + F(thr)), p[0])                       # ... one ulp of that coordinate inside
        elif i % 6 == 3:
            g[1] = p[1] - F(thr)                                              # exactly the threshold, along -y
        elif i % 6 == 4:
            g[1], g[2] = p[1] + F(0.0625), p[2] - F(0.0625)
        else:
            g[1] = np.nextafter(F(p[1] + F(thr)), F(np.inf))                  # one ulp outside
        goal[q] = g
        expect[q] = inside[i % 6]
    start = (pos * F(0.5)).astype(F)
    t = R.Tables(ms, start, goal)
    swapped = t.step(R.PATROL, pos, thr)
    assert np.array_equal(swapped, expect) and expect[0] and expect.sum() >= len(near) // 2 - 1      # (the restatement, by construction)

    pl, plain = L.SwarmPlanner(ms, cfg), L.SwarmPlanner(ms, cfg)
    try:
        pl.mission_open(start, goal, state="patrol")
        g = pl.plan(state, None, traj)
        m = pl.mission_read()
        assert np.array_equal(m["legs"], expect.astype(np.int32)), np.nonzero(m["legs"] != expect)[0]
        assert np.array_equal(m["desired"], t.desired) and np.array_equal(m["start"], t.start)
        assert np.array_equal(m["desired"][expect], start[expect]) and np.array_equal(m["start"][expect], goal[expect])
        assert np.array_equal(m["desired"][~expect], goal[~expect]) and np.array_equal(m["start"][~expect], start[~expect])
        p = plain.plan(state, t.desired, traj)
        for k in ("traj", "cost", "status", "iters"):
            assert np.array_equal(g[k], p[k]), k
        assert np.array_equal(pl.last_goals(), plain.last_goals())
        # the same tick again in GOTO: nothing moves, and the plans are the plain context's
        pl.mission_state("goto")
        traj = g["traj"]                        # (planner_seq 2 reads a previous plan: the one just made, which starts where the agents are)
        g, p = pl.plan(state, None, traj), plain.plan(state, t.desired, traj)
        m2 = pl.mission_read()
        for k in m:
            assert np.array_equal(m[k], m2[k]), k
        for k in ("traj", "cost", "status", "iters"):
            assert np.array_equal(g[k], p[k]), "goto: " + k
    finally:
        pl.close(); plain.close()


# ------------------------------------------------------------------------------------------------ 3. GOBACK and back to PATROL
def test_goback_sends_everybody_home_and_patrol_resumes_from_there(L):
    ms, cfg, rows = patrol_leg(L, 2, "static")
    T = next(j + 1 for j, r in enumerate(rows) if r["swapped"].any())         # one agent has just swapped, the other is mid-leg
    assert rows[T - 1]["swapped"].sum() == 1 and R.unmet(rows[T - 1]["pos"], rows[T - 1]["desired"], 0.1).all()
    back, again = 45, 25
    state_of = lambda tick: R.PATROL if tick <= T or tick > T + back else R.GOBACK
    ref = reference_leg(L, ms, cfg, T + back + again, state_of)
    first = ref[T]                                                            # the first tick in GOBACK
    assert np.array_equal(first["desired"], ms.start) and np.array_equal(first["start"], ms.goal) and first["unmet"] == 2
    home = [j + 1 for j in range(T, T + back) if ref[j]["unmet"] == 0]
    assert home and home[0] > T + 5, home                                     # the flight reaches "all home" (isFinished in GOBACK)
    assert all(np.array_equal(r["desired"], ms.start) for r in ref[T:T + back])
    legs_home = ref[T + back - 1]["legs"]
    assert (ref[T + back]["legs"] == legs_home + 1).all()                     # at home each agent is at its desired goal: patrol swaps at once
    assert (ref[-1]["legs"] >= legs_home + 1).all() and np.array_equal(ref[T + back]["desired"], ms.goal)
    mission_leg(L, ms, cfg, ref, [T, 1, back - 1, again], log=True, state_of=state_of, what="goback")
    mission_leg(L, ms, cfg, ref, chunks(T, 7) + chunks(back, 7) + chunks(again, 7), state_of=state_of, what="goback by sevens")


# ------------------------------------------------------------------------------------------------ 4. the right-hand rule
def test_right_hand_rule_on_single_ticks(L):
    """Hand-made states through lsc_replan_tick: stalled and far; moving; at the goal; slower than the threshold by a little and far."""
    n = 4
    pos = np.asarray([[-3, -3, 1.0], [3, -3, 1.0], [-3, 3, 1.25], [3, 3, 0.75]], F)
    goal = np.asarray([[-1, -2, 1.5], [1, -3, 1.0], [-3, 3, 1.25], [2, 1, 1.0]], F)
    vel = np.asarray([[0, 0, 0], [-0.5, 0, 0], [0, 0, 0], [0.05, -0.05, 0.05]], F)
    ms = L.Mission(pos, goal, np.asarray([-6, -6, 0], F), np.asarray([6, 6, 2.5], F), np.full(n, 0.15), np.full(n, 2.0), np.ones((n, 3)),
                   np.full((n, 3), 2.0), np.full(n, 1.0), name="right_hand4")
    state = np.zeros((n, 9), F); state[:, :3] = pos; state[:, 3:6] = vel
    traj = np.repeat(pos[:, :, None], 30, axis=2).astype(F)                      # previous plan: everybody rests where it is
    pl, plain = L.SwarmPlanner(ms, L.PlannerConfig(goal_mode="right_hand")), L.SwarmPlanner(ms, L.PlannerConfig(goal_mode="static"))
    try:
        for seq, fired in ((5, [False] * 4), (6, [True, False, False, True])):
            table = R.rule_goals(pos, vel, goal, seq)
            assert (table != goal).any(axis=1).tolist() == fired, (seq, table)    # (the restatement, by hand)
            pl.planner_seq = plain.planner_seq = seq - 1
            g, p = pl.plan(state, goal, traj), plain.plan(state, table, traj)
            assert pl.last_goals().tobytes() == table.tobytes(), (seq, pl.last_goals(), table)
            for k in ("traj", "cost", "status", "iters"):
                assert np.array_equal(g[k], p[k]), (seq, k)
        assert np.array_equal(table[0], pos[0] + np.asarray([1, -2, 0], F))
        # the thresholds are the setter's: nobody is deadlocked at planner_seq 6 when it takes more than 6 plans
        pl.set_goal_rule("right_hand", 6, 0.1)
        pl.planner_seq = 5
        pl.plan(state, goal, traj)
        assert pl.last_goals().tobytes() == goal.tobytes()
        pl.set_goal_rule("config")
        pl.plan(state, goal, traj)
        assert pl.last_goals().tobytes() == goal.tobytes()
    finally:
        pl.close(); plain.close()


def test_right_hand_patrol_closed_loop(L):
    """A patrolling agent is slow and far from its new goal right after it swaps: the rule fires there.  40 ticks against the host-rewritten leg."""
    ms = R.two_agent_mission()
    rule = dict(seq_threshold=5, velocity_threshold=0.3)
    ref = reference_leg(L, ms, L.PlannerConfig(goal_mode="static"), 40, rule=rule)
    fired = [(r["table"] != r["desired"]).any() for r in ref]
    assert any(fired) and not all(fired), fired
    cfg = L.PlannerConfig(goal_mode="right_hand", deadlock_velocity_threshold=0.3)
    mission_leg(L, ms, cfg, ref, chunks(40, 7), log=True, what="right_hand")
    d = Dev(L, ms, cfg)
    try:
        d.pl.mission_open(state="patrol")
        d.fly(40)
        d.torch.cuda.synchronize()
        assert d.pl.last_goals().tobytes() == ref[-1]["table"].tobytes()
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 5. variants
@pytest.mark.parametrize("variant", ["m4", "planar", "forest", "obstacles"])
def test_variants_fly_the_host_rewritten_loop(L, tmp_path, variant):
    """One short flight each.  Agent 0's mission goal lies within the threshold of its start, so it swaps on every tick of the flight."""
    bt, setup, ticks = None, None, 8
    if variant == "m4":
        ms, cfg = L.circle_swap(5, 2.0), L.PlannerConfig(goal_mode="prior_based", dt=0.5, horizon=2.0)
    elif variant == "planar":
        ms, cfg = L.circle_swap(6, 2.0), L.PlannerConfig(goal_mode="prior_based", world_dimension=2, world_z_2d=1.0)
    elif variant == "forest":
        ms, bt = _forest(L, tmp_path, 6)
        cfg = L.PlannerConfig(use_octomap=True, goal_mode="prior_based")
    else:
        ms, cfg = L.circle_swap(6, 2.0), L.PlannerConfig(goal_mode="static")

        def setup(pl):
            pl.set_obstacles([0.2, 0.25], [1.5, 1.0])
            pl.obstacle_states([[0.3, 0.2, 1.0], [-0.4, -0.3, 1.2]], [[0.05, 0, 0], [0, -0.05, 0]])
    goal = np.array(ms.goal, F)
    goal[0] = ms.start[0] + np.asarray([0.03, 0.02, 0.0], F)
    ref = reference_leg(L, ms, cfg, ticks, bt=bt, setup=setup, goal=goal)
    assert ref[-1]["legs"][0] == ticks and not ref[-1]["legs"][1:].any()
    if variant != "obstacles":
        mission_leg(L, ms, cfg, ref, [3, ticks - 3], log=True, bt=bt, goal=goal, what=variant)
        return
    d = Dev(L, ms, cfg)                          # (lsc_fly_device is not built for dynamic obstacles: single fused ticks)
    try:
        setup(d.pl)
        d.pl.mission_open(goal=goal, state="patrol")
        for j in range(ticks):
            d.tick()
            assert_is_row(d, ref[j], f"obstacles tick {j + 1}")
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 6. refusals, and closing
def test_refusals_by_name_leave_the_context_as_it_was(L):
    ms = R.two_agent_mission()
    cfg = L.PlannerConfig(goal_mode="static")
    pl, twin, plain, other = (L.SwarmPlanner(ms, cfg) for _ in range(4))
    state = np.zeros((2, 9), F); state[:, :3] = ms.start
    traj = np.zeros((2, 3, 30), F)
    try:
        for p in (pl, twin):
            p.mission_open(state="patrol")

        def refused(word, call):
            with pytest.raises(L.LscError, match=word):
                call()
        refused("batch ticks", lambda: L.replan_tick_batch([other, pl], [state] * 2, [ms.goal] * 2, [traj] * 2, [1, 1]))
        refused("batch ticks", lambda: L.replan_tick_batch([pl, other], [state] * 2, [ms.goal] * 2, [traj] * 2, [1, 1]))
        pl.set_goal_trace(16)
        refused("goal trace", lambda: pl.plan(state, None, traj))
        pl.set_goal_trace(0)
        pl.goal_profile(1)
        refused("goal profiling", lambda: pl.plan(state, None, traj))
        pl.goal_profile(0)
        pl.set_shard(0, 1)
        refused("not the whole swarm", lambda: pl.plan(state, None, traj))
        pl.set_shard(0, 2)
        refused("goal_mode 0", lambda: L.SwarmPlanner(ms, L.PlannerConfig(goal_mode="prior_based")).set_goal_rule("right_hand"))
        pl.planner_seq = 0                      # (the refused ticks counted on the host side only)
        assert not pl.mission_read()["legs"].any()
        t = R.Tables(ms)
        for tick in range(1, 26):
            t.step(R.PATROL, state[:, :3])
            g, w, p = pl.plan(state, None, traj), twin.plan(state, None, traj), plain.plan(state, t.desired, traj)
            for k in ("traj", "cost", "status", "iters"):
                assert np.array_equal(g[k], w[k]) and np.array_equal(g[k], p[k]), (tick, k)
            traj = g["traj"]
            state = L.planner.next_state_host(traj)
        assert t.legs.any() and np.array_equal(pl.mission_read()["legs"], t.legs)
        # closed: the goal argument counts again, and the context plans what a context that never had a mission state plans
        pl.mission_close()
        refused("no mission state", lambda: pl.mission_read())
        for tick in range(26, 31):
            g, p = pl.plan(state, ms.goal, traj), plain.plan(state, ms.goal, traj)
            for k in ("traj", "cost", "status", "iters"):
                assert np.array_equal(g[k], p[k]), (tick, k)
            assert np.array_equal(pl.last_goals(), plain.last_goals())
            traj = g["traj"]
            state = L.planner.next_state_host(traj)
    finally:
        for p in (pl, twin, plain, other):
            p.close()


# ------------------------------------------------------------------------------------------------ 7. lsc_sim --patrol
@pytest.mark.parametrize("flags", [["--patrol", "--max-iter", "60"], ["--patrol", "--stop-patrol-at", "30"]])
def test_simulator_patrol_writes_the_same_run_with_the_device_loop(L, tmp_path, flags):
    ms = R.two_agent_mission()
    mp = tmp_path / "patrol2.json"
    _write_mission(str(mp), ms)
    runs = {}
    for name, extra in (("host", []), ("k7", ["--device-loop", "7"])):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([SIM, "--mission", str(mp), "--csv", str(out), "--quiet"] + flags + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, name + ": " + r.stdout + r.stderr
        runs[name] = (_figures(r.stdout), list(csv.reader(open(out / "result_LSC_2agents.csv"))), list(csv.reader(open(out / "summary_LSC_2agents.csv"))),
                      [ln for ln in r.stderr.splitlines() if "collision" in ln or "deadlock" in ln])
    fig, result, summary, lines = runs["host"]
    f2, r2, s2, l2 = runs["k7"]
    assert f2 == fig and l2 == lines, (f2, fig)
    assert len(result) == 1 + 2 * int(fig["ticks"]) and len(r2) == len(result) and r2[0] == result[0]
    for a, b in zip(result[1:], r2[1:]):
        assert [v for i, v in enumerate(a) if i % 15 != RESULT_TIME_COLUMN] == [v for i, v in enumerate(b) if i % 15 != RESULT_TIME_COLUMN]
    assert s2[0] == summary[0] and len(s2) == len(summary) == 2
    for col, a, b in zip(summary[0], summary[1], s2[1]):
        if col not in SUMMARY_TIME_COLUMNS and col != "mission_file_name":
            assert a == b, (col, a, b)
    px = np.asarray([[float(v) for v in row[15 * q + 2:15 * q + 5]] for row in result[1:] for q in range(2)]).reshape(-1, 2, 3)
    if "--max-iter" in flags:
        assert int(fig["ticks"]) == 59                                       # a patrol never finishes: the run goes to --max-iter
        far = np.linalg.norm(px - ms.start[None], axis=2).max(axis=0)
        assert (far > 0.8).all(), far                                        # ... and the agents did leave
    else:
        assert 30 < int(fig["ticks"]) < 120, fig
        # the last tick's input positions (its record time 0) are home; the CSV prints six digits, hence the 1e-5
        assert (np.linalg.norm(px[-2] - ms.start, axis=1) <= 0.1 + 1e-5).all(), px[-2]
        assert np.linalg.norm(px[58] - ms.start, axis=1).max() > 0.3         # tick 30 started away from home


def test_simulator_flies_the_right_hand_rule_and_says_so(L, tmp_path):
    mp = tmp_path / "patrol2.json"
    _write_mission(str(mp), R.two_agent_mission())
    r = subprocess.run([SIM, "--mission", str(mp), "--csv", str(tmp_path), "--quiet", "--goal-mode", "right_hand", "--max-iter", "40"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    head, row = list(csv.reader(open(tmp_path / "summary_LSC_2agents.csv")))
    assert row[head.index("goal_mode")] == "right_hand"
    for extra, word in ((["--patrol", "--on-deadlock", "noise"], "--on-deadlock noise"), (["--patrol", "--concurrent", "2"], "--concurrent"),
                        (["--stop-patrol-at", "5"], "needs --patrol")):
        r = subprocess.run([SIM, "--mission", str(mp), "--quiet"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
