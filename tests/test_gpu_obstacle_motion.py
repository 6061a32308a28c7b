"""-m gpu: motion models on the device (lsc_obstacle_motion / lsc_obstacle_clock; csrc/lsc_obstacles.hip): the obstacle stage in front of a
tick and the obstacle track beside the flight log.

The stage is held to ObstacleSet.at at the clock's time: straight and multisim_patrol bit for bit, spin within one float32 step of the
rounded result (the bound of tests/test_obstacle_motion.py; the device's double sin / cos are not the host's).  The plan path is held to
today's tested path with no tolerance: a twin fed the read-back states by lsc_obstacle_states plans the same bits.  The track is held to
the float32 / float64 numpy restatement of tests/obstacle_track_reference.py, bit for bit.
"""
import numpy as np
import pytest

from harness import assert_lockstep, assert_tick_matches, circle, fly, same_bits, start_inputs
from obstacle_reference import HOVER_DOWNWASH, HOVER_RADIUS, HOVER_START, HOVER_VEL, ObstacleSwarm, hover_mission, hover_states
from obstacle_track_reference import track_reference
from test_obstacle_motion import PATROL, SPIN, STRAIGHT
from tolerances import ACTIVE_SET_TRAJ_ATOL, COST_ATOL

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
MIXED = [STRAIGHT, SPIN, PATROL]                       # one of each kind; EXACT: the two whose states are the host's bits
EXACT = [0, 2]
# the hover scenario's three spheres as straight models: 50 m on along their velocity, at its speed
HOVER_MODELS = [{"type": "straight", "start": list(map(float, s)), "goal": list(map(float, s + 50.0 * v / 0.05)), "speed": 0.05, "size": float(r),
                 "downwash": float(d)} for s, v, r, d in zip(HOVER_START, HOVER_VEL, HOVER_RADIUS, HOVER_DOWNWASH)]
TRACK_TIMES = {0.2: [0.0, 0.1], 0.5: [0.0, 0.25]}      # record times of a tick: the simulator's two per step


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


def _cfg(L, dt=0.2, **kw):
    kw.setdefault("solver", "active_set")
    if dt != 0.2:
        kw.update(dt=dt, horizon=4 * dt)               # (dt 0.5: the four-segment library)
    return L.PlannerConfig(**kw)


def _moving(L, ms, obstacles, dt=0.2, **kw):
    """A context that moves `obstacles` itself, its clock where the simulator's update() sets its times."""
    from lsc_planner_amd.obstacles import ObstacleSet
    pl = L.SwarmPlanner(ms, _cfg(L, dt, **kw))
    pl.set_obstacle_motion(ObstacleSet(obstacles))
    pl.obstacle_clock(dt, dt, dt)
    return pl


def _refused(L, call, code, *words):
    with pytest.raises(L.LscError) as e:
        call()
    msg = str(e.value)
    assert f"lsc error {code}:" in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def _assert_states(got, ref, exact, what):
    """(pos, vel) read back against ObstacleSet.at: the obstacles in `exact` bit for bit, the others within one float32 step."""
    for g, r in zip(got, ref):
        assert g.dtype == np.float32 and g.shape == r.shape, what
        for k in range(len(r)):
            if k in exact:
                assert same_bits(g[k], r[k]), (what, k, g[k], r[k])
            else:
                assert (np.abs(g[k].astype(np.float64) - r[k].astype(np.float64)) <= np.spacing(np.abs(r[k]))).all(), (what, k, g[k], r[k])


def _stage_against_obstacleset(L, obstacles, exact, ticks, dt=0.2):
    from lsc_planner_amd.obstacles import ObstacleSet
    ms, ref = hover_mission(), ObstacleSet(obstacles)
    pl = _moving(L, ms, obstacles, dt)
    clock = {"now": dt}

    def check(tick, state, traj, outs):
        t = clock["now"] - dt                          # the host's pair of statements
        clock["now"] += dt
        _assert_states(pl.obstacle_states_read(), ref.at(t), exact, (len(obstacles), tick))
        doubles = pl.obstacle_positions_read()                         # what the stage rounded: float32(doubles) is the state
        assert doubles.dtype == np.float64 and same_bits(doubles.astype(np.float32), pl.obstacle_states_read()[0]), tick
        assert pl.obstacle_clock_read() == clock["now"], tick
    fly(pl, ms, ticks, each_tick=check)
    pl.close()


# ------------------------------------------------------------------------------------------------ 1. the stage
@pytest.mark.parametrize("obstacles,exact,ticks", [(MIXED, EXACT, 30), ([PATROL], [0], 30)], ids=["K3", "K1"])
def test_stage_against_obstacleset(L, obstacles, exact, ticks):
    _stage_against_obstacleset(L, obstacles, exact, ticks)


def test_stage_with_a_full_wave_of_straights(L):
    """K = 64: every lane of the stage's workgroup; N - 1 + K = 71 obstacles per agent, the generic LSC build."""
    rng = np.random.default_rng(64)
    a, b = rng.uniform(-4, 4, (64, 3)) + [0, 0, 6], rng.uniform(-4, 4, (64, 3)) + [0, 0, 6]      # (above the swarm: the plans are not the point)
    obstacles = [dict(STRAIGHT, start=list(a[k]), goal=list(b[k]), speed=0.1 + 0.01 * k, size=0.1) for k in range(64)]
    _stage_against_obstacleset(L, obstacles, range(64), 1)


# ------------------------------------------------------------------------------------------------ 2. lockstep with a host-fed twin
class _Fed:
    """A context whose obstacles' states are fed, in front of every tick, what `source` read in its last tick."""

    def __init__(self, pl, source):
        self.pl, self.source = pl, source

    def plan(self, *a, **kw):
        self.pl.obstacle_states(*self.source.obstacle_states_read())
        return self.pl.plan(*a, **kw)

    def __getattr__(self, name):
        return getattr(self.pl, name)


def test_lockstep_with_a_host_fed_twin(L):
    from lsc_planner_amd.obstacles import ObstacleSet
    ms, s = hover_mission(), ObstacleSet(MIXED)
    pl, twin = _moving(L, ms, MIXED), L.SwarmPlanner(ms, _cfg(L))
    twin.set_obstacles(s.radius, s.downwash)
    fly([pl, _Fed(twin, pl)], ms, 40, each_tick=lambda tick, state, traj, outs: assert_lockstep(pl, twin, tick, outs, eq=same_bits))
    pl.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 3. the reference composition
def test_against_the_reference_composition(L, oracle):
    """Ticks 1 .. 12 of the hover scenario, the spheres as straight models; the reference tick is fed the states the stage wrote.  (Checked on
    the CPU: in this window the reference's own flight has plans the obstacles move by more than 1 mm -- see the assertion.)"""
    ms = hover_mission()
    pl = _moving(L, ms, HOVER_MODELS)
    ref = ObstacleSwarm(oracle, ms, HOVER_RADIUS, HOVER_DOWNWASH)
    moved = []

    def check(tick, state, traj, outs):
        pos, vel = pl.obstacle_states_read()
        hp, hv = hover_states(tick)
        assert np.abs(pos - hp).max() < 1e-6 and np.abs(vel - hv).max() < 1e-8, tick          # (the scenario of test_gpu_obstacles.py)
        r = ref.tick(state, ms.goal, traj, tick, pos, vel)
        assert_tick_matches(outs[0], r, tick, rows="bits", cost_atol=COST_ATOL, traj_atol=ACTIVE_SET_TRAJ_ATOL)
        bare = ref.tick(state, ms.goal, traj, tick, pos, vel, with_obstacles=False)
        moved.append(int((np.abs(outs[0]["traj"] - bare["traj"]).max(axis=(1, 2)) > 1e-3).sum()))
        ref.stale[:] = outs[0]["traj"]
    fly(pl, ms, 12, each_tick=check, want_constraints=True)
    print("agent-plans per tick that the obstacles moved by more than 1 mm:", moved)
    assert sum(moved) >= 1, moved
    pl.close()


# ------------------------------------------------------------------------------------------------ 4. / 5. K ticks per call, the track
class Loop:
    """The swarm on the device: K ticks per call (fly) or one fused tick per call (tick), on the same buffers either way."""

    def __init__(self, pl, ms):
        import torch
        self.torch, self.pl, self.flown = torch, pl, 0
        dev, N = torch.device("cuda", 0), ms.qn
        s0, _ = start_inputs(ms, pl.SEGV)
        self.states = [torch.from_numpy(s0).to(dev), torch.zeros((N, 9), device=dev)]
        self.trajs = [torch.zeros((N, 3 * pl.SEGV), device=dev), torch.zeros((N, 3 * pl.SEGV), device=dev)]
        self.goal = torch.from_numpy(np.ascontiguousarray(ms.goal, np.float32)).to(dev)
        self.cost = torch.zeros(N, dtype=torch.float64, device=dev)
        self.status, self.iters = torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)

    def _pair(self, bufs):
        return [bufs[self.flown & 1], bufs[(self.flown + 1) & 1]]

    def fly(self, n):
        self.pl.fly(self._pair(self.states), self.goal, self._pair(self.trajs), self.flown + 1, n, self.cost, self.status, self.iters)
        self.flown += n

    def tick(self):
        (s, sn), (t, tn) = self._pair(self.states), self._pair(self.trajs)
        self.pl.tick_device_fused(s, self.goal, t, tn, sn, self.cost, self.status, self.iters, self.flown + 1)
        self.flown += 1

    def results(self):
        self.torch.cuda.synchronize()
        return {"state": self.states[self.flown & 1].cpu().numpy(), "traj": self.trajs[self.flown & 1].cpu().numpy(), "cost": self.cost.cpu().numpy(),
                "status": self.status.cpu().numpy(), "iters": self.iters.cpu().numpy()}


def _recorded_flight(L, ms, obstacles, ticks, dt=0.2):
    """`ticks` ticks by one fly() with everything recorded -> (results, flight rows, track rows, the context's radii of the obstacles)."""
    pl = _moving(L, ms, obstacles, dt)
    pl.flight_begin(TRACK_TIMES[dt], ticks)
    lp = Loop(pl, ms)
    lp.fly(ticks)
    out = (lp.results(), pl.flight_read(0, ticks), pl.flight_obstacles_read(0, ticks))
    pl.flight_end()
    pl.close()
    return out


def _per_tick_flight(L, ms, obstacles, ticks, dt=0.2):
    """The same flight, one fused tick per call -> (results, the states every tick read [ticks][K][6])."""
    pl = _moving(L, ms, obstacles, dt)
    lp, states = Loop(pl, ms), []
    for _ in range(ticks):
        lp.tick()
        states.append(np.concatenate(pl.obstacle_states_read(), axis=1))
    out = (lp.results(), np.stack(states))
    pl.close()
    return out


def _assert_track(ms, obstacles, rows, track, where):
    """The track against the numpy restatement, from the flight log's samples and the track's own states."""
    from lsc_planner_amd.obstacles import ObstacleSet
    ratio, partner = track_reference(rows["samples"], track["pos_vel"], ms.radius, ObstacleSet(obstacles).radius)
    assert same_bits(track["ratio"], ratio), (where, np.abs(track["ratio"] - ratio).max())
    assert same_bits(track["partner"], partner), where
    assert same_bits(track["min_ratio"], ratio.min(axis=(1, 2))), where
    assert same_bits(track["below_one"], (ratio < 1).sum(axis=(1, 2)).astype(np.int32)), where


@pytest.fixture(scope="module")
def hover_flight(L):
    ms = hover_mission()
    return ms, _recorded_flight(L, ms, MIXED, 20), _per_tick_flight(L, ms, MIXED, 20)


def test_k_ticks_per_call_are_the_per_tick_loop(hover_flight):
    ms, (res, rows, track), (res1, states1) = hover_flight
    for k in ("state", "traj", "cost", "status", "iters"):
        assert same_bits(res[k], res1[k]), k
    # the flight rows are what a log without a track returns, in shape and in content: the last row's plan is the final table
    assert rows["samples"].shape == (20, 2, 8, 9) and rows["ratio"].shape == (20, 2, 8) and rows["partner"].shape == (20, 2, 8)
    assert rows["cost"].shape == (20, 8) and rows["status"].shape == (20, 8) and rows["end"].shape == (20, 8, 3)
    assert list(rows["summary"]["planner_seq"]) == list(range(1, 21))
    assert same_bits(rows["cost"][-1], res["cost"]) and same_bits(rows["status"][-1], res["status"])
    assert same_bits(rows["end"][-1], res["traj"].reshape(8, 3, -1)[:, :, -1])


def test_track_against_numpy(hover_flight):
    ms, (_, rows, track), (_, states1) = hover_flight
    assert track["pos_vel"].shape == (20, 3, 6) and track["ratio"].shape == (20, 2, 8)
    assert same_bits(track["pos_vel"], states1)                      # the tick's states, as the per-tick twin read them back
    assert track["positions"].shape == (20, 3, 3) and same_bits(track["positions"].astype(np.float32), track["pos_vel"][:, :, :3])
    assert (track["positions"] != track["pos_vel"][:, :, :3].astype(np.float64)).any()       # (doubles, not widened floats)
    _assert_track(ms, MIXED, rows, track, "hover")
    assert np.isfinite(track["min_ratio"]).all() and (track["min_ratio"] < 1e300).all() and set(np.unique(track["partner"])) <= {0, 1, 2}


def test_track_over_two_workgroups(L):
    """N = 130, T = 2, K = 5: 260 pairs spill into a second workgroup, whose atomics meet the first's in the summary."""
    ms = circle(L, 130, 16.0)
    rng = np.random.default_rng(130)
    obstacles = [dict(STRAIGHT, start=list(rng.uniform(-14, 14, 2)) + [1.0], goal=list(rng.uniform(-14, 14, 2)) + [1.2], speed=0.3, size=0.2) for _ in range(4)]
    # a sphere of 20 m parked 10 m above the swarm: every pair is below 1 whatever the QPs answer (an agent whose QP fails keeps a plan
    # inside the sphere as well), so the count has a share from each workgroup
    obstacles.append(dict(STRAIGHT, start=[0.0, 0.0, 11.0], goal=[0.0, 0.0, 11.0], size=20.0, speed=0.1))
    _, rows, track = _recorded_flight(L, ms, obstacles, 3)
    assert track["ratio"].shape == (3, 2, 130)
    _assert_track(ms, obstacles, rows, track, "N130")
    assert list(track["below_one"]) == [260, 260, 260], track["below_one"]          # 256 pairs of the first workgroup and 4 of the second


def test_track_counts_a_collision_and_is_reproducible(L):
    """A sphere of radius 1.5 m parked on agent 0's way, half way between its start and the origin: the ratio of agent 0 at record time 0 of
    tick 1 is below 1 whatever its QP answers -- solved, that sample is its input position, 1.58 m from the centre; failed, the agent keeps
    the zero plan of a first tick and the sample is the origin, 1.58 m from it as well.  The same flight twice: the same track rows."""
    ms = hover_mission()
    assert 1.5 < np.linalg.norm(ms.start[0]) / 2 < 1.65
    p = [float(x) for x in ms.start[0] / 2]
    obstacles = [dict(STRAIGHT, start=p, goal=p, size=1.5, speed=0.1), MIXED[2]]
    _, rows, track = _recorded_flight(L, ms, obstacles, 6)
    _assert_track(ms, obstacles, rows, track, "parked")
    assert track["below_one"][0] > 0 and track["ratio"][0, 0, 0] < 1 and track["partner"][0, 0, 0] == 0 and track["min_ratio"][0] < 1
    _, rows2, track2 = _recorded_flight(L, ms, obstacles, 6)
    for k in track:
        assert same_bits(track[k], track2[k]), k
    assert same_bits(rows["samples"], rows2["samples"])


# ------------------------------------------------------------------------------------------------ 6. the four-segment library
def test_the_four_segment_library(L):
    _stage_against_obstacleset(L, MIXED, EXACT, 5, dt=0.5)
    ms = hover_mission()
    res, rows, track = _recorded_flight(L, ms, MIXED, 5, dt=0.5)
    res1, states1 = _per_tick_flight(L, ms, MIXED, 5, dt=0.5)
    assert res["traj"].shape == (8, 3 * 24) and rows["samples"].shape == (5, 2, 8, 9)
    for k in ("state", "traj", "cost", "status", "iters"):
        assert same_bits(res[k], res1[k]), k
    assert same_bits(track["pos_vel"], states1)
    _assert_track(ms, MIXED, rows, track, "m4")


# ------------------------------------------------------------------------------------------------ 7. with a mission state open
def test_patrol_mission_state_with_moving_obstacles(L):
    """A patrol mission state and moving obstacles in one tick (stage order: obstacles, mission, goal ...): 15 ticks by one fly() against
    the per-tick loop, the same bits, tables included."""
    ms = circle(L, 8, 1.0)                              # (a small circle: agents arrive and swap within the window)
    got = []
    for per_call in (15, 1):
        pl = _moving(L, ms, MIXED)
        pl.mission_open(state="patrol")
        lp = Loop(pl, ms)
        for _ in range(15 // per_call):
            lp.fly(per_call) if per_call > 1 else lp.tick()
        got.append((lp.results(), pl.mission_read(), np.concatenate(pl.obstacle_states_read(), axis=1), pl.obstacle_clock_read()))
        pl.close()
    (a, ma, sa, ca), (b, mb, sb, cb) = got
    for k in a:
        assert same_bits(a[k], b[k]), k
    for x, y in zip(ma, mb):
        assert same_bits(x, y)
    assert same_bits(sa, sb) and ca == cb


# ------------------------------------------------------------------------------------------------ 8. refusals and lifetimes
def test_refusals_and_lifetimes(L):
    import torch
    from lsc_planner_amd.obstacles import ObstacleSet
    ms, s = hover_mission(), ObstacleSet(MIXED)
    models = s.models()
    state, traj = start_inputs(ms, 30)
    pl = L.SwarmPlanner(ms, _cfg(L))
    _refused(L, lambda: pl.set_obstacle_motion(models), ESTATE, "lsc_obstacle_motion", "lsc_set_obstacles")       # models before the obstacles
    pl.set_obstacles(s.radius, s.downwash)
    _refused(L, lambda: pl.set_obstacle_motion(models[:2]), EINVAL, "2 models", "3 obstacles")                     # K mismatch
    bad = [models[0], (0, 0.4, [[0.0, 0.0, 1.0], [np.nan, 0.0, 1.0]]), models[2]]
    _refused(L, lambda: pl.set_obstacle_motion(bad), EINVAL, "obstacle 1", "not finite")
    _refused(L, lambda: pl.set_obstacle_motion([models[0], models[1], (2, 0.5, [[1, 1, 1], [1, 1, 1]])]), EINVAL, "obstacle 2", "span no distance")
    _refused(L, lambda: pl.obstacle_clock(0.2, 0.2, 0.2), ESTATE, "no motion models")
    pl.set_obstacle_motion(models)
    _refused(L, lambda: pl.plan(state, ms.goal, traj), ESTATE, "no clock")                                         # a tick without a clock
    _refused(L, lambda: pl.obstacle_states(*s.at(0.0)), ESTATE, "moves its obstacles itself")
    _refused(L, lambda: pl.obstacle_states(torch.zeros((3, 6), device="cuda")), ESTATE, "moves its obstacles itself")
    pl.obstacle_clock(0.2, 0.2, 0.2)
    pl.planner_seq = 0
    first = pl.plan(state, ms.goal, traj)
    assert pl.obstacle_clock_read() == 0.2 + 0.2
    # a patrol tick beyond the walk's bound: refused in front of everything, the clock stays
    late = 0.2 + 65536.0 * 3.0 * 1.01                   # (PATROL's shortest leg: 1.5132 m at 0.5 m/s, a little over 3 s)
    pl.obstacle_clock(0.2, late, 0.2)
    _refused(L, lambda: pl.plan(state, ms.goal, traj), EINVAL, "obstacle 2", "65536")
    assert pl.obstacle_clock_read() == late
    # rows not flown; K ticks whose LAST time is beyond the bound enqueue nothing
    pl.obstacle_clock(0.2, late - 65536.0 * 3.0 * 0.02 - 0.4, 65536.0 * 3.0 * 0.01)
    pl.flight_begin([0.0, 0.1], 4)
    _refused(L, lambda: pl.flight_obstacles_read(0, 1), EINVAL, "not all flown")
    lp = Loop(pl, ms)
    _refused(L, lambda: lp.fly(4), EINVAL, "lsc_fly_device", "65536")
    torch.cuda.synchronize()
    assert not lp.trajs[1].any().item() and not lp.states[1].any().item()
    pl.flight_end()
    # removing the models restores today's refusals
    pl.set_obstacle_motion(None)
    _refused(L, lambda: pl.flight_begin([0.0, 0.1], 4), EINVAL, "lsc_flight_begin", "dynamic obstacles")
    _refused(L, lambda: pl.plan(state, ms.goal, traj), ESTATE, "no states")
    _refused(L, lambda: pl.obstacle_clock_read(), ESTATE, "no clock")
    _refused(L, lambda: pl.obstacle_positions_read(), ESTATE, "no motion models")
    # a log opened before the models (and a context without a track)
    bare = L.SwarmPlanner(ms, _cfg(L))
    bare.flight_begin([0.0, 0.1], 4)
    _refused(L, lambda: bare.flight_obstacles_read(0, 0), ESTATE, "obstacle track")
    bare.set_obstacle_motion(s)
    bare.obstacle_clock(0.2, 0.2, 0.2)
    lb = Loop(bare, ms)
    _refused(L, lambda: lb.fly(2), ESTATE, "lsc_fly_device", "obstacle track")
    torch.cuda.synchronize()
    assert not lb.trajs[1].any().item()
    bare.close()
    # lsc_set_obstacles drops the models
    pl.set_obstacle_motion(models)
    pl.set_obstacles(s.radius, s.downwash)
    _refused(L, lambda: pl.flight_begin([0.0, 0.1], 4), EINVAL, "dynamic obstacles")
    _refused(L, lambda: pl.obstacle_clock(0.2, 0.2, 0.2), ESTATE, "no motion models")
    # the context plans the same bits afterwards
    pl.set_obstacle_motion(models)
    pl.obstacle_clock(0.2, 0.2, 0.2)
    pl.planner_seq = 0
    again = pl.plan(state, ms.goal, traj)
    for k in ("traj", "cost", "status", "iters"):
        assert same_bits(again[k], first[k]), k
    pl.close()


# ------------------------------------------------------------------------------------------------ 9. a context that never installs models
def test_models_installed_and_removed_leave_todays_context(L):
    ms = hover_mission()
    never, had = L.SwarmPlanner(ms, _cfg(L)), L.SwarmPlanner(ms, _cfg(L))
    never.set_obstacles(HOVER_RADIUS, HOVER_DOWNWASH)
    had.set_obstacle_motion(HOVER_MODELS)
    had.obstacle_clock(0.2, 0.2, 0.2)
    state, traj = start_inputs(ms, had.SEGV)
    had.plan(state, ms.goal, traj)
    had.planner_seq = 0
    had.set_obstacle_motion([])

    class _Hover:
        def __init__(self, pl):
            self.pl = pl

        def plan(self, *a, **kw):
            self.pl.obstacle_states(*hover_states(self.pl.planner_seq + 1))
            return self.pl.plan(*a, **kw)

        def __getattr__(self, name):
            return getattr(self.pl, name)
    fly([_Hover(never), _Hover(had)], ms, 10, each_tick=lambda tick, st, tr, outs: assert_lockstep(never, had, tick, outs, eq=same_bits,
                                                                                                    keys=("traj", "cost", "status", "iters", "normal", "d")),
        want_constraints=True)
    never.close(); had.close()
