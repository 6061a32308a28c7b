"""K closed-loop ticks per call (lsc_fly_device) and the flight log (csrc/lsc_flight.hip): the plans are those of single fused ticks, and
the log is the host's accounting -- lsc_safety_ratio's ratios and partners, getStateFromControlPoints' record samples, isFinished's and
checkDeadlock's counts.  Every comparison is bitwise: the same kernels plan, and the record repeats the reference's arithmetic."""
import os

import numpy as np
import pytest

from test_flight_host import _weights_restated      # (the reference's expression of the Bernstein weights, stated once)
from test_gpu_sim import _write_mission

pytestmark = pytest.mark.gpu

NC = 6


# ------------------------------------------------------------------------------------------------ numpy restatements
def _bezier(c, w):
    """getPointFromControlPoints: a double sum of float x double weight in index order, rounded to float; c [..., n + 1] float32."""
    x = np.zeros(c.shape[:-1], np.float64)
    for i, wi in enumerate(w):
        x = x + c[..., i].astype(np.float64) * wi
    return x.astype(np.float32)


def samples_ref(traj, times, dt, M):
    """getStateFromControlPoints (include/polynomial.hpp:63-97) for every agent and time: [T][N][9]."""
    traj = np.asarray(traj, np.float32).reshape(len(traj), 3, M * NC)
    out = np.zeros((len(times), len(traj), 9), np.float32)
    f5, f4, finv = np.float32(5), np.float32(4), np.float32(dt ** -1)
    for ti, t in enumerate(times):
        m, (w5, w4, w3) = _weights_restated(dt, t, M)
        c = traj[:, :, NC * m:NC * m + NC]
        v = ((c[..., 1:] - c[..., :-1]) * f5) * finv
        a = ((v[..., 1:] - v[..., :-1]) * f4) * finv
        assert v.dtype == np.float32 and a.dtype == np.float32
        out[ti, :, 0:3], out[ti, :, 3:6], out[ti, :, 6:9] = _bezier(c, w5), _bezier(v, w4), _bezier(a, w3)
    return out


def safety_ref(pos, radius, downwash):
    """savePlanningResult's pair loop (src/multi_sync_simulator.cpp:446-503) on sample positions pos [T][N][3]: ratio, first partner."""
    T, N = pos.shape[:2]
    ratio = np.full((T, N), 1e300)
    partner = np.full((T, N), -1, np.int32)
    for ti in range(T):
        for qi in range(N):
            for qj in range(N):
                if qi == qj:
                    continue
                ra, rb = radius[qi], radius[qj]
                dw = (downwash[qi] * ra + downwash[qj] * rb) / (ra + rb)
                d = pos[ti, qi] - pos[ti, qj]
                d[2] = np.float32(float(d[2]) / dw)
                n2 = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                r = np.sqrt(float(n2)) / (ra + rb)
                if r < ratio[ti, qi]:
                    ratio[ti, qi], partner[ti, qi] = r, qj
    return ratio, partner


def _distf(p, q):
    """octomath::Vector3::distance: float differences, products and sums, the square root in double."""
    d = np.asarray(p, np.float32) - np.asarray(q, np.float32)
    n2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert n2.dtype == np.float32
    return np.sqrt(n2.astype(np.float64))


def summary_ref(state, goal, traj_prev, traj_next, status, seq, M, goal_threshold=0.1):
    n = len(state)
    end = np.asarray(traj_next, np.float32).reshape(n, 3, M * NC)[:, :, -1]
    end_prev = np.asarray(traj_prev, np.float32).reshape(n, 3, M * NC)[:, :, -1]
    return dict(planner_seq=seq, unmet=int((_distf(state[:, :3], goal) > goal_threshold).sum()),
                end_unmet=int((_distf(end, goal) > goal_threshold).sum()),
                moved=n if seq <= 1 else int((_distf(end, end_prev) >= 1e-5).sum()),
                n_status=np.bincount(status, minlength=6)[:6].astype(np.int32)), end


# ------------------------------------------------------------------------------------------------ device-resident runs
class Dev:
    """A swarm on the device: two state buffers, two trajectory tables, the tick's outputs."""

    def __init__(self, L, ms, cfg, bt=None):
        import torch
        self.torch, self.ms = torch, ms
        self.pl = L.SwarmPlanner(ms, cfg)
        if bt is not None:
            self.pl.load_octomap(bt)
        dev = torch.device("cuda", 0)
        n, nv = ms.qn, self.pl.NV
        s0 = torch.zeros((n, 9), dtype=torch.float32, device=dev)
        s0[:, :3] = torch.from_numpy(ms.start).to(dev)
        self.states = [s0, torch.zeros_like(s0)]
        self.goal = torch.from_numpy(np.ascontiguousarray(ms.goal, np.float32)).to(dev).contiguous()
        self.trajs = [torch.zeros((n, nv), dtype=torch.float32, device=dev) for _ in range(2)]
        self.cost = torch.zeros(n, dtype=torch.float64, device=dev)
        self.status = torch.zeros(n, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(n, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.seq = 0            # ticks flown

    def fly(self, k):
        """k ticks by ONE call; the buffer pair is handed over in the order the next tick reads it"""
        j = self.seq & 1
        self.pl.fly([self.states[j], self.states[j ^ 1]], self.goal, [self.trajs[j], self.trajs[j ^ 1]], self.seq + 1, k, self.cost, self.status,
                    self.iters, self.stream)
        self.seq += k

    def tick(self):
        j = self.seq & 1
        self.pl.tick_device_fused(self.states[j], self.goal, self.trajs[j], self.trajs[j ^ 1], self.states[j ^ 1], self.cost, self.status,
                                  self.iters, self.seq + 1, self.stream)
        self.seq += 1

    def snapshot(self):
        """what the next tick would read, and the last tick's outputs"""
        self.torch.cuda.synchronize()
        j = self.seq & 1
        return {k: t.cpu().numpy().copy() for k, t in (("traj", self.trajs[j]), ("state", self.states[j]), ("cost", self.cost),
                                                       ("status", self.status), ("iters", self.iters))}

    def close(self):
        self.pl.close()


def assert_same_snapshot(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"


def single_ticks(L, ms, cfg, n, bt=None):
    """n single fused ticks on a context of its own: per tick (input state, input table, output table, cost, status), and the last snapshot"""
    d = Dev(L, ms, cfg, bt)
    rows = []
    try:
        for _ in range(n):
            before = d.snapshot()
            d.tick()
            after = d.snapshot()
            rows.append(dict(state=before["state"], prev=before["traj"], next=after["traj"], cost=after["cost"], status=after["status"],
                             iters=after["iters"], state_next=after["state"]))
    finally:
        d.close()
    return rows


def assert_log_is_the_accounting(ms, log, rows, times, dt, M, first_seq=1):
    """rows of the flight log against the numpy restatements on the single ticks' tables (rows[j]: tick j)"""
    for j, r in enumerate(rows):
        s = log["summary"][j]
        ref, end = summary_ref(r["state"], np.asarray(ms.goal, np.float32), r["prev"], r["next"], r["status"], first_seq + j, M)
        for k in ("planner_seq", "unmet", "end_unmet", "moved"):
            assert int(s[k]) == ref[k], f"tick {j}: {k} {int(s[k])} != {ref[k]}"
        assert np.array_equal(s["n_status"], ref["n_status"]), f"tick {j}: n_status"
        assert not s["pad"].any()
        smp = samples_ref(r["next"], times, dt, M)
        if "samples" in log:
            assert np.array_equal(log["samples"][j], smp), f"tick {j}: samples"
        if "ratio" in log:
            ratio, partner = safety_ref(smp[:, :, :3], ms.radius, ms.downwash)
            assert np.array_equal(log["ratio"][j], ratio), f"tick {j}: ratio"
            assert np.array_equal(log["partner"][j], partner), f"tick {j}: partner"
            assert s["min_ratio"] == ratio.min(), f"tick {j}: min_ratio"
        else:
            assert s["min_ratio"] == 1e300
        if "cost" in log:
            assert np.array_equal(log["cost"][j], r["cost"]) and np.array_equal(log["status"][j], r["status"]), f"tick {j}: cost / status"
            assert np.array_equal(log["end"][j], end), f"tick {j}: end point"


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    return L


def _sized(ms, n):
    ms.radius[:] = np.random.default_rng(3).uniform(0.1, 0.2, n)
    ms.downwash[:] = np.random.default_rng(4).uniform(1.0, 2.5, n)
    return ms


# ------------------------------------------------------------------------------------------------ 1. plans unchanged
@pytest.fixture(scope="module")
def circle8_single(L):
    ms = L.circle_swap(8, 2.0)
    cfg = L.PlannerConfig(goal_mode="prior_based", reset_threshold=0.15)
    return ms, cfg, single_ticks(L, ms, cfg, 12)


@pytest.mark.parametrize("record", [False, True])
def test_flown_plans_are_the_single_ticks_plans(L, circle8_single, record):
    ms, cfg, rows = circle8_single
    times = [0.0, 0.1]
    d = Dev(L, ms, cfg)
    try:
        if record:
            d.pl.flight_begin(times, 12)
        for k, upto in ((5, 5), (7, 12)):
            d.fly(k)
            snap = d.snapshot()
            ref = rows[upto - 1]
            assert_same_snapshot(snap, dict(traj=ref["next"], state=ref["state_next"], cost=ref["cost"], status=ref["status"], iters=ref["iters"]),
                                 f"after {upto} ticks (record {record})")
        if record:
            assert_log_is_the_accounting(ms, d.pl.flight_read(0, 12), rows, times, 0.2, 5)
            d.pl.flight_end()
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 2. the log is the host's accounting
@pytest.mark.parametrize("times", [[0.0, 0.1, 0.17], [0.0, 0.45]])
def test_log_equals_the_host_buffer_accounting(L, times):
    from lsc_planner_amd.planner import next_state_host
    n, ticks = 7, 6
    ms = _sized(L.random_swarm(n, world=(-3, -3, 0, 3, 3, 2.5), seed=31), n)
    cfg = L.PlannerConfig(goal_mode="static")
    d = Dev(L, ms, cfg)
    host = L.SwarmPlanner(ms, cfg)
    try:
        d.pl.flight_begin(times, ticks)
        d.fly(ticks)
        log = d.pl.flight_read(0, ticks)
        state = np.zeros((n, 9), np.float32)
        state[:, :3] = ms.start
        traj = np.zeros((n, 3, 30), np.float32)
        for j in range(ticks):
            prev = traj
            g = host.plan(state, ms.goal, traj)
            traj = g["traj"]
            ratio, partner, mn = host.safety_ratio(times)
            assert np.array_equal(log["ratio"][j], ratio) and np.array_equal(log["partner"][j], partner), f"tick {j}: ratio / partner"
            assert log["summary"][j]["min_ratio"] == mn, f"tick {j}: minimum"
            assert np.array_equal(log["cost"][j], g["cost"]) and np.array_equal(log["status"][j], g["status"]), f"tick {j}: cost / status"
            assert np.array_equal(log["samples"][j], samples_ref(traj, times, 0.2, 5)), f"tick {j}: samples"
            ref, end = summary_ref(state, ms.goal, prev, traj, g["status"], j + 1, 5)
            s = log["summary"][j]
            assert (int(s["planner_seq"]), int(s["unmet"]), int(s["end_unmet"]), int(s["moved"])) == (j + 1, ref["unmet"], ref["end_unmet"], ref["moved"]), f"tick {j}"
            assert np.array_equal(s["n_status"], ref["n_status"]) and np.array_equal(log["end"][j], end)
            state = next_state_host(traj)
    finally:
        d.close()
        host.close()


# ------------------------------------------------------------------------------------------------ 3. ties and edges
def test_the_first_partner_of_a_tie_stays(L):
    ms = L.circle_swap(4, 1.0)
    ms.start[:] = np.asarray([(1, 1, 1), (-1, 1, 1), (-1, -1, 1), (1, -1, 1)], np.float32)
    ms.goal[:] = -ms.start
    ms.goal[:, 2] = 1.0
    cfg = L.PlannerConfig(goal_mode="static")
    rows = single_ticks(L, ms, cfg, 2)
    d = Dev(L, ms, cfg)
    try:
        d.pl.flight_begin([0.0, 0.1], 2)
        d.fly(2)
        log = d.pl.flight_read(0, 2)
        assert_log_is_the_accounting(ms, log, rows, [0.0, 0.1], 0.2, 5)
        # at time 0 of the first tick every agent is 2 m from its two neighbours on the square: equal ratios, the lower index is named
        assert log["partner"][0][0].tolist() == [1, 0, 1, 0]
        assert (log["ratio"][0][0] == 2.0 / 0.3).all()
    finally:
        d.close()


@pytest.mark.parametrize("n,times", [(2, [0.0, 0.1]), (1, [0.0, 0.1]), (3, [0.1])])
def test_small_swarms_and_a_single_time(L, n, times):
    ms = L.circle_swap(n, 1.5)
    cfg = L.PlannerConfig(goal_mode="static")
    rows = single_ticks(L, ms, cfg, 3)
    d = Dev(L, ms, cfg)
    try:
        d.pl.flight_begin(times, 3)
        d.fly(3)
        log = d.pl.flight_read(0, 3)
        assert_log_is_the_accounting(ms, log, rows, times, 0.2, 5)
        if n == 1:
            assert (log["ratio"] == 1e300).all() and (log["partner"] == -1).all() and (log["summary"]["min_ratio"] == 1e300).all()
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 4. partner stride
@pytest.mark.parametrize("n", [65, 257])
def test_partners_beyond_a_wave_and_beyond_a_pass(L, n):
    from lsc_planner_amd.planner import next_state_host
    ms = _sized(L.random_swarm(n, world=(-6, -6, 0, 6, 6, 3.0), seed=57), n)
    cfg = L.PlannerConfig(goal_mode="static")
    times = [0.0, 0.1]
    d = Dev(L, ms, cfg)
    host = L.SwarmPlanner(ms, cfg)
    try:
        d.pl.flight_begin(times, 2, samples=False, agents=False)
        d.fly(2)
        log = d.pl.flight_read(0, 2)
        assert set(log) == {"summary", "ratio", "partner"}
        state = np.zeros((n, 9), np.float32)
        state[:, :3] = ms.start
        traj = np.zeros((n, 3, 30), np.float32)
        for j in range(2):
            traj = host.plan(state, ms.goal, traj)["traj"]
            ratio, partner, mn = host.safety_ratio(times)
            assert np.array_equal(log["ratio"][j], ratio) and np.array_equal(log["partner"][j], partner), f"tick {j}"
            assert log["summary"][j]["min_ratio"] == mn
            state = next_state_host(traj)
    finally:
        d.close()
        host.close()


# ------------------------------------------------------------------------------------------------ 5. capacity and refusals
def test_capacity_and_refusals(L):
    from lsc_planner_amd import LscError
    ms = L.circle_swap(6, 2.0)
    cfg = L.PlannerConfig(goal_mode="static")
    rows = single_ticks(L, ms, cfg, 5)
    d = Dev(L, ms, cfg)
    try:
        with pytest.raises(LscError, match="horizon"):
            d.pl.flight_begin([0.0, 1.2], 4)
        with pytest.raises(LscError, match="horizon"):
            d.pl.flight_begin([-0.1], 4)
        with pytest.raises(LscError):
            d.pl.flight_begin([0.0], 0)
        d.pl.flight_begin([0.0, 1.0], 4)                     # exactly the horizon is a record time
        d.fly(0)                                             # a no-op
        assert d.seq == 0
        d.fly(3)
        before = d.snapshot()
        with pytest.raises(LscError, match="lsc error -5.*do not fit"):
            d.fly(2)                                         # (nothing is flown)
        assert_same_snapshot(d.snapshot(), before, "a refused flight")
        with pytest.raises(LscError, match="lsc error -1.*not all flown"):
            d.pl.flight_read(2, 2)
        with pytest.raises(LscError, match="lsc error -1"):
            d.pl.flight_read(-1, 1)
        log = d.pl.flight_read(0, 3)
        assert_log_is_the_accounting(ms, log, rows[:3], [0.0, 1.0], 0.2, 5)
        tail = d.pl.flight_read(1, 2)                        # any range of flown rows
        assert np.array_equal(tail["ratio"], log["ratio"][1:]) and tail["summary"].tobytes() == log["summary"][1:].tobytes()
        d.pl.flight_reset()
        with pytest.raises(LscError, match="not all flown"):
            d.pl.flight_read(0, 1)
        d.fly(2)
        assert_log_is_the_accounting(ms, d.pl.flight_read(0, 2), rows[3:5], [0.0, 1.0], 0.2, 5, first_seq=4)
        assert_same_snapshot(d.snapshot(), dict(traj=rows[4]["next"], state=rows[4]["state_next"], cost=rows[4]["cost"], status=rows[4]["status"],
                                                iters=rows[4]["iters"]), "after a reset")
        # a context that plans a shard only
        d.pl.set_shard(0, 5)
        with pytest.raises(LscError, match="lsc error -1.*shard"):
            d.fly(1)
        with pytest.raises(LscError, match="lsc error -1.*shard"):
            d.pl.flight_begin([0.0], 2)
        d.pl.set_shard(0, 6)
        d.pl.flight_end()
        d.fly(1)                                             # no log open: it only flies
        with pytest.raises(LscError):
            d.pl.flight_read(0, 1)
    finally:
        d.close()


def test_record_launch_is_timed_as_group_six(L):
    ms = L.circle_swap(6, 2.0)
    d = Dev(L, ms, L.PlannerConfig(goal_mode="static"))
    try:
        d.pl.flight_begin([0.0, 0.1], 4)
        d.pl.set_timing(True)
        d.fly(4)
        d.torch.cuda.synchronize()
        t = d.pl.kernel_times_ms(6)
        assert len(t) == 4 and (t > 0).all() and (t < 1.0).all(), t
        assert d.pl.kernel_time_ms(0)[1] == 4
        d.pl.set_timing(False)
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 6. variants
def _forest(L, tmp_path, n):
    from lsc_planner_amd.maps import forest_leaves, write_bt
    leaves, res = forest_leaves()
    bt = os.path.join(str(tmp_path), "simple_forest.bt")
    write_bt(bt, leaves, res)
    world = (-5.0, -5.0, 0.0, 5.0, 5.0, 2.5)
    dist, kmin, r = L.edt_from_bt(bt, np.asarray(world[:3], np.float32), np.asarray(world[3:], np.float32))
    return L.random_swarm(n, world=world, seed=20260928, edt=dist, edt_key_min=kmin, edt_res=r), bt


@pytest.mark.parametrize("variant", ["m4", "planar", "forest"])
def test_variants_fly_their_single_ticks_and_log_their_accounting(L, tmp_path, variant):
    bt, dt, M = None, 0.2, 5
    if variant == "m4":
        ms, cfg, times, ticks, dt, M = L.circle_swap(5, 2.0), L.PlannerConfig(goal_mode="prior_based", dt=0.5, horizon=2.0), [0.0, 0.25], 4, 0.5, 4
    elif variant == "planar":
        ms, cfg, times, ticks = L.circle_swap(6, 2.0), L.PlannerConfig(goal_mode="prior_based", world_dimension=2, world_z_2d=1.0), [0.0, 0.1], 5
    else:
        ms, bt = _forest(L, tmp_path, 6)
        cfg, times, ticks = L.PlannerConfig(use_octomap=True, goal_mode="prior_based"), [0.0, 0.1], 4
    rows = single_ticks(L, ms, cfg, ticks, bt)
    d = Dev(L, ms, cfg, bt)
    try:
        d.pl.flight_begin(times, ticks)
        d.fly(ticks)
        ref = rows[-1]
        assert_same_snapshot(d.snapshot(), dict(traj=ref["next"], state=ref["state_next"], cost=ref["cost"], status=ref["status"], iters=ref["iters"]), variant)
        log = d.pl.flight_read(0, ticks)
        assert_log_is_the_accounting(ms, log, rows, times, dt, M)
        # ... and lsc_safety_ratio's, from a host-buffer context that plans the same ticks
        host = L.SwarmPlanner(ms, cfg)
        try:
            if bt is not None:
                host.load_octomap(bt)
            for j, r in enumerate(rows):
                g = host.plan(r["state"], ms.goal, r["prev"])
                assert np.array_equal(g["traj"].reshape(ms.qn, -1), r["next"]), f"{variant} tick {j}: host-buffer plan"
                ratio, partner, mn = host.safety_ratio(times)
                assert np.array_equal(log["ratio"][j], ratio) and np.array_equal(log["partner"][j], partner), f"{variant} tick {j}: ratio / partner"
                assert log["summary"][j]["min_ratio"] == mn
        finally:
            host.close()
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 7. lsc_sim --device-loop
SIM = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsc_planner_amd", "lsc_sim")
RESULT_TIME_COLUMN = 11          # planning_time, of the 15 columns per agent of the result CSV
SUMMARY_TIME_COLUMNS = {"average_planning_time", "min_planning_time", "max_planning_time", "initial_traj_planning_time", "obstacle_prediction_time",
                        "goal_planning_time", "lsc_generation_time", "sfc_generation_time", "traj_optimization_time"}


def _figures(stdout):
    """the simulator's closing figures that are not wall-clock times"""
    f = lambda key: stdout.split(key)[1].split()[0].rstrip(",")
    return {"flight time": f("total flight time:"), "distance": f("total distance:"), "safety ratio": f("safety ratio between agent:"),
            "collided": f("collided:"), "ticks": f("ticks:")}


def test_simulator_device_loop_writes_the_run_without_the_flag(L, tmp_path):
    import csv
    import subprocess
    mp = tmp_path / "circle6.json"
    _write_mission(str(mp), L.circle_swap(6, 2.0, world=(-5, -5, 0, 5, 5, 2.5)))
    runs = {}
    for name, extra in (("host", []), ("k7", ["--device-loop", "7"]), ("k1000", ["--device-loop", "1000"])):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([SIM, "--mission", str(mp), "--csv", str(out), "--quiet", "--max-noise", "0.02", "--noise-seed", "7"] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, name + ": " + r.stdout + r.stderr
        runs[name] = (_figures(r.stdout), list(csv.reader(open(out / "result_LSC_6agents.csv"))), list(csv.reader(open(out / "summary_LSC_6agents.csv"))),
                      [ln for ln in r.stderr.splitlines() if "collision" in ln or "deadlock" in ln])
    fig, result, summary, lines = runs["host"]
    assert int(fig["ticks"]) > 20 and float(fig["flight time"]) > 0 and len(result) == 1 + 2 * int(fig["ticks"])
    for name in ("k7", "k1000"):
        f2, r2, s2, l2 = runs[name]
        assert f2 == fig, (name, f2, fig)
        assert l2 == lines, name
        assert len(r2) == len(result) and r2[0] == result[0]
        for a, b in zip(result[1:], r2[1:]):
            assert [v for i, v in enumerate(a) if i % 15 != RESULT_TIME_COLUMN] == [v for i, v in enumerate(b) if i % 15 != RESULT_TIME_COLUMN], name
        assert s2[0] == summary[0] and len(s2) == len(summary) == 2
        for col, a, b in zip(summary[0], summary[1], s2[1]):
            if col not in SUMMARY_TIME_COLUMNS and col != "mission_file_name":
                assert a == b, (name, col, a, b)


def test_simulator_device_loop_names_the_same_deadlock_tick(ticks, tmp_path):
    import subprocess
    from conftest import golden_mission
    mp = tmp_path / "multi_simple4.json"
    _write_mission(str(mp), golden_mission(ticks, "multi_simple4"))
    said = []
    for extra in ([], ["--device-loop", "16"]):
        r = subprocess.run([SIM, "--mission", str(mp), "--max-iter", "90", "--on-deadlock", "report", "--quiet"] + extra, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        line = [ln for ln in r.stderr.splitlines() if "deadlock: no agent's horizon end point has moved for 20 ticks" in ln]
        assert len(line) == 1 and "applying it now" not in line[0], r.stderr
        said.append((line[0].split("(tick ")[1].split(")")[0], _figures(r.stdout)))
    assert said[0] == said[1], said


@pytest.mark.parametrize("extra,message", [(["--ranks", "2", "--rank", "0", "--comm-file", "token"], "--ranks"), (["--concurrent", "2"], "--concurrent"),
                                           (["--on-deadlock", "noise"], "--on-deadlock noise")])
def test_simulator_device_loop_refusals(L, tmp_path, extra, message):
    import subprocess
    mp = tmp_path / "circle6.json"
    _write_mission(str(mp), L.circle_swap(6, 2.0, world=(-5, -5, 0, 5, 5, 2.5)))
    r = subprocess.run([SIM, "--mission", str(mp), "--quiet", "--device-loop", "5"] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--device-loop does not combine with" in r.stderr and message in r.stderr, r.stdout + r.stderr
