"""-m gpu: chasing and gaussian obstacles on the device (lsc_obstacle_motion_ex; lsc_obstacle_step_kernel of csrc/lsc_obstacles.hip).

The stage is held to ObstacleSet (lsc_planner_amd/obstacles.py), an independent float64 restatement of getChasingObstacle /
getGaussianObstacle, bit for bit: both sides use + - x / sqrt and comparisons only, in the same order, nothing contracted.  The loop is
closed -- a chaser reads the agents, the agents plan against the chaser -- so one different bit in a chaser moves every later tick.
The scenario is tests/pursuit_scenario.py, whose branches tests/test_obstacle_reactive.py counts on the CPU.

The pursuit scenario's 12-entry table at cycle 0.5 serves 29 ticks of 0.2 s; the flights of 30 and 40 ticks use the same scenario with
the table drawn on to 17 entries (pursuit_scenario.py), so that every tick is flown.
"""
import csv
import json
import os
import re
import subprocess

import numpy as np
import pytest

from harness import assert_lockstep, circle, fly, same_bits, start_inputs
from obstacle_reference import sim_mission_doc
from pursuit_scenario import DT, acc_table, full_wave, hover_mission, pursuit
from test_gpu_obstacle_motion import EINVAL, ESTATE, MIXED, TRACK_TIMES, Loop, _cfg, _Fed, _refused

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


def _pursuing(L, ms, obstacles, dt=DT):
    """A context that moves `obstacles` itself; the first tick evaluates at now - start = dt."""
    from lsc_planner_amd.obstacles import ObstacleSet
    pl = L.SwarmPlanner(ms, _cfg(L, dt, reset_threshold=0.0))
    pl.set_obstacle_motion(ObstacleSet(obstacles, n_agents=ms.qn))
    pl.obstacle_clock(0.0, dt, dt)
    return pl


def _stage_against_obstacleset(L, ms, obstacles, ticks, dt=DT):
    """Closed loop on host buffers: after every tick the stage's float32 states, its positions in doubles and the chaser states against
    ObstacleSet stepped with the agent positions the tick read."""
    from lsc_planner_amd.obstacles import ObstacleSet
    ref = ObstacleSet(obstacles, n_agents=ms.qn)
    pl = _pursuing(L, ms, obstacles, dt)
    clock = {"now": dt}

    def check(tick, state, traj, outs):
        t = clock["now"] - 0.0                              # the host's pair of statements
        clock["now"] += dt
        pos, vel = ref.at(t, state[:, :3])
        got_pos, got_vel = pl.obstacle_states_read()
        assert same_bits(got_pos, pos), (tick, got_pos, pos)
        assert same_bits(got_vel, vel), (tick, got_vel, vel)
        assert same_bits(pl.obstacle_positions_read(), ref.positions), (tick, pl.obstacle_positions_read() - ref.positions)
        assert same_bits(pl.chaser_states_read(), ref.chaser_states()), tick
        assert pl.obstacle_clock_read() == clock["now"], tick
    fly(pl, ms, ticks, each_tick=check)
    pl.close()
    return ref


# ------------------------------------------------------------------------------------------------ 1. the stage, closed loop
def test_stage_against_obstacleset(L):
    ref = _stage_against_obstacleset(L, hover_mission(), pursuit(17), 30)
    # the flight itself took the branches the CPU test counts on agents at rest
    twin, lone, walker = ref.motions[0].counts, ref.motions[2].counts, ref.motions[3].counts
    assert twin["skipped"] == 29 and lone["zero_first_step"] == 1 and lone["repulsion"] >= 4, (twin, lone)
    assert all(ref.motions[k].counts["acc_clamp"] and ref.motions[k].counts["vel_clamp"] for k in (0, 1, 2))
    assert walker["capped"] and walker["applied"], walker


# ------------------------------------------------------------------------------------------------ 2. a full wave
def test_stage_with_a_full_wave_of_chasers(L):
    """K = 64 chasers, every one inside every other's Q*: a lane that stored before another had read, or skipped the barrier, would
    hand some chaser an obstacle of THIS tick."""
    ref = _stage_against_obstacleset(L, circle(L, 4, 3.0), full_wave(4), 5)
    assert all(mo.counts["repulsion"] == 4 * 63 for mo in ref.motions)


# ------------------------------------------------------------------------------------------------ 3. lockstep with a host-fed twin
def test_lockstep_with_a_host_fed_twin(L):
    from lsc_planner_amd.obstacles import ObstacleSet
    ms, obstacles = hover_mission(), pursuit(17)
    s = ObstacleSet(obstacles, n_agents=ms.qn)
    pl, twin = _pursuing(L, ms, obstacles), L.SwarmPlanner(ms, _cfg(L, reset_threshold=0.0))
    twin.set_obstacles(s.radius, s.downwash)
    fly([pl, _Fed(twin, pl)], ms, 40, each_tick=lambda tick, state, traj, outs: assert_lockstep(pl, twin, tick, outs, eq=same_bits))
    pl.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 4. K ticks per call
def _flights(L, ms, obstacles, ticks, dt=DT):
    """(one fly() of `ticks` ticks with the log and the track open, `ticks` single fused ticks): results, track rows / per-tick read-backs,
    final chaser states."""
    pl = _pursuing(L, ms, obstacles, dt)
    pl.flight_begin(TRACK_TIMES[dt], ticks)
    lp = Loop(pl, ms)
    lp.fly(ticks)
    many = (lp.results(), pl.flight_obstacles_read(0, ticks), pl.chaser_states_read())
    pl.flight_end()
    pl.close()
    pl = _pursuing(L, ms, obstacles, dt)
    lp, states, positions = Loop(pl, ms), [], []
    for _ in range(ticks):
        lp.tick()
        states.append(np.concatenate(pl.obstacle_states_read(), axis=1))
        positions.append(pl.obstacle_positions_read())
    single = (lp.results(), {"pos_vel": np.stack(states), "positions": np.stack(positions)}, pl.chaser_states_read())
    pl.close()
    return many, single


def test_k_ticks_per_call_are_the_per_tick_loop(L):
    """The stage of tick j reads tick j's own state buffer: 20 ticks by one call, chasers following the agents tick by tick, are the 20
    single ticks to the bit."""
    (res, track, chasers), (res1, track1, chasers1) = _flights(L, hover_mission(), pursuit(), 20)
    for k in ("state", "traj", "cost", "status", "iters"):
        assert same_bits(res[k], res1[k]), k
    assert track["pos_vel"].shape == (20, 5, 6) and track["positions"].shape == (20, 5, 3)
    assert same_bits(track["pos_vel"], track1["pos_vel"]) and same_bits(track["positions"], track1["positions"])
    assert same_bits(chasers, chasers1) and np.isfinite(chasers[:3]).all() and np.isnan(chasers[3:]).all()
    assert chasers[0, 6] == chasers[2, 6] and abs(chasers[0, 6] - 20 * DT) < 1e-12      # t_last: the clock's time of the last tick
    moved = np.abs(track["positions"][-1, :3] - track["positions"][0, :3]).max(axis=1)
    assert (moved > 0.05).all(), moved                      # (19 ticks at up to 0.3 m/s: the chasers chased)


# ------------------------------------------------------------------------------------------------ 5. the four-segment library
def test_the_four_segment_library(L):
    _stage_against_obstacleset(L, hover_mission(), pursuit(), 10, dt=0.5)


# ------------------------------------------------------------------------------------------------ 6. refusals and lifetimes
def test_refusals_and_lifetimes(L):
    from lsc_planner_amd.obstacles import ObstacleSet
    ms, obstacles = hover_mission(), pursuit()
    s = ObstacleSet(obstacles, n_agents=ms.qn)
    models, chasers, walkers = s.models(), s.chasers(), s.walkers()
    state, traj = start_inputs(ms, 30)
    pl = L.SwarmPlanner(ms, _cfg(L, reset_threshold=0.0))
    pl.set_obstacles(s.radius, s.downwash)
    _refused(L, lambda: pl.chaser_states_read(), ESTATE, "no chasing obstacles")
    # kind 3 through the old call names the new one; records that do not match the kinds
    _refused(L, lambda: pl.set_obstacle_motion(models), EINVAL, "lsc_obstacle_motion:", "obstacle 0", "lsc_obstacle_motion_ex")
    _refused(L, lambda: pl.set_obstacle_motion_ex(models, [dict(chasers[0], obstacle=4)] + chasers[1:], walkers), EINVAL, "obstacle 4", "kind 0")
    _refused(L, lambda: pl.set_obstacle_motion_ex(models, chasers, [dict(walkers[0], obstacle=2)]), EINVAL, "obstacle 2", "kind 3")
    _refused(L, lambda: pl.set_obstacle_motion_ex(models, chasers[:2], walkers), EINVAL, "obstacle 2", "no chaser record")
    _refused(L, lambda: pl.set_obstacle_motion_ex(models, chasers, []), EINVAL, "obstacle 3", "no walker record")
    _refused(L, lambda: pl.set_obstacle_motion_ex(models, chasers + [chasers[0]], walkers), EINVAL, "obstacle 0", "more than one")
    # the installation's own checks, naming the obstacle
    _refused(L, lambda: pl.set_obstacle_motion_ex(models, [chasers[0], dict(chasers[1], max_acc=0.01), chasers[2]], walkers), EINVAL, "obstacle 1", "max_acc")
    _refused(L, lambda: pl.set_obstacle_motion_ex(models, [chasers[0], chasers[1], dict(chasers[2], target=8)], walkers), EINVAL, "obstacle 2", "target")
    _refused(L, lambda: pl.set_obstacle_motion_ex(models, chasers, [dict(walkers[0], max_vel=float("nan"))]), EINVAL, "obstacle 3", "not finite")
    _refused(L, lambda: pl.set_obstacle_motion_ex(models, chasers, [dict(walkers[0], acc_update_cycle=0.0)]), EINVAL, "obstacle 3", "acc_update_cycle")
    _refused(L, lambda: pl.set_obstacle_motion_ex(models, chasers, [dict(walkers[0], acc=np.zeros((4097, 3)))]), EINVAL, "obstacle 3", "4096")
    _refused(L, lambda: pl.obstacle_clock(0.0, DT, DT), ESTATE, "no motion models")          # (nothing was installed by a refused call)
    pl.set_obstacle_motion(s)
    start = pl.chaser_states_read()
    assert same_bits(start, s.chaser_states()) and start[2].tolist() == [0.06, 0.08, 0.0, 0.0, 0.0, 0.0, 0.0]
    _refused(L, lambda: pl.obstacle_states(*s.at(0.0, ms.start)), ESTATE, "moves its obstacles itself")
    s.reset()
    pl.obstacle_clock(0.0, DT, DT)
    pl.planner_seq = 0
    first = pl.plan(state, ms.goal, traj)
    after = pl.chaser_states_read()
    assert after[0, 6] == DT and not same_bits(after, start)
    # a clock set backwards under a chaser: refused in front of everything; neither the clock nor the chasers move
    pl.obstacle_clock(0.0, 0.1, DT)
    _refused(L, lambda: pl.plan(state, ms.goal, traj), EINVAL, "obstacle 0", "backwards")
    assert pl.obstacle_clock_read() == 0.1 and same_bits(pl.chaser_states_read(), after)
    # a tick beyond the walker's table (12 entries at cycle 0.5: times below 6 s - 1e-5), alone and as the last of K ticks
    pl.obstacle_clock(0.0, 6.0, DT)
    _refused(L, lambda: pl.plan(state, ms.goal, traj), EINVAL, "gaussian obstacle 3", "12 entries")
    assert pl.obstacle_clock_read() == 6.0 and same_bits(pl.chaser_states_read(), after)
    pl.obstacle_clock(0.0, 6.0 - 3 * DT, DT)
    lp = Loop(pl, ms)
    _refused(L, lambda: lp.fly(4), EINVAL, "lsc_fly_device", "gaussian obstacle 3")
    lp.torch.cuda.synchronize()
    assert not lp.trajs[1].any().item() and pl.obstacle_clock_read() == 6.0 - 3 * DT and same_bits(pl.chaser_states_read(), after)
    # re-installation puts the chasers back: the same first tick again, to the bit
    pl.set_obstacle_motion(s)
    assert same_bits(pl.chaser_states_read(), start)
    pl.obstacle_clock(0.0, DT, DT)
    pl.planner_seq = 0
    again = pl.plan(state, ms.goal, traj)
    for k in ("traj", "cost", "status", "iters"):
        assert same_bits(again[k], first[k]), k
    assert same_bits(pl.chaser_states_read(), after)
    # lsc_set_obstacles drops everything
    pl.set_obstacles(s.radius, s.downwash)
    _refused(L, lambda: pl.chaser_states_read(), ESTATE, "no chasing obstacles")
    _refused(L, lambda: pl.obstacle_clock(0.0, DT, DT), ESTATE, "no motion models")
    _refused(L, lambda: pl.plan(state, ms.goal, traj), ESTATE, "no states")
    # ... and so does removing the models
    pl.set_obstacle_motion(s)
    pl.set_obstacle_motion(None)
    _refused(L, lambda: pl.chaser_states_read(), ESTATE, "no chasing obstacles")
    pl.close()


# ------------------------------------------------------------------------------------------------ 7. kinds 0 to 2 through the new call
def test_closed_forms_through_the_new_call_are_unaffected(L):
    from lsc_planner_amd.obstacles import ObstacleSet
    ms, s = hover_mission(), ObstacleSet(MIXED)
    old, new = L.SwarmPlanner(ms, _cfg(L)), L.SwarmPlanner(ms, _cfg(L))
    old.set_obstacle_motion(s)
    new.set_obstacles(s.radius, s.downwash)
    new.set_obstacle_motion_ex(s.models(), [], [])
    _refused(L, lambda: new.chaser_states_read(), ESTATE, "no chasing obstacles")
    for pl in (old, new):
        pl.obstacle_clock(DT, DT, DT)

    def check(tick, state, traj, outs):
        assert_lockstep(new, old, tick, outs, eq=same_bits)
        for a, b in zip(new.obstacle_states_read(), old.obstacle_states_read()):
            assert same_bits(a, b), tick
        assert same_bits(new.obstacle_positions_read(), old.obstacle_positions_read()), tick
    fly([new, old], ms, 10, each_tick=check)
    old.close(); new.close()


# ------------------------------------------------------------------------------------------------ 8. the simulator
SIM = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsc_planner_amd", "lsc_sim")
SIM_RUNS = {"host": [], "device": ["--obstacles-on-device"], "loop": ["--obstacles-on-device", "--device-loop", "10"]}


def _sim_pursuit():
    """The pursuit obstacles over the three-agent mission of the simulator's tests (the lone chaser aimed at agent 2), the walker's history
    written into the file: 26 entries at cycle 0.5 for the 50 ticks of 0.2 s."""
    obstacles = pursuit()
    obstacles[2] = dict(obstacles[2], target=2)
    obstacles[3] = dict(obstacles[3], acc_history=acc_table(26).tolist())
    return sim_mission_doc(obstacles)


def test_simulator_three_ways_write_the_same_csv(tmp_path):
    """lsc_sim per tick with the chasers stepped on the host (lsc_obstacle_states), with --obstacles-on-device, and with --device-loop 10:
    the same CSV, cell for cell as text except planning_time (a wall clock), and the same printed obstacle safety ratio."""
    assert os.path.exists(SIM), "lsc_sim not built"
    rows, summary = {}, {}
    for run, flags in SIM_RUNS.items():
        d = tmp_path / run
        d.mkdir()
        (d / "m.json").write_text(json.dumps(_sim_pursuit()))
        r = subprocess.run([SIM, "--mission", str(d / "m.json"), "--csv", str(d), "--quiet", "--max-iter", "50", "--reset-threshold", "0",
                            "--on-deadlock", "report"] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (run, r.returncode, r.stderr[-1500:])            # (a run that crashed: nothing more is started)
        rows[run] = [[c for i, c in enumerate(row) if not (i < 45 and i % 15 == 11)] for row in csv.reader(open(d / "result_LSC_3agents.csv"))]
        ratio = re.search(r"safety ratio between agent and obstacle: (\S+)", r.stdout)
        assert ratio, r.stdout[-800:]
        summary[run] = (ratio.group(1), re.search(r"safety ratio between agent: (\S+)", r.stdout).group(1), re.search(r"collided: (\d)", r.stdout).group(1))
    assert len(rows["host"]) > 20 and all(len(row) == 3 * 14 + 5 * 6 for row in rows["host"][1:])
    for run in ("device", "loop"):
        differing = [(j, i, x, y) for j, (ra, rb) in enumerate(zip(rows["host"], rows[run])) for i, (x, y) in enumerate(zip(ra, rb)) if x != y]
        assert len(rows[run]) == len(rows["host"]) and not differing, (run, len(differing), differing[:6])
        assert summary[run] == summary["host"], summary
    chaser_cells = {tuple(row[42 + 2:42 + 5]) for row in rows["host"][1:]}
    assert len(chaser_cells) > 20                                                   # (the chaser moved)
