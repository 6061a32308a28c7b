"""The yardstick of the dynamic obstacles, without a GPU: the composed reference tick (tests/obstacle_reference.py) against the oracle's own
Swarm.tick where the two must agree, the closed loop it is meant for, and the two new rules of csrc/lsc_rules.hpp compiled for the host."""
import os
import subprocess

import numpy as np
import pytest

import lsc_planner_amd as L
from lsc_planner_amd.planner import next_state_host
from obstacle_reference import (HOVER_DOWNWASH, HOVER_RADIUS, HOVER_TICKS, ObstacleSwarm, hover_mission, hover_states)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _phantom(ms, pos, radius, downwash):
    """The N + K swarm whose last K "agents" are the obstacles."""
    n, k = ms.qn, len(pos)
    return L.Mission(np.concatenate([ms.start, pos]).astype(np.float32), np.concatenate([ms.goal, pos]).astype(np.float32), ms.world_min,
                     ms.world_max, np.concatenate([ms.radius, radius]), np.concatenate([ms.downwash, downwash]),
                     np.concatenate([ms.max_vel, np.ones((k, 3))]), np.concatenate([ms.max_acc, 2 * np.ones((k, 3))]),
                     np.concatenate([ms.nominal_velocity, np.ones(k)]))


def _first_tick(oracle, agent_downwash, pos):
    ms = L.circle_swap(4, circle_radius=1.0, world=(-5, -5, 0, 5, 5, 2.5))
    ms.downwash[:] = agent_downwash
    pos = np.asarray(pos, np.float32)
    vel = np.array([[0.1, 0.0, 0.0], [0.0, -0.1, 0.05]], np.float32)
    rad, dw = np.array([0.25, 0.2]), np.array([1.5, 2.0])
    state = np.zeros((4, 9), np.float32); state[:, :3] = ms.start
    prev = np.zeros((4, 3, 30), np.float32)
    ref = ObstacleSwarm(oracle, ms, rad, dw).tick(state, ms.goal, prev, 1, pos, vel)
    ph = _phantom(ms, pos, rad, dw)
    sw = oracle.Swarm(oracle.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True), ph.radius, ph.downwash, ph.max_vel,
                      ph.max_acc, ph.nominal_velocity)
    st6 = np.zeros((6, 9), np.float32); st6[:, :3] = ph.start; st6[4:, 3:6] = vel
    o = sw.tick(st6, ph.goal, np.zeros((6, 3, 30), np.float32), 1, want_lsc=True)
    return ref, o


def test_composed_tick_equals_the_phantom_swarm_at_downwash_one(oracle):
    """planner_seq 1, every agent's downwash 1.0: an obstacle is then indistinguishable from a cooperating agent with its velocity -- the
    phantom swarm's agent rows [:4] carry the same obstacle list (3 agents, then the 2 phantoms) -- rows bit for bit, equal costs."""
    ref, o = _first_tick(oracle, 1.0, [[0.3, 0.2, 1.0], [-0.4, 0.1, 1.4]])
    assert np.array_equal(ref["normal"].view(np.uint32), o["normal"][:4].view(np.uint32))
    assert np.array_equal(ref["d"].view(np.uint64), o["d"][:4].view(np.uint64))
    assert (ref["status"] == 0).all() and (o["status"][:4] == 0).all()
    assert np.array_equal(ref["cost"], o["cost"][:4])
    assert np.array_equal(ref["traj"], o["traj"][:4])


def test_the_non_agent_downwash_rule_is_what_is_tested(oracle):
    """Agent downwash 2.0 and an obstacle 0.4 m above an agent: the agents' formula (the phantom swarm) and the non-agent rule differ."""
    ms = L.circle_swap(4, circle_radius=1.0, world=(-5, -5, 0, 5, 5, 2.5))
    above = ms.start[0] + np.array([0.05, 0.0, 0.4], np.float32)
    ref, o = _first_tick(oracle, 2.0, [above, [-0.4, 0.1, 1.4]])
    # agent columns agree, the obstacle's differ
    assert np.array_equal(ref["normal"][:, :3], o["normal"][:4, :3]) and np.array_equal(ref["d"][:, :3], o["d"][:4, :3])
    assert not (np.array_equal(ref["normal"][0, 3], o["normal"][0, 3]) and np.array_equal(ref["d"][0, 3], o["d"][0, 3]))


@pytest.fixture(scope="module")
def hover_flight(oracle):
    """The hover scenario flown by the composed reference alone, its own plans feeding the next tick."""
    ms = hover_mission()
    ref = ObstacleSwarm(oracle, ms, HOVER_RADIUS, HOVER_DOWNWASH)
    state = np.zeros((8, 9), np.float32); state[:, :3] = ms.start
    traj = np.zeros((8, 3, 30), np.float32)
    statuses, moved = [], 0
    for j in range(1, HOVER_TICKS + 1):
        pos, vel = hover_states(j)
        alone = ref.tick(state, ms.goal, traj, j, pos, vel, with_obstacles=False)
        r = ref.tick(state, ms.goal, traj, j, pos, vel)
        statuses.append(r["status"])
        moved += int((np.abs(r["traj"] - alone["traj"]).max(axis=(1, 2)) > 1e-3).sum())
        traj = r["traj"]
        state = next_state_host(traj)
    return np.array(statuses), moved, state, ms


def test_hover_scenario_is_feasible_and_not_vacuous(hover_flight):
    statuses, moved, state, ms = hover_flight
    assert statuses.shape == (HOVER_TICKS, 8) and (statuses == 0).all(), np.argwhere(statuses != 0)
    print("agent-ticks whose plan the obstacles moved by more than 1e-3 m:", moved)
    assert moved >= 10, moved


def test_obstacle_rules_of_the_header_on_the_host(oracle, tmp_path):
    """rule_obstacle_segment against const_vel_traj and rule_pair_downwash against the two formulas of src/traj_planner.cpp:1339-1345 in
    Python doubles, bit for bit, on seeded inputs (tests/native/obstacle_rules_check.cpp, built here for M = 5 and M = 4)."""
    src = os.path.join(ROOT, "tests", "native", "obstacle_rules_check.cpp")
    rng = np.random.default_rng(20261019)
    n = 200
    pv = np.concatenate([rng.uniform(-8, 8, (n, 3)), rng.normal(size=(n, 3)) * np.array([1.0, 1.0, 0.3])], axis=1).astype(np.float32)
    pv[0, 3:] = 0.0
    par = np.stack([rng.uniform(0.05, 0.4, n), rng.uniform(0.5, 3.0, n), rng.uniform(0.05, 0.5, n).astype(np.float32).astype(np.float64),
                    rng.uniform(0.5, 3.0, n).astype(np.float32).astype(np.float64)], axis=1)
    par[1, 1] = 1.0
    for m, dt in ((5, 0.2), (4, 0.5)):
        exe = str(tmp_path / f"obstacle_rules_check_m{m}")
        subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-O2", "-std=c++17", f"-DLSC_SEGMENTS={m}", "-o", exe, src])
        dtb = np.array([dt]).view(np.uint64)[0]
        text = "\n".join(" ".join(f"{w:x}" for w in pv[i].view(np.uint32)) + f" {dtb:x} " + " ".join(f"{w:x}" for w in par[i].view(np.uint64))
                         for i in range(n)) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
        assert len(out) == n
        with oracle.segments(m):
            for i, line in enumerate(out):
                words = line.split()
                seg = np.array([int(w, 16) for w in words[:m * 18]], np.uint32).reshape(m, 6, 3)
                ref = oracle.const_vel_traj(pv[i, :3], pv[i, 3:], dt)                      # [3][m * 6]
                assert np.array_equal(seg, ref.view(np.uint32).reshape(3, m, 6).transpose(1, 2, 0)), (m, i)
                dw = np.array([int(w, 16) for w in words[m * 18:]], np.uint64).view(np.float64)
                r_a, dw_a, r_o, dw_o = (float(v) for v in par[i])
                assert dw[0] == (dw_a * r_a + dw_o * r_o) / (r_a + r_o) and dw[1] == (r_a + dw_o * r_o) / (r_a + r_o), (m, i, dw)
