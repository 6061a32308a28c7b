"""The goal stage's rules (csrc/lsc_rules.hpp: rule_patrol_arrived, rule_patrol_swap, rule_goback_leg, rule_deadlock, rule_right_hand_goal)
without a GPU: compiled for the host by the test itself and held to the float32 numpy restatement of the reference's lines
(tests/patrol_reference.py; src/traj_planner.cpp:477-538, 1733-1740), and a two-agent patrol flown on the CPU with the oracle."""
import os
import subprocess

import numpy as np
import pytest

import patrol_reference as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "lsc_planner_amd", "csrc")
F = np.float32

CASE = np.dtype([("pos", F, 3), ("vel", F, 3), ("desired", F, 3), ("start", F, 3), ("seq", np.int32), ("seq_thr", np.int32),
                 ("goal_thr", np.float64), ("vel_thr", np.float64)])
OUT = np.dtype([("arrived", np.int32), ("unmet", np.int32), ("deadlock", np.int32), ("pad", np.int32), ("right", F, 3),
                ("swap_desired", F, 3), ("swap_start", F, 3), ("back_desired", F, 3), ("back_start", F, 3)])

HOST_RULES = r"""
// every case of the input file through the goal stage's rules, results to the output file (layouts: CASE / OUT of the test)
#include <cstdio>
#include <vector>
#include "lsc_rules.hpp"
struct Case { float pos[3], vel[3], desired[3], start[3]; int seq, seq_thr; double goal_thr, vel_thr; };
struct Out { int arrived, unmet, deadlock, pad; float right[3], swap_desired[3], swap_start[3], back_desired[3], back_start[3]; };
static void put(float *o, const lsc::F3 &v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
int main(int argc, char **argv)
{
    static_assert(sizeof(Case) == 72 && sizeof(Out) == 76, "the test's dtypes");
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    Case c;
    while (std::fread(&c, sizeof(c), 1, in) == 1) {
        Out o = {};
        o.arrived = lsc::rule_patrol_arrived(c.desired, c.pos, c.goal_thr);
        o.unmet = lsc::rule_goal_unmet(c.pos, c.desired, c.goal_thr);
        o.deadlock = lsc::rule_deadlock(c.pos, c.vel, c.desired, c.seq, c.seq_thr, c.vel_thr, c.goal_thr);
        put(o.right, lsc::rule_right_hand_goal(c.pos, c.desired));
        const lsc::MissionLeg s = lsc::rule_patrol_swap(c.desired, c.start);
        put(o.swap_desired, s.desired); put(o.swap_start, s.start);
        const lsc::MissionLeg b = lsc::rule_goback_leg(c.start, c.desired);      // (mission start, mission goal)
        put(o.back_desired, b.desired); put(o.back_start, b.start);
        if (std::fwrite(&o, sizeof(o), 1, out) != 1) return 3;
    }
    std::fclose(in); std::fclose(out);
    return 0;
}
"""


def _case(pos=(0, 0, 0), vel=(0, 0, 0), desired=(0, 0, 0), start=(9, 9, 9), seq=6, seq_thr=5, goal_thr=0.125, vel_thr=0.125):
    c = np.zeros(1, CASE)
    c["pos"], c["vel"], c["desired"], c["start"] = pos, vel, desired, start
    c["seq"], c["seq_thr"], c["goal_thr"], c["vel_thr"] = seq, seq_thr, goal_thr, vel_thr
    return c


THR = F(0.125)
INSIDE, OUTSIDE = np.nextafter(THR, F(0)), np.nextafter(THR, F(1))
NAMED = {
    "at_threshold": _case(desired=(THR, 0, 0)),                               # neither arrived nor unmet
    "at_threshold_shifted": _case(pos=(1, 2, 1), desired=(1.125, 2, 1)),
    "one_ulp_inside": _case(desired=(INSIDE, 0, 0)),
    "one_ulp_outside": _case(desired=(OUTSIDE, 0, 0)),
    "stalled_far_seq6": _case(desired=(2, 0, 0), seq=6),
    "stalled_far_seq5": _case(desired=(2, 0, 0), seq=5),
    "velocity_at_threshold": _case(desired=(2, 0, 0), vel=(THR, 0, 0)),
    "velocity_one_ulp_inside": _case(desired=(2, 0, 0), vel=(0, INSIDE, 0)),
    "velocity_one_ulp_outside": _case(desired=(2, 0, 0), vel=(0, 0, OUTSIDE)),
    "stalled_at_goal": _case(desired=(INSIDE, 0, 0), seq=9),
    "zeros_plus": _case(pos=(1, 1, 1), desired=(1, 1, 1)),
    "zeros_minus_dz": _case(pos=(1, 1, 1), desired=(2, 3, 1), vel=(-0.0, 0.0, -0.0)),
    "zeros_negative_pos": _case(pos=(-0.0, -0.0, -0.0), desired=(-0.0, 0.0, -0.0)),
    "below_goal": _case(pos=(0.5, -0.25, 2.0), desired=(-1.5, 0.75, 0.5)),
}


@pytest.fixture(scope="module")
def host_rules(tmp_path_factory):
    """-> run(cases) -> OUT array: the rules compiled for the host (no contraction: the reference's build has no fused multiply-add)"""
    d = tmp_path_factory.mktemp("mission_rules")
    src, exe = d / "mission_rules_host.cpp", d / "mission_rules_host"
    src.write_text(HOST_RULES)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(exe)])

    def run(cases):
        fin, fout = d / "cases.bin", d / "out.bin"
        np.ascontiguousarray(cases).tofile(fin)
        subprocess.check_call([str(exe), str(fin), str(fout)], timeout=60)
        out = np.fromfile(fout, OUT)
        assert len(out) == len(cases)
        return out
    return run


def _restated(c):
    o = np.zeros(len(c), OUT)
    for i, x in enumerate(c):
        o["arrived"][i] = R.arrived(x["desired"], x["pos"], x["goal_thr"])
        o["unmet"][i] = R.unmet(x["pos"], x["desired"], x["goal_thr"])
        o["deadlock"][i] = R.deadlock(x["pos"], x["vel"], x["desired"], x["seq"], x["seq_thr"], x["vel_thr"], x["goal_thr"])
        o["right"][i] = R.right_hand_goal(x["pos"], x["desired"])
    o["swap_desired"], o["swap_start"] = c["start"], c["desired"]             # :482-484
    o["back_desired"], o["back_start"] = c["start"], c["desired"]             # :488-489 with (mission start, mission goal) = (start, desired)
    return o


def test_rules_equal_the_restated_lines(host_rules):
    rng = np.random.default_rng(7)
    rnd = np.zeros(400, CASE)
    rnd["pos"] = rng.uniform(-3, 3, (400, 3))
    rnd["desired"] = rnd["pos"] + rng.uniform(-0.2, 0.2, (400, 3)) * rng.integers(0, 2, (400, 1))
    rnd["start"] = rng.uniform(-3, 3, (400, 3))
    rnd["vel"] = rng.uniform(-0.12, 0.12, (400, 3))
    rnd["seq"], rnd["seq_thr"] = rng.integers(1, 12, 400), 5
    rnd["goal_thr"], rnd["vel_thr"] = 0.1, 0.1
    cases = np.concatenate(list(NAMED.values()) + [rnd])
    got, ref = host_rules(cases), _restated(cases)
    for k in ("arrived", "unmet", "deadlock"):
        assert np.array_equal(got[k], ref[k]), (k, np.nonzero(got[k] != ref[k])[0])
    for k in ("right", "swap_desired", "swap_start", "back_desired", "back_start"):
        assert np.array_equal(got[k], ref[k]), (k, np.nonzero((got[k] != ref[k]).any(axis=1))[0])      # by value: -0.0 == 0.0
    assert 0 < got["arrived"][len(NAMED):].sum() < 400 and 0 < got["deadlock"][len(NAMED):].sum() < 400


def test_rules_at_their_edges(host_rules):
    """What the named cases must give, said by hand (the thresholds and offsets are exact in float32)."""
    names = list(NAMED)
    got = {n: o for n, o in zip(names, host_rules(np.concatenate([NAMED[n] for n in names])))}
    for n in ("at_threshold", "at_threshold_shifted"):
        assert got[n]["arrived"] == 0 and got[n]["unmet"] == 0, n          # exactly at the threshold: no swap, and not unmet
    assert got["one_ulp_inside"]["arrived"] == 1 and got["one_ulp_inside"]["unmet"] == 0
    assert got["one_ulp_outside"]["arrived"] == 0 and got["one_ulp_outside"]["unmet"] == 1
    assert got["stalled_far_seq6"]["deadlock"] == 1 and got["stalled_far_seq5"]["deadlock"] == 0      # planner_seq > 5
    assert got["velocity_at_threshold"]["deadlock"] == 0                     # norm < threshold, strictly
    assert got["velocity_one_ulp_inside"]["deadlock"] == 1 and got["velocity_one_ulp_outside"]["deadlock"] == 0
    assert got["stalled_at_goal"]["deadlock"] == 0
    assert np.array_equal(got["zeros_plus"]["right"], [1, 1, 1])
    assert np.array_equal(got["zeros_minus_dz"]["right"], np.asarray([1 + 2, 1 - 1, 1], F))      # (dy, -dx, 0) added to pos
    assert np.array_equal(got["zeros_negative_pos"]["right"], [0, 0, 0])
    assert np.array_equal(got["below_goal"]["right"], np.asarray([0.5 + 1.0, -0.25 + 2.0, 2.0], F))
    assert np.array_equal(got["stalled_far_seq6"]["swap_desired"], [9, 9, 9]) and np.array_equal(got["stalled_far_seq6"]["swap_start"], [2, 0, 0])


def fly_patrol_on_the_oracle(O, ms, ticks):
    """-> (tick of every swap per agent, legs): static goals, the numpy swap in front of every tick"""
    from conftest import oracle_swarm
    from harness import start_inputs
    from lsc_planner_amd.planner import next_state_host
    sw = oracle_swarm(O, ms)
    t = R.Tables(ms)
    state, traj = start_inputs(ms, 30)
    swaps = [[] for _ in range(ms.qn)]
    for tick in range(1, ticks + 1):
        for q in np.nonzero(t.step(R.PATROL, state[:, :3]))[0]:
            swaps[q].append(tick)
        sw.stale[:] = traj if tick > 1 else 0
        o = sw.tick(state, t.desired, traj, tick)
        assert (o["status"] == 0).all(), (tick, o["status"])
        traj = o["traj"]
        state = next_state_host(traj)
    return swaps, t.legs


def test_two_agent_patrol_swaps_on_the_cpu(oracle):
    """The mission the GPU tests fly: within 80 ticks each agent swaps at least twice, and the two never swap on the same tick."""
    ms = R.two_agent_mission()
    lengths = R.distf(ms.start, ms.goal)
    assert 0.9 < lengths[0] < 1.1 and 1.5 < lengths[1] < 1.7, lengths
    swaps, legs = fly_patrol_on_the_oracle(oracle, ms, 80)
    print("swap ticks", swaps)
    assert min(len(s) for s in swaps) >= 2 and legs.tolist() == [len(s) for s in swaps], swaps
    assert not set(swaps[0]) & set(swaps[1]), swaps
