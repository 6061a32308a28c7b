"""Chasing and gaussian obstacles without a GPU: ObstacleSet's float64 restatement (lsc_planner_amd/obstacles.py) on the pursuit scenario,
and the statements the device stage runs (csrc/lsc_obstacle_motion.hpp: obstacle_chase_step, obstacle_gaussian_at and the installation
checks) compiled for the host by the test itself, in a stand-alone program, and held to ObstacleSet bit for bit.

Both sides use + - x / sqrt and comparisons only, every operation correctly rounded and nothing contracted (-ffp-contract=off), in the
same order: the doubles are equal, not close.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from lsc_planner_amd.obstacles import ObstacleSet
from pursuit_scenario import DT, acc_table, chaser, pursuit
from test_obstacle_motion_device_rules import MODEL, models_of

CSRC = os.path.join(ROOT, "lsc_planner_amd", "csrc")
N_AGENTS, STEPS = 8, 60

# one obstacle as the host program reads it: the model of kinds 0 to 2, or a chaser's / walker's record
REC = np.dtype([("kind", np.int32), ("target", np.int32), ("n_acc", np.int32), ("acc_first", np.int32), ("start", np.float64, 3), ("initial_vel", np.float64, 3),
                ("radius", np.float64), ("max_vel", np.float64), ("max_acc", np.float64), ("gamma_target", np.float64), ("gamma_obs", np.float64),
                ("cycle", np.float64), ("message_radius", np.float64), ("model", MODEL)])
HEAD = np.dtype([("steps", np.int32), ("agents", np.int32), ("K", np.int32), ("n_acc", np.int32)])
# per step and obstacle: the build's code, position and velocity in doubles, the chaser's state (NaN for the others)
OUT = np.dtype([("code", np.int32), ("pad", np.int32), ("pos", np.float64, 3), ("vel", np.float64, 3), ("state", np.float64, 7)])

HOST_PROGRAM = r"""
// The obstacle stage on the host: every obstacle of the scene file at every time, a chaser against the obstacles of the previous step (zeros
// and no radii before the first) and its target's position of the step's agent table -- the order of lsc_obstacle_step_kernel: read the
// previous step, then write.  `messages` prints obstacle_refusal_ex of every code.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/lsc_planner_amd.h"
#include "lsc_obstacle_motion.hpp"
struct Head { int steps, agents, K, n_acc; };
struct Rec { int kind, target, n_acc, acc_first; double start[3], initial_vel[3], radius, max_vel, max_acc, gamma_target, gamma_obs, cycle, message_radius; lsc_obstacle_model model; };
struct Out { int code, pad; double pos[3], vel[3], state[7]; };
int main(int argc, char **argv)
{
    using namespace lsc;
    static_assert(sizeof(Rec) == 16 + 13 * 8 + 208 && sizeof(Out) == 8 + 13 * 8, "the test's dtypes");
    if (argc == 2 && !std::strcmp(argv[1], "messages")) {
        for (int why = 1; why <= 11; why++) std::printf("%d: %s\n", why, obstacle_refusal_ex(why));
        return 0;
    }
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    Head h;
    if (std::fread(&h, sizeof(h), 1, in) != 1) return 2;
    std::vector<Rec> rec(h.K);
    std::vector<double> acc(3 * (size_t)h.n_acc + 3), times(h.steps);
    std::vector<float> agents((size_t)h.steps * h.agents * 3);
    if (std::fread(rec.data(), sizeof(Rec), h.K, in) != (size_t)h.K || std::fread(acc.data(), 24, h.n_acc, in) != (size_t)h.n_acc ||
        std::fread(times.data(), 8, h.steps, in) != (size_t)h.steps || std::fread(agents.data(), 4, agents.size(), in) != agents.size()) return 2;
    std::vector<ObstacleEntry> entry(h.K);
    std::vector<ObstacleChaser> ch(h.K);
    std::vector<ObstacleWalker> wk(h.K);
    std::vector<ObstacleChaserState> st(h.K);
    std::vector<int> code(h.K);
    std::vector<double> radius(h.K);
    for (int o = 0; o < h.K; o++) {
        const Rec &r = rec[o];
        radius[o] = r.message_radius;
        if (r.kind == OBSTACLE_CHASING) {
            code[o] = obstacle_chaser_build(r.target, h.agents, r.start, r.radius, r.max_vel, r.max_acc, r.gamma_target, r.gamma_obs, ch[o]);
            st[o] = ObstacleChaserState{{r.start[0], r.start[1], r.start[2]}, {0.0, 0.0, 0.0}, 0.0};
        } else if (r.kind == OBSTACLE_GAUSSIAN) {
            code[o] = obstacle_walker_build(r.start, r.initial_vel, r.max_vel, r.cycle, r.n_acc, acc.data() + 3 * (size_t)r.acc_first, r.acc_first, wk[o]);
        } else {
            code[o] = obstacle_entry_build(r.model.kind, r.model.n_points, r.model.speed, r.model.points, entry[o]);
        }
    }
    std::vector<double> prev(3 * (size_t)h.K, 0.0), next(3 * (size_t)h.K, 0.0);
    for (int j = 0; j < h.steps; j++) {
        for (int o = 0; o < h.K; o++) {
            Out w = {};
            w.code = code[o];
            for (double &x : w.state) x = std::nan("");
            double p[3] = {0, 0, 0}, v[3] = {0, 0, 0};
            if (!code[o] && rec[o].kind == OBSTACLE_CHASING) {
                const float *a = agents.data() + ((size_t)j * h.agents + ch[o].target) * 3;
                const double goal[3] = {(double)a[0], (double)a[1], (double)a[2]};
                obstacle_chase_step(ch[o], st[o], times[j], goal, reinterpret_cast<const double (*)[3]>(prev.data()), j == 0 ? nullptr : radius.data(), h.K, o);
                for (int k = 0; k < 3; k++) { p[k] = st[o].pos[k]; v[k] = st[o].vel[k]; }
                std::memcpy(w.state, &st[o], sizeof(w.state));
            } else if (!code[o] && rec[o].kind == OBSTACLE_GAUSSIAN) {
                if (obstacle_walker_entries(wk[o], times[j]) <= (double)wk[o].n_acc)
                    obstacle_gaussian_at(wk[o], reinterpret_cast<const double (*)[3]>(acc.data() + 3 * (size_t)wk[o].acc_first), times[j], p, v);
                else w.code = -1;
            } else if (!code[o]) {
                obstacle_at(entry[o], times[j], p, v);
            }
            for (int k = 0; k < 3; k++) { w.pos[k] = next[3 * o + k] = p[k]; w.vel[k] = v[k]; }
            if (std::fwrite(&w, sizeof(w), 1, out) != 1) return 3;
        }
        prev = next;
    }
    std::fclose(in); std::fclose(out);
    return 0;
}
"""


def scripted_agents(steps=STEPS, n=N_AGENTS):
    """float32 [steps][n][3]: agents on slow circles of their own, so that every chaser's goal point moves every step."""
    j = np.arange(steps)[:, None]
    q = np.arange(n)[None, :]
    ang = 0.7 * q + 0.05 * j
    return np.stack([(2.0 + 0.1 * q) * np.cos(ang), (2.0 + 0.1 * q) * np.sin(ang), 1.0 + 0.02 * j + 0.0 * q], axis=2).astype(np.float32)


def records_of(obstacles):
    """REC rows and the acceleration table of mission obstacles, without ObstacleSet's checks."""
    rec, acc = np.zeros(len(obstacles), REC), []
    for r, o in zip(rec, obstacles):
        r["message_radius"] = np.float32(o["size"])                 # (dynamic_msgs::Obstacle::radius)
        if o["type"] == "chasing":
            r["kind"], r["target"], r["start"], r["radius"] = 3, o["target"], o["start"], o["size"]
            for k in ("max_vel", "max_acc", "gamma_target", "gamma_obs"):
                r[k] = o[k]
        elif o["type"] == "gaussian":
            hist = np.asarray(o["acc_history"], np.float64).reshape(-1, 3)
            r["kind"], r["n_acc"], r["acc_first"] = 4, o.get("n_acc", len(hist)), len(acc)
            r["start"], r["initial_vel"], r["max_vel"], r["cycle"] = o["start"], o["initial_vel"], o["max_vel"], o["acc_update_cycle"]
            acc += list(hist)
        else:
            r["model"] = models_of([o])[0]
            r["kind"] = r["model"]["kind"]
    return rec, np.asarray(acc, np.float64).reshape(-1, 3)


def _build(d, name, *flags):
    src, exe = d / "obstacle_reactive_host.cpp", d / name
    src.write_text(HOST_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", *flags, "-I", CSRC, str(src), "-o", str(exe)])
    return exe


def _run(d, exe, obstacles, times, agents):
    rec, acc = records_of(obstacles)
    fin, fout = d / "scene.bin", d / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.array((len(times), agents.shape[1], len(rec), len(acc)), HEAD).tobytes())
        f.write(rec.tobytes()); f.write(acc.tobytes())
        f.write(np.ascontiguousarray(times, np.float64).tobytes()); f.write(np.ascontiguousarray(agents, np.float32).tobytes())
    subprocess.check_call([str(exe), str(fin), str(fout)], timeout=60)
    out = np.fromfile(fout, OUT)
    assert len(out) == len(times) * len(rec)
    return out.reshape(len(times), len(rec))


@pytest.fixture(scope="module")
def host_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("obstacle_reactive")


@pytest.fixture(scope="module")
def host_exe(host_dir):
    return _build(host_dir, "obstacle_reactive_host")


def _reference(obstacles, times, agents):
    """ObstacleSet over the same steps -> (positions, velocities [steps][K][3], chaser states [steps][K][7], the set)."""
    s = ObstacleSet(obstacles, n_agents=agents.shape[1])
    pos, vel, st = [], [], []
    for t, a in zip(times, agents):
        s.at(t, a)
        pos.append(s.positions.copy()); vel.append(s.velocities.copy()); st.append(s.chaser_states())
    return np.stack(pos), np.stack(vel), np.stack(st), s


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ the scenario takes every branch
def test_the_pursuit_scenario_takes_every_branch_within_ten_ticks():
    """The GPU tests fly this scenario: here the reference's own statements count their branches over its first 10 ticks, the agents
    at rest at their starts (a flight's agents move; the branches below do not depend on where exactly they are)."""
    from pursuit_scenario import hover_mission
    ms = hover_mission()
    s = ObstacleSet(pursuit(), n_agents=ms.qn)
    assert s.has_chasers and s.reactive and len(s) == 5
    for j in range(1, 11):
        s.at(DT * j, ms.start)
        assert np.array_equal(_bits(s.positions[0]), _bits(s.positions[1])), j       # the twins stay coincident
    twin, lone = s.motions[0].counts, s.motions[2].counts
    assert twin["skipped"] == 9, twin                       # steps 2 .. 10: the other twin at dist < 1e-5 (step 1 sees the zero obstacles)
    assert lone["zero_first_step"] == 1 and twin["zero_first_step"] == 1
    assert lone["repulsion"] >= 4, lone                     # step 1: the four zero obstacles at 0.1 m < Q* = 0.3 m
    assert all(s.motions[k].counts["acc_clamp"] >= 1 and s.motions[k].counts["vel_clamp"] >= 1 for k in (0, 1, 2)), [s.motions[k].counts for k in (0, 1, 2)]
    # the first step was taken with dt > 0: the chaser moved
    assert s.motions[2].t_last == DT * 10 and s.motions[2].pos != s.motions[2].start


def test_a_chasers_first_step_is_against_zero_obstacles():
    """obstacle_generator.hpp:30, :108: before the first update the previous obstacles are default-constructed -- positions 0, radii 0.
    A chaser 0.1 m from the origin with radius 0.15 is pushed away from it (Q* = 0.3 m); with radius 0.04 (Q* = 0.08 m) it is not."""
    agents = np.zeros((2, 3), np.float32)
    moved = []
    for size in (0.15, 0.04):
        s = ObstacleSet([chaser([0.06, 0.08, 0.0], 0, size=size, gamma_target=0.0, gamma_obs=0.05), chaser([3.0, 3.0, 3.0], 1, size=size)], n_agents=2)
        s.at(0.2, agents)
        moved.append(s.motions[0].counts["repulsion"])
    assert moved == [1, 0], moved
    assert (s.positions[0] == [0.06, 0.08, 0.0]).all()      # gamma_target 0 and no repulsion: a = 0, it stays
    s.reset()
    assert s.motions[0].pos == [0.06, 0.08, 0.0] and s.motions[0].t_last == 0.0 and not s.positions.any()


def test_chasers_need_the_agents():
    s = ObstacleSet(pursuit(), n_agents=8)
    with pytest.raises(ValueError, match="agents"):
        s.at(0.2)
    with pytest.raises(ValueError, match="chases agent 3"):
        s.at(0.2, np.zeros((2, 3), np.float32))


# ------------------------------------------------------------------------------------------------ the walker's branches
def test_gaussian_branches():
    walker = pursuit()[3]
    s = ObstacleSet([walker])
    w = s.motions[0]
    assert len(w.acc) == 12 and w.cycle == 0.5
    # an exact multiple of the cycle: n = floor((1.5 + 1e-5) / 0.5) = 3, the last entry's dt = t - 3 x 0.5 = 0: it adds nothing
    assert w.entries(1.5) == 4 and w.entries(np.nextafter(1.5, 0.0)) == 4 and w.entries(1.5 - 2e-5) == 3
    s.at(1.5)
    at_multiple = s.positions[0].copy()
    s.at(1.5 - 2e-5)
    assert np.abs(at_multiple - s.positions[0]).max() < 1e-5 and (at_multiple != s.positions[0]).any()
    # both branches of the velocity cap over the table's ticks, and an entry that is ignored leaves the reported velocity alone
    w.counts.update(capped=0, applied=0)
    for j in range(1, 30):
        s.at(DT * j)
    assert w.counts["capped"] > 0 and w.counts["applied"] > 0, w.counts
    capped = dict(walker, acc_history=[[10.0, 0.0, 0.0]] * 3)
    sc = ObstacleSet([capped])
    pos, vel = sc.at(1.2)
    assert sc.motions[0].counts == dict(capped=3, applied=0)
    assert np.array_equal(vel[0], np.float32(walker["initial_vel"]))
    x = walker["start"][0]
    for dt in (0.5, 0.5, 1.2 - 2.0 * 0.5):                  # the position advances by v dt, entry after entry
        x += 0.1 * dt
    assert np.array_equal(_bits(sc.positions[0]), _bits([x, walker["start"][1], walker["start"][2]]))
    # the last admissible tick of the table: 12 entries serve floor((t + 1e-5) / 0.5) + 1 <= 12, t < 6 - 1e-5
    last = 6.0 - 2e-5
    assert w.entries(last) == 12 and w.entries(6.0) == 13
    s.at(last)
    with pytest.raises(ValueError, match="13 entries"):
        s.at(6.0)


def test_a_missing_history_is_drawn_from_the_seed():
    o = {k: v for k, v in pursuit()[3].items() if k != "acc_history"}
    a, b, c = ObstacleSet([o], seed=3), ObstacleSet([o], seed=3), ObstacleSet([o], seed=4)
    assert a.motions[0].acc.shape == (20, 3)                # ceil(10 / 0.5): update_acc_history(10)
    assert np.array_equal(a.motions[0].acc, b.motions[0].acc) and not np.array_equal(a.motions[0].acc, c.motions[0].acc)
    norms = np.linalg.norm(a.motions[0].acc, axis=1)
    assert (norms <= o["max_acc"] * (1 + 1e-12)).all()
    assert ObstacleSet([dict(o, acc_update_cycle=0)]).motions[0].cycle == 0.1      # src/mission.cpp:256-258


# ------------------------------------------------------------------------------------------------ host statements against ObstacleSet
def _scene():
    times = np.array([DT * j for j in range(1, STEPS + 1)], np.float64)
    obstacles = pursuit()
    obstacles[3] = dict(obstacles[3], acc_history=acc_table(25).tolist())       # 60 steps of 0.2 s: 12 s, 25 entries at cycle 0.5
    return obstacles, times, scripted_agents()


def _assert_host_equals_obstacleset(out, obstacles, times, agents):
    pos, vel, st, s = _reference(obstacles, times, agents)
    assert not out["code"].any()
    for name, ref in (("pos", pos), ("vel", vel), ("state", st)):
        differs = np.argwhere(_bits(out[name]) != _bits(ref))
        assert len(differs) == 0, (name, differs[:4], out[name][tuple(differs[0][:2])], ref[tuple(differs[0][:2])])
    return s


def test_host_statements_equal_obstacleset_bit_for_bit(host_dir, host_exe):
    obstacles, times, agents = _scene()
    out = _run(host_dir, host_exe, obstacles, times, agents)
    s = _assert_host_equals_obstacleset(out, obstacles, times, agents)
    # ... and the comparison saw every branch
    for k in (0, 1, 2):
        c = s.motions[k].counts
        assert c["acc_clamp"] and c["vel_clamp"] and c["zero_first_step"], (k, c)
    assert s.motions[2].counts["repulsion"] >= 4
    assert s.motions[0].counts["skipped"] == STEPS - 1
    assert s.motions[3].counts["capped"] and s.motions[3].counts["applied"]
    assert np.isnan(out["state"][:, 3:]).all() and np.isfinite(out["state"][:, :3]).all()


def test_host_statements_with_a_full_wave_of_chasers(host_dir, host_exe):
    from pursuit_scenario import full_wave
    times = np.array([DT * j for j in range(1, 6)])
    agents = scripted_agents(5, 4)
    out = _run(host_dir, host_exe, full_wave(), times, agents)
    s = _assert_host_equals_obstacleset(out, full_wave(), times, agents)
    assert all(mo.counts["repulsion"] == 4 * 63 for mo in s.motions), s.motions[0].counts       # steps 2 .. 5: every other chaser inside Q*


def test_host_program_under_the_sanitizers(host_dir):
    """The same stand-alone program with -fsanitize=address,undefined (host code only): the same bits, no report."""
    exe = _build(host_dir, "obstacle_reactive_host_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    obstacles, times, agents = _scene()
    _assert_host_equals_obstacleset(_run(host_dir, exe, obstacles, times, agents), obstacles, times, agents)


# ------------------------------------------------------------------------------------------------ refusals
NAN = float("nan")
BAD = [  # (obstacle, the code of csrc/lsc_obstacle_motion.hpp, words of both messages)
    (chaser([0.0, NAN, 0.0], 0), 3, "not finite"),
    (chaser([0.0, 0.0, 0.0], 0, gamma_obs=float("inf")), 3, "not finite"),
    (chaser([0.0, 0.0, 0.0], 0, max_vel=0.0), 7, "max_vel"),
    (chaser([0.0, 0.0, 0.0], 0, max_acc=0.01), 8, "max_acc"),
    (chaser([0.0, 0.0, 0.0], N_AGENTS), 9, "target"),
    (chaser([0.0, 0.0, 0.0], -1), 9, "target"),
    (dict(pursuit()[3], max_vel=-1.0), 7, "max_vel"),
    (dict(pursuit()[3], acc_update_cycle=-0.5), 10, "acc_update_cycle"),
    (dict(pursuit()[3], initial_vel=[0.0, NAN, 0.0]), 3, "not finite"),
    (dict(pursuit()[3], acc_history=[[0.0, 0.0, NAN]]), 3, "not finite"),
    (dict(pursuit()[3], acc_history=[]), 11, "entries"),
    (dict(pursuit()[3], acc_history=np.zeros((4097, 3)).tolist()), 11, "entries"),
]


def test_installation_refusals_by_message(host_dir, host_exe):
    text = subprocess.check_output([str(host_exe), "messages"], text=True)
    message = {int(line.split(":")[0]): line.split(": ", 1)[1] for line in text.splitlines()}
    assert message[7] == "max_vel is not positive" and message[9] == "the target is not an agent (0 .. N - 1)"
    assert message[8].startswith("max_acc is not above 0.01") and message[10] == "acc_update_cycle is not positive"
    assert message[11] == "the acceleration history has fewer than 1 or more than 4096 entries" and message[3] == "a value is not finite"
    assert message[1].startswith("unknown kind") and message[6].startswith("the patrol")      # (the closed forms' messages stand)
    for o, code, word in BAD:
        out = _run(host_dir, host_exe, [o], [0.2], scripted_agents(1))
        assert out["code"][0, 0] == code, (o["type"], word, out["code"])
        assert word in message[code], (word, message[code])
        with pytest.raises(ValueError, match=word):
            ObstacleSet([o], n_agents=N_AGENTS)
    # a good one of each passes both
    assert not _run(host_dir, host_exe, pursuit(), [0.2], scripted_agents(1))["code"].any()


@pytest.mark.parametrize("kind,keys", [("chasing", ("start", "size", "max_vel", "max_acc", "gamma_target", "gamma_obs")),
                                       ("gaussian", ("start", "initial_vel", "size", "max_vel"))])
def test_missing_keys_are_named(kind, keys):
    full = pursuit()[0 if kind == "chasing" else 3]
    for k in keys:
        with pytest.raises(ValueError, match=f"{kind}.*'{k}'"):
            ObstacleSet([{x: v for x, v in full.items() if x != k}], n_agents=N_AGENTS)
    if kind == "gaussian":                                  # without a history it needs what the draw needs
        for k in ("stddev_acc", "max_acc"):
            with pytest.raises(ValueError, match=f"gaussian.*'{k}'"):
                ObstacleSet([{x: v for x, v in full.items() if x not in ("acc_history", k)}])


def test_bernstein_and_static_stay_refused():
    from lsc_planner_amd.obstacles import SUPPORTED, UNSUPPORTED
    assert UNSUPPORTED == ("bernstein", "static") and "chasing" in SUPPORTED and "gaussian" in SUPPORTED
    for kind in UNSUPPORTED:
        with pytest.raises(ValueError, match=kind):
            ObstacleSet([{"type": kind, "size": 0.2}])
