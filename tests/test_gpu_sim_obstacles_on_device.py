"""-m gpu: lsc_sim --obstacles-on-device: the library moves the mission's obstacles itself (lsc_obstacle_motion / lsc_obstacle_clock), in the
per-tick loop and with --device-loop, where the obstacles' part of the accounting is replayed from the obstacle track.

CSVs are compared as text, cell for cell, except planning_time (column 15 q + 11 of agent q), the wall clock of that run's ticks.
"""
import csv
import json
import os
import re
import subprocess

import numpy as np
import pytest

from obstacle_reference import SIM_OBSTACLES, sim_mission_doc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "lsc_planner_amd", "lsc_sim")
# the two exact motions, beside the agents' ways (where SIM_OBSTACLES has its spin)
EXACT_OBSTACLES = [
    SIM_OBSTACLES[0],
    {"type": "multisim_patrol", "waypoints": [{"waypoint": [-1.0, -1.3, 1.0]}, {"waypoint": [-0.6, -1.3, 1.0]}, {"waypoint": [-0.6, -1.7, 1.1]}], "size": 0.25,
     "speed": 0.1, "max_acc": 1.0, "downwash": 0},
]
RUNS = {"plain": [], "flag": ["--obstacles-on-device"], "loop": ["--obstacles-on-device", "--device-loop", "5"]}


@pytest.fixture(scope="module")
def flights(tmp_path_factory):
    """(mission, run) -> (completed process, CSV rows): every flight of this file, flown once."""
    assert os.path.exists(SIM), "lsc_sim not built"
    out = {}
    for mission, obstacles, runs in (("exact", EXACT_OBSTACLES, ("plain", "flag", "loop")), ("spin", SIM_OBSTACLES, ("flag", "loop"))):
        for run in runs:
            d = tmp_path_factory.mktemp(f"{mission}_{run}")
            mp = d / "m.json"
            mp.write_text(json.dumps(sim_mission_doc(obstacles)))
            r = subprocess.run([SIM, "--mission", str(mp), "--csv", str(d), "--quiet", "--max-iter", "120", "--reset-threshold", "0"] + RUNS[run],
                               capture_output=True, text=True, timeout=120)
            f = d / "result_LSC_3agents.csv"
            out[mission, run] = (r, list(csv.reader(open(f))) if f.exists() else [], f)
            if r.returncode < 0 or r.returncode > 3:               # (killed or crashed: nothing more is started)
                return out
    return out


def _cells(rows, skip=lambda i: i < 45 and i % 15 == 11):
    return [[c for i, c in enumerate(row) if not skip(i)] for row in rows]


def test_every_flight_ends_with_status_0(flights):
    for key, (r, rows, _) in flights.items():
        assert r.returncode == 0, (key, r.stderr[-1500:])
        assert len(rows) > 20 and all(len(row) == 3 * 15 + 2 * 6 for row in rows[1:]), key


def test_flag_against_the_mission_without_it_as_text(flights):
    """--reset-threshold 0 --obstacles-on-device against the same mission without the flag: every cell as text, except planning_time.  The
    obstacles' cells included: without the flag lsc_sim prints the host's doubles with nine digits, with it the doubles the stage formed
    before it rounded them to float32 (lsc_obstacle_positions_read), which for straight and patrol are the host's bits."""
    a, b = flights["exact", "plain"][1], flights["exact", "flag"][1]
    differing = [(j, i, x, y) for j, (ra, rb) in enumerate(zip(_cells(a), _cells(b))) for i, (x, y) in enumerate(zip(ra, rb)) if x != y]
    print("cells that differ:", len(differing), differing[:6])
    assert len(a) == len(b) and not differing, (len(differing), differing[:6])
    assert len({tuple(row[45:]) for row in a[1:]}) > 20                # (the obstacles moved)


@pytest.mark.parametrize("mission", ["exact", "spin"])
def test_device_loop_writes_the_per_tick_loops_csv(flights, mission):
    """--obstacles-on-device against --obstacles-on-device --device-loop 5: identical, spin included (both print the device's doubles: the
    per-tick loop reads them behind its tick, the device loop from the track's rows)."""
    a, b = flights[mission, "flag"][1], flights[mission, "loop"][1]
    assert len(a) == len(b) and _cells(a) == _cells(b)


@pytest.mark.parametrize("mission", ["exact", "spin"])
def test_summaries_agree_on_the_obstacles(flights, mission):
    seen = []
    for run in ("flag", "loop"):
        out = flights[mission, run][0].stdout
        ratio = re.search(r"safety ratio between agent and obstacle: (\S+)", out)
        collided = re.search(r"collided: (\d)", out)
        assert ratio and collided, out[-800:]
        seen.append((ratio.group(1), collided.group(1), re.search(r"safety ratio between agent: (\S+)", out).group(1)))
    assert seen[0] == seen[1] and seen[0][1] == "0" and 1.0 < float(seen[0][0]) < 1e3, seen


def test_replay_reads_the_obstacles(flights):
    for run in ("flag", "loop"):
        rp = subprocess.run([SIM, "--replay", str(flights["exact", run][2])], capture_output=True, text=True, timeout=60)
        assert rp.returncode == 0 and "agents 3 obstacles 2" in rp.stdout, rp.stdout + rp.stderr
