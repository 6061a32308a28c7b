"""-m gpu: lsc_sim flying a mission list on a list of worlds, back to back (--concurrent 1) and in lockstep (--concurrent 4: one batched
tick, lsc_replan_tick_batch, for every mission in flight).  Every mission must fly the same: the summary's flight time, distance,
collision flag and safety ratio, and the per-swarm-size result CSV (all but its timing column) are those of the back-to-back run, and
the world_file_name column names the paired world."""
import csv
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
SIM = os.path.join(ROOT, "lsc_planner_amd", "lsc_sim")
COLS = ("total_flight_time", "total_flight_distance", "is_collided", "safety_ratio_agent", "mission_file_name", "world_file_name")


def _lay_out(tmp_path, kind, idx, worlds):
    missions = json.load(open(os.path.join(GOLDEN, "testall_missions_20agents.json")))[kind]
    maps = np.load(os.path.join(GOLDEN, "reference_maps.npz"))
    md, wd = tmp_path / "missions", tmp_path / "worlds"
    md.mkdir()
    wd.mkdir()
    for i in idx:
        (md / f"multi_random_20agents_{i}.json").write_text(missions[f"multi_random_20agents_{i}.json"])
    for key in worlds:
        (wd / os.path.basename(key)).write_bytes(maps[key].tobytes())
    return str(md), str(wd)


def _fly(md, wd, out, k):
    os.makedirs(out)
    r = subprocess.run([SIM, "--mission-dir", md, "--world", wd, "--concurrent", str(k), "--csv", out, "--quiet", "--max-iter", "200"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-2000:]
    with open(os.path.join(out, "summary_LSC_20agents.csv")) as f:
        rows = [{c: row[c] for c in COLS} for row in csv.DictReader(f)]
    with open(os.path.join(out, "result_LSC_20agents.csv")) as f:
        result = [[v for j, v in enumerate(line.rstrip("\n").split(",")) if j % 15 != 11] for line in f]     # (planning_time: wall clock)
    return rows, result, r.stderr


def _check(tmp_path, kind, idx, worlds, expect_world):
    assert os.path.exists(SIM), "lsc_sim not built (python -c 'import __graft_entry__ as g; g.build()')"
    md, wd = _lay_out(tmp_path, kind, idx, worlds)
    one, res1, _ = _fly(md, wd, str(tmp_path / "k1"), 1)
    four, res4, err4 = _fly(md, wd, str(tmp_path / "k4"), 4)
    assert len(one) == len(idx)
    assert one == four
    assert res1 == res4
    names = sorted(f"multi_random_20agents_{i}.json" for i in idx)
    assert [os.path.basename(r["mission_file_name"]) for r in four] == names
    assert [os.path.basename(r["world_file_name"]) for r in four] == [expect_world(m) for m in names]
    return err4


def test_forest_list_on_its_own_worlds_concurrent_equals_back_to_back(tmp_path):
    idx = (1, 10, 2, 3)
    _check(tmp_path, "forest", idx, [f"forest/forest{i}.bt" for i in idx],
           lambda m: "forest" + m[len("multi_random_20agents_"):-len(".json")] + ".bt")


def test_office_list_on_one_world_concurrent_equals_back_to_back(tmp_path):
    err = _check(tmp_path, "office", (1, 2, 3), ["office.bt"], lambda m: "office.bt")
    assert err.count("The number of world file is not match") == 1
