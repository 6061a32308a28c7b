"""lsc_sim's mission / world lists without a GPU (`--list-missions` stops before any GPU call): `--world DIR` scans every *.bt in name
order like `--mission-dir` scans missions, pairs world i with mission i when the counts agree and otherwise gives every mission the first
world with one warning (the reference's node: src/multi_sync_simulator_node.cpp:45-53, lists built by src/param.cpp:104-139)."""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

SIM = os.path.join(ROOT, "lsc_planner_amd", "lsc_sim")


@pytest.fixture(scope="module")
def forest_missions():
    return json.load(open(os.path.join(GOLDEN, "testall_missions_20agents.json")))["forest"]


def _write(tmp_path, forest_missions, idx, worlds):
    md, wd = tmp_path / "missions", tmp_path / "worlds"
    md.mkdir()
    wd.mkdir()
    for i in idx:
        name = f"multi_random_20agents_{i}.json"
        (md / name).write_text(forest_missions[name])
    for w in worlds:
        (wd / w).write_bytes(b"")            # (listed only: --list-missions reads no map)
    return str(md), str(wd)


def _list(md, wd):
    assert os.path.exists(SIM), "lsc_sim not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([SIM, "--mission-dir", md, "--world", wd, "--list-missions"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return [tuple(os.path.basename(x) for x in line.split()) for line in r.stdout.splitlines()], r.stderr


def test_world_directory_pairs_with_the_mission_list_by_index(tmp_path, forest_missions):
    """The reference's names sort as 1, 10, 2 in both lists ('.' sorts before '0'), so index pairing matches forest i with mission i."""
    md, wd = _write(tmp_path, forest_missions, (1, 10, 2), ("forest1.bt", "forest10.bt", "forest2.bt", "notes.txt"))
    pairs, err = _list(md, wd)
    assert pairs == [("multi_random_20agents_1.json", "forest1.bt"), ("multi_random_20agents_10.json", "forest10.bt"),
                     ("multi_random_20agents_2.json", "forest2.bt")]
    assert "not match" not in err


def test_world_count_mismatch_gives_the_first_world_and_one_warning(tmp_path, forest_missions):
    md, wd = _write(tmp_path, forest_missions, (1, 10, 2), ("office.bt", "zz_other.bt"))
    pairs, err = _list(md, wd)
    assert pairs == [(m, "office.bt") for m in ("multi_random_20agents_1.json", "multi_random_20agents_10.json", "multi_random_20agents_2.json")]
    assert err.count("The number of world file is not match to the number of mission file, use") == 1
    assert err.rstrip().endswith("office.bt")
