"""The reference's own Astar-3D (oracle/_ref/libref_astar.so) on the seeded cases of tests/astar_ref_cases.py, stored so that the tests
hold the oracle, tests/astar_model.py and the kernels to the reference's answers where oracle/_ref has not been built.

Needs oracle/_ref (make -C oracle ref REF=<reference checkout>):  python tests/golden/make_astar_golden.py

  astar_ref_searches.npz    bare searches (AstarPlanner::plan): per case shape, seed, density, start, goal, grid CRC-32, verdict,
                            numberofsteps and the path (int16 cells); in the metadata the number of model cases whose path changes
                            under a deliberately wrong bucket rule (front insertion).
  astar_ref_goal_cases.npz  goal-stage ticks of 12 agents in seeded mazes, planned by oracle.goal_prior_based_map INSIDE
                            oracle.reference_astar() (the reference's search in the loop): inputs, and per agent flags, path, summed
                            steps and goal.  Seeds are searched upwards from the base seeds below until the conditions of
                            astar_ref_cases.check_goal_conditions hold.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle import oracle as O  # noqa: E402
import astar_model  # noqa: E402
import astar_ref_cases as C  # noqa: E402

GOAL_BASE_SEEDS = {"small_0": 100, "small_1": 101, "small_2": 102, "wide": 200, "tall": 300, "planar": 400, "m4": 500}
NEEDS_SECOND_ATTEMPT = "small_2"        # this case's seed is searched until one of its agents takes the unprioritised search


def record_searches():
    specs = C.search_specs()
    n = len(specs)
    shape = np.zeros((n, 3), np.int16); seed = np.zeros(n, np.int32); density = np.zeros(n)
    start = np.zeros((n, 3), np.int16); goal = np.zeros((n, 3), np.int16); crc = np.zeros(n, np.uint32)
    found = np.zeros(n, bool); steps = np.zeros(n, np.int32); off = np.zeros(n + 1, np.int32)
    kinds, cells, model, front_diffs = [], [], np.zeros(n, bool), 0
    orig = astar_model.Row._place
    for t, spec in enumerate(specs):
        c = C.search_case(spec)
        path, st = O.ref_astar(c["occ"], c["start"], c["goal"])
        kinds.append(c["kind"])
        shape[t], seed[t], density[t], start[t], goal[t], crc[t] = c["shape"], c["seed"], c["density"], c["start"], c["goal"], c["crc"]
        found[t], steps[t], off[t + 1] = len(path) > 0, st, off[t] + len(path)
        cells.append(path.astype(np.int16))
        model[t] = C.in_model_subset(t, c)
        if model[t]:
            astar_model.Row._place = lambda self, lst, nb, e: lst.insert(0, e)
            try:
                got, _ = astar_model.astar(c["occ"], c["start"], c["goal"])
            finally:
                astar_model.Row._place = orig
            front_diffs += not (got.shape == path.shape and np.array_equal(got, path))
    C.check_search_conditions(found, steps)
    assert front_diffs > 0, "the model cases do not tell the bucket rule from front insertion"
    meta = dict(cases=n, model_cases=int(model.sum()), front_insertion_diffs=int(front_diffs), unreachable=int((~found).sum()),
                steps_1000=int((steps >= 1000).sum()), steps_500=int((steps > 500).sum()))
    np.savez_compressed(C.SEARCHES, kind=np.asarray(kinds), shape=shape, seed=seed, density=density, start=start, goal=goal, crc=crc,
                        found=found, steps=steps, path_off=off, path_cells=np.concatenate(cells).reshape(-1, 3), model=model,
                        meta=np.asarray(json.dumps(meta)))
    print("searches:", meta, os.path.getsize(C.SEARCHES), "bytes")


def plan_case(L, name, field_seed, swarm_seed):
    sp, ms, dist, kmin, fcrc, state, traj = C.goal_inputs(L, name, field_seed, swarm_seed)
    with O.segments(sp["M"]):
        dm = O.DistMap.from_array(dist, kmin, C.FIELD_RES)
        prm = O.make_params(dt=sp["dt"], world_min=ms.world_min, world_max=ms.world_max, obs_f32=True, world_dimension=sp["dim"],
                            world_z_2d=sp["z2d"])
        dims, _ = O.grid_dims(prm)
        assert tuple(int(v) for v in dims) == C.EXPECTED_GRID[name], (name, dims)
        kw = dict(grid_margin=C.GRID_MARGIN, want_paths=True, want_expansions=True)
        with O.reference_astar():
            goals, paths, flags, steps = O.goal_prior_based_map(prm, dm, state, ms.goal, traj, sp["planner_seq"], ms.radius, ms.downwash, **kw)
        own = O.goal_prior_based_map(prm, dm, state, ms.goal, traj, sp["planner_seq"], ms.radius, ms.downwash, **kw)
    # (the oracle's own search on the same tick: a difference here is the oracle's bug, to be fixed before anything is recorded)
    assert np.array_equal(own[0], goals) and np.array_equal(own[2], flags) and np.array_equal(own[3], steps), name
    assert all(np.array_equal(a, b) for a, b in zip(own[1], paths)), name
    return dict(sp=sp, ms=ms, fcrc=fcrc, dims=dims, state=state, traj=traj, goals=goals, paths=paths, flags=flags, steps=steps,
                path_len=np.asarray([len(p) for p in paths]), path_cap=sp["path_cap"], field_seed=field_seed, swarm_seed=swarm_seed)


def record_goal_cases():
    import lsc_planner_amd as L
    done = {}
    for name in C.GOAL_SPECS:
        for bump in range(200):
            fs, ss = GOAL_BASE_SEEDS[name] + 1000 * bump, GOAL_BASE_SEEDS[name] + 1000 * bump + 50
            try:
                r = plan_case(L, name, fs, ss)
            except ValueError:                         # random_swarm could not place the agents in this maze
                continue
            ran = ((r["flags"] & 1) == 0) & (r["path_len"] > 0)
            if ran.sum() < 8 or r["path_len"].max() >= r["path_cap"]:
                continue
            if name == NEEDS_SECOND_ATTEMPT and not (r["flags"] & 2).any():
                continue
            done[name] = r
            break
        else:
            raise SystemExit(f"no seed found for goal case {name}")
    C.check_goal_conditions(done)
    out = {}
    for name, r in done.items():
        off = np.concatenate([[0], np.cumsum(r["path_len"])]).astype(np.int32)
        cells = np.concatenate([p.reshape(-1, 3) for p in r["paths"]]).astype(np.int16)
        for k, v in dict(field_seed=r["field_seed"], swarm_seed=r["swarm_seed"], field_crc=np.uint32(r["fcrc"]), grid_dims=r["dims"],
                         path_cap=r["path_cap"], state=r["state"], goal=r["ms"].goal.astype(np.float32), traj=r["traj"],
                         flags=r["flags"].astype(np.int32), steps=r["steps"].astype(np.int32), goals_out=r["goals"], path_off=off,
                         path_cells=cells).items():
            out[f"{name}/{k}"] = np.asarray(v)
    meta = dict(cases=list(done), second_attempts={n: int(((r["flags"] & 2) != 0).sum()) for n, r in done.items()},
                longest_path={n: int(r["path_len"].max()) for n, r in done.items()},
                most_steps={n: int(r["steps"].max()) for n, r in done.items()})
    np.savez_compressed(C.GOAL_CASES, meta=np.asarray(json.dumps(meta)), **out)
    print("goal cases:", meta, os.path.getsize(C.GOAL_CASES), "bytes")


def main():
    if O.ref_astar_lib() is None:
        raise SystemExit("oracle/_ref/libref_astar.so missing: run `make -C oracle ref` with the reference checkout")
    record_searches()
    record_goal_cases()
    for f in (C.SEARCHES, C.GOAL_CASES):
        assert os.path.getsize(f) < 268 * 1024, (f, os.path.getsize(f))     # no fixture larger than the largest one there (gjk_vectors.npz)


if __name__ == "__main__":
    main()
