"""The seeded inputs behind tests/golden/astar_ref_searches.npz and astar_ref_goal_cases.npz: one generator shared by the recorder
(tests/golden/make_astar_golden.py), tests/test_oracle_astar_ref.py and tests/test_gpu_goal_reference.py, so that the recorded
answers of the reference's Astar-3D provably belong to the inputs a test rebuilds (every grid and field carries a CRC-32).
No test in here; numpy only."""
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEARCHES = os.path.join(GOLDEN, "astar_ref_searches.npz")
GOAL_CASES = os.path.join(GOLDEN, "astar_ref_goal_cases.npz")

# ---------------------------------------------------------------------------------------------------------------- bare searches
N_RANDOM = 400                                   # the distribution of tests/test_goal_planning.py::_random_case, one seed per case
LARGE_SHAPES = [(34, 34, 9), (67, 67, 9), (133, 133, 9), (200, 200, 9), (140, 90, 1), (128, 100, 5), (3, 3, 1), (1, 40, 1), (40, 1, 3)]
LARGE_FILLS = [("empty", 0.0), ("dense", 0.1), ("dense", 0.25), ("dense", 0.35), ("blocky", 0.12), ("blocky", 0.2)]
HAND = ["start_is_goal", "goal_cell_occupied", "goal_column_free_at_another_altitude", "goal_column_blocked", "walled_in_start",
        "single_row", "single_column", "single_layer"]
N_MODEL_RANDOM = 80                              # tests/astar_model.py is pure Python: the first random cases, the hand-made ones and
MODEL_MAX_CELLS = 200                            # the grids of the shape list up to this many cells


def _blocks(rng, shape, density):
    coarse = rng.random(tuple(d // 3 + 1 for d in shape)) < density
    return np.kron(coarse, np.ones((3, 3, 3), bool))[:shape[0], :shape[1], :shape[2]]


def _hand(name):
    """(occ, start, goal) of an edge made by hand."""
    if name == "start_is_goal":
        occ = (np.random.default_rng(7).random((5, 5, 3)) < 0.2).astype(np.uint8)
        occ[2, 3, 1] = 0
        return occ, [2, 3, 1], [2, 3, 1]
    if name == "goal_cell_occupied":             # the goal test ignores the altitude (isearch.cpp:74): reached one layer off
        occ = np.zeros((9, 9, 3), np.uint8)
        occ[7, 6, 1] = 1
        return occ, [1, 1, 1], [7, 6, 1]
    if name == "goal_column_free_at_another_altitude":
        occ = np.zeros((9, 8, 4), np.uint8)
        occ[6, 5, :] = 1
        occ[6, 5, 3] = 0
        return occ, [0, 0, 0], [6, 5, 0]
    if name == "goal_column_blocked":
        occ = np.zeros((7, 7, 3), np.uint8)
        occ[5, 5, :] = 1
        return occ, [1, 1, 1], [5, 5, 1]
    if name == "walled_in_start":
        occ = np.zeros((7, 7, 5), np.uint8)
        for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            occ[3 + d[0], 3 + d[1], 2 + d[2]] = 1
        return occ, [3, 3, 2], [6, 6, 4]
    if name == "single_row":
        return np.zeros((1, 40, 1), np.uint8), [0, 3, 0], [0, 38, 0]
    if name == "single_column":
        return np.zeros((40, 1, 1), np.uint8), [37, 0, 0], [2, 0, 0]
    if name == "single_layer":
        occ = (np.random.default_rng(9).random((20, 20, 1)) < 0.2).astype(np.uint8)
        occ[1, 1, 0] = occ[18, 17, 0] = 0
        return occ, [1, 1, 0], [18, 17, 0]
    raise KeyError(name)


def search_specs():
    """[(kind, seed, shape or None, density or None)]: the whole case list, in fixture order."""
    specs = [("random", 1000 + t, None, None) for t in range(N_RANDOM)]
    t = 0
    for shape in LARGE_SHAPES:
        for fill, density in LARGE_FILLS:
            specs.append((fill, 2000 + t, shape, density))
            t += 1
    specs += [("hand:" + name, -1, None, None) for name in HAND]
    return specs


def search_case(spec):
    """dict(kind, seed, shape, density, occ uint8 [ni][nj][nk], start, goal, crc) of one spec."""
    kind, seed, shape, density = spec
    if kind.startswith("hand:"):
        occ, s, g = _hand(kind[5:])
        density = float(occ.mean())
    else:
        rng = np.random.default_rng(seed)
        if kind == "random":                     # _random_case: sides 3..35, 1..8 layers, one of four densities, the goal cell as it falls
            shape = (int(rng.integers(3, 36)), int(rng.integers(3, 36)), int(rng.integers(1, 9)))
            density = float(rng.choice([0.0, 0.1, 0.25, 0.35]))
        occ = (_blocks(rng, shape, density) if kind == "blocky" else rng.random(shape) < density).astype(np.uint8)
        s = [int(rng.integers(0, d)) for d in shape]
        g = [int(rng.integers(0, d)) for d in shape]
        occ[tuple(s)] = 0
        if kind != "random":
            occ[tuple(g)] = 0
    occ = np.ascontiguousarray(occ, np.uint8)
    head = np.asarray(list(occ.shape) + list(s) + list(g), np.int32)
    crc = zlib.crc32(occ.tobytes(), zlib.crc32(head.tobytes())) & 0xffffffff
    return dict(kind=kind, seed=seed, shape=tuple(occ.shape), density=density, occ=occ, start=s, goal=g, crc=crc)


def in_model_subset(index, case):
    k = case["kind"]
    if k == "random":
        return index < N_MODEL_RANDOM
    return k.startswith("hand:") or case["occ"].size <= MODEL_MAX_CELLS


def check_search_conditions(found, steps):
    """The conditions the case set has to meet (not measurements): recorder and test call this on the reference's answers."""
    found, steps = np.asarray(found, bool), np.asarray(steps)
    assert (~found).mean() <= 0.25, f"{(~found).mean():.3f} of the searches are unreachable"
    assert (steps >= 1000).sum() >= 10, (steps >= 1000).sum()
    assert (steps > 500).sum() >= 5, (steps > 500).sum()         # a row of such a search goes through rehashes


def load_searches():
    z = np.load(SEARCHES)
    meta = json.loads(str(z["meta"]))
    off = z["path_off"]
    paths = [z["path_cells"][off[t]:off[t + 1]].astype(np.int32) for t in range(len(off) - 1)]
    return z, meta, paths


# ------------------------------------------------------------------------------------------------------------ goal-stage cases
N_AGENTS = 12
FIELD_RES = 0.1
GRID_MARGIN, MIN_CLEARANCE = 0.05, 0.5
SMALL, WIDE, TALL = (-4, -4, 0, 4, 4, 2), (-10, -10, 0, 10, 10, 2), (-20, -4, 0, 20, 4, 2)
# name: world box, block density, world dimension (z_2d), segments M (dt, horizon), path capacity of the trace, planner_seq of the tick
GOAL_SPECS = {
    "small_0": dict(world=SMALL, density=0.12),
    "small_1": dict(world=SMALL, density=0.17),
    "small_2": dict(world=SMALL, density=0.22),
    "wide":    dict(world=WIDE, density=0.17),                     # rows of more than 64 cells: two bookkeeping slots per lane, rehashes
    "tall":    dict(world=TALL, density=0.17),                     # more than 128 rows: no register-resident search
    "planar":  dict(world=WIDE, density=0.12, dim=2, z2d=1.0),     # one layer: ties everywhere
    "m4":      dict(world=SMALL, density=0.17, M=4, dt=0.5, horizon=2.0, planner_seq=2),   # the LOS goal reads the last of 4 segments
}
BATCH = ("small_0", "small_1", "small_2")                          # one replan_tick_batch launch of these three
GOAL_DEFAULTS = dict(dim=3, z2d=1.0, M=5, dt=0.2, horizon=1.0, planner_seq=1, path_cap=1024)
EXPECTED_GRID = {"small_0": (27, 27, 7), "small_1": (27, 27, 7), "small_2": (27, 27, 7), "wide": (67, 67, 7), "tall": (133, 27, 7),
                 "planar": (67, 67, 1), "m4": (27, 27, 7)}


def goal_spec(name):
    return dict(GOAL_DEFAULTS, **GOAL_SPECS[name])


def maze_field(world, density, seed, planar=False):
    """'Distance field' of a maze: 0 inside random blocks of 3 x 3 x 3 field cells (columns of 3 x 3 in a planar world), 1 m
    elsewhere.  Returns (dist float32 [nx][ny][nz], key_min int32 [3], crc)."""
    rng = np.random.default_rng(seed)
    kmin = np.array([np.floor(world[k] / FIELD_RES) + 32768 for k in range(3)], np.int32)
    dims = [int(np.floor(world[3 + k] / FIELD_RES) + 32768 - kmin[k] + 1) for k in range(3)]
    if planar:
        coarse = rng.random((dims[0] // 3 + 1, dims[1] // 3 + 1)) < density
        blocked = np.repeat(np.kron(coarse, np.ones((3, 3), bool))[:dims[0], :dims[1], None], dims[2], axis=2)
    else:
        coarse = rng.random((dims[0] // 3 + 1, dims[1] // 3 + 1, dims[2] // 3 + 1)) < density
        blocked = np.kron(coarse, np.ones((3, 3, 3), bool))[:dims[0], :dims[1], :dims[2]]
    dist = np.ascontiguousarray(np.where(blocked, 0.0, 1.0), np.float32)
    return dist, kmin, zlib.crc32(dist.tobytes()) & 0xffffffff


def goal_inputs(L, name, field_seed, swarm_seed):
    """The tick a goal case plans: (spec, mission, dist, key_min, crc, state [n][9], prev_traj [n][3][6 M]).  L: lsc_planner_amd."""
    sp = goal_spec(name)
    dist, kmin, crc = maze_field(sp["world"], sp["density"], field_seed, planar=sp["dim"] == 2)
    ms = L.random_swarm(N_AGENTS, world=sp["world"], seed=swarm_seed, edt=dist, edt_key_min=kmin, min_clearance=MIN_CLEARANCE)
    if sp["dim"] == 2:
        ms.start[:, 2] = ms.goal[:, 2] = np.float32(sp["z2d"])      # what Mission::initialize does with world/dimension = 2
    state = np.zeros((N_AGENTS, 9), np.float32)
    state[:, :3] = ms.start
    segv = 6 * sp["M"]
    traj = np.zeros((N_AGENTS, 3, segv), np.float32)
    if sp["planner_seq"] >= 2:
        # a previous plan to read: every agent drifting at a seeded velocity, its previous trajectory that constant-velocity motion
        # (Bernstein control points of segment m: pos + vel * (m + i / 5) * dt, in float32)
        rng = np.random.default_rng(swarm_seed + 1)
        state[:, 3:6] = rng.uniform(-0.3, 0.3, (N_AGENTS, 3)).astype(np.float32)
        t = (np.arange(sp["M"], dtype=np.float32)[:, None] + np.arange(6, dtype=np.float32)[None, :] / np.float32(5)).reshape(-1)
        t = t * np.float32(sp["dt"])
        traj = (state[:, :3, None] + state[:, 3:6, None] * t[None, None, :]).astype(np.float32)
    return sp, ms, dist, kmin, crc, state, traj


def check_goal_conditions(cases):
    """cases: {name: dict(flags, path_len, path_cap)} -- the conditions on the goal-stage case set."""
    second = 0
    for name, c in cases.items():
        flags, plen = np.asarray(c["flags"]), np.asarray(c["path_len"])
        ran = ((flags & 1) == 0) & (plen > 0)
        assert ran.sum() >= 8, (name, int(ran.sum()))
        assert int(c["path_cap"]) > int(plen.max()), (name, int(plen.max()))
        second += int(((flags & 2) != 0).sum())
    assert second >= 1, "no agent needed the second, unprioritised attempt"


def load_goal_cases():
    z = np.load(GOAL_CASES)
    meta = json.loads(str(z["meta"]))
    out = {}
    for name in meta["cases"]:
        g = lambda k: z[f"{name}/{k}"]
        off = g("path_off")
        out[name] = dict(field_seed=int(g("field_seed")), swarm_seed=int(g("swarm_seed")), field_crc=int(g("field_crc")),
                         grid_dims=tuple(int(v) for v in g("grid_dims")), path_cap=int(g("path_cap")), state=g("state"), goal=g("goal"),
                         traj=g("traj"), flags=g("flags"), steps=g("steps"), goals_out=g("goals_out"), path_len=np.diff(off),
                         paths=[g("path_cells")[off[q]:off[q + 1]].astype(np.int32) for q in range(len(off) - 1)])
    return meta, out
