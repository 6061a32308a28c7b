"""-m gpu: the goal kernels against the REFERENCE's own Astar-3D build, through recorded answers.  tests/golden/astar_ref_goal_cases.npz
holds one tick of 12 agents per case, planned by the oracle's goal stage with the reference's search in the loop
(oracle.reference_astar(), tests/golden/make_astar_golden.py); here the kernel's flags, grid paths (cell for cell, wherever the retreat
rule did not fire), expansion counts and goals must be the recorded ones, bit for bit, under every goal_search that admits the grid.
Nothing in here reads the reference or oracle/_ref: inputs are rebuilt from their seeds and checksummed against the fixture.

Expansion counts: the kernel's `expansions` is compared with the reference's SearchResult::numberofsteps summed over the agent's one
or two searches, as it is: both count one per pop, the pop of the goal cell included (src/Astar-3D/isearch.cpp:68-71; lsc_goal.hip,
top of the pop loops of search_fast and general_search), and lsc_goal_kernel adds every attempt to the agent's count.  No convention
is applied between the two."""
import numpy as np
import pytest

import astar_ref_cases as C

pytestmark = pytest.mark.gpu

SEARCHES = ("general", "auto", "key64", "hbm")


def _admits(search, grid):
    """The register-resident searches ("auto", "key64") keep one or two rows per lane: grids of more than 128 rows are not theirs
    (goal_fast_slots, lsc_goal.hip) -- a context asked for them there runs the general search, which this test already runs by name."""
    return grid[0] <= 128 or search in ("general", "hbm")


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


@pytest.fixture(scope="module")
def recorded():
    meta, cases = C.load_goal_cases()
    assert list(cases) == list(C.GOAL_SPECS)
    C.check_goal_conditions(cases)          # >= 8 of 12 agents searched in every case, a second attempt somewhere, paths below path_cap
    return cases


def _inputs(L, name, c):
    sp, ms, dist, kmin, crc, state, traj = C.goal_inputs(L, name, c["field_seed"], c["swarm_seed"])
    assert crc == c["field_crc"], name                             # the recorded answers are for exactly this field and this tick
    assert np.array_equal(state, c["state"]) and np.array_equal(traj, c["traj"]) and np.array_equal(ms.goal.astype(np.float32), c["goal"]), name
    return sp, ms, dist, kmin, state, traj


def _planner(L, sp, ms, dist, kmin, search, path_cap=0):
    extra = dict(world_dimension=2, world_z_2d=sp["z2d"]) if sp["dim"] == 2 else {}
    pl = L.SwarmPlanner(ms, L.PlannerConfig(use_octomap=True, goal_mode="prior_based", grid_margin=C.GRID_MARGIN, goal_search=search,
                                            dt=sp["dt"], horizon=sp["horizon"], **extra))
    pl.set_distmap(dist, kmin, C.FIELD_RES)
    if path_cap:
        pl.set_goal_trace(path_cap)
    assert pl.M == sp["M"]
    return pl


def _assert_recorded(name, search, c, pl, status, paths=True):
    tr = pl.goal_trace()
    what = (name, search)
    assert tuple(int(v) for v in tr["grid_dims"]) == c["grid_dims"] == C.EXPECTED_GRID[name], what
    assert (status != 5).all(), (what, "goal planner capacity", np.nonzero(status == 5))
    where = pl.goal_storage()                                      # 0 rows in LDS, 1 an LDS search restarted in HBM, 2 the HBM search
    assert (where == 2).all() if search == "hbm" else (where != 2).all(), (what, where)
    assert np.array_equal(pl.last_goals().view(np.uint32), c["goals_out"].view(np.uint32)), what
    assert np.array_equal(tr["flags"], c["flags"]), (what, tr["flags"], c["flags"])
    for q in range(C.N_AGENTS if paths else 0):
        if not (c["flags"][q] & 1):
            assert tr["path_len"][q] == len(c["paths"][q]), (what, q, tr["path_len"][q], len(c["paths"][q]))
            assert np.array_equal(tr["paths"][q], c["paths"][q]), (what, q)
    assert np.array_equal(tr["expansions"], c["steps"]), (what, tr["expansions"], c["steps"])


@pytest.mark.parametrize("name", list(C.GOAL_SPECS))
def test_kernel_against_the_recorded_reference(L, recorded, name):
    """One recorded tick per case -- 3-D mazes of three densities (27 x 27 x 7), rows wider than 64 cells (67 x 67 x 7), more than 128
    rows (133 x 27 x 7: the general and the HBM search only), a planar maze (67 x 67 x 1), the M = 4 build -- under every admissible search."""
    c = recorded[name]
    sp, ms, dist, kmin, state, traj = _inputs(L, name, c)
    ran = [s for s in SEARCHES if _admits(s, c["grid_dims"])]
    assert ran == (["general", "hbm"] if name == "tall" else list(SEARCHES)), ran
    for search in ran:
        pl = _planner(L, sp, ms, dist, kmin, search, c["path_cap"])
        try:
            pl.planner_seq = sp["planner_seq"] - 1                  # plan() counts the tick up first
            g = pl.plan(state, ms.goal, traj)
            _assert_recorded(name, search, c, pl, g["status"])
        finally:
            pl.close()


@pytest.mark.parametrize("search", SEARCHES)
def test_batch_launch_against_the_recorded_reference(L, recorded, search):
    """The three small mazes as one replan_tick_batch (one goal launch for the three contexts): the same recorded answers -- goals, flags
    and expansion counts.  The goal batch records no paths (lsc_replan_tick_batch refuses a context with a path trace on), so the cells
    themselves are compared in the single launches above; a path that differed would show here in its goal and its expansion count."""
    pls, states, goals, trajs = [], [], [], []
    try:
        for name in C.BATCH:
            c = recorded[name]
            sp, ms, dist, kmin, state, traj = _inputs(L, name, c)
            pls.append(_planner(L, sp, ms, dist, kmin, search))
            states.append(state); goals.append(ms.goal); trajs.append(traj)
        for pl in pls:
            pl.planner_seq += 1
        outs = L.replan_tick_batch(pls, states, goals, trajs, [pl.planner_seq for pl in pls])
        for name, pl, o in zip(C.BATCH, pls, outs):
            _assert_recorded(name, search, recorded[name], pl, o[2], paths=False)
    finally:
        for pl in pls:
            pl.close()
