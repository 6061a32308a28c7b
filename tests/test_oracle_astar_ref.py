"""CPU: the oracle's grid search (oracle/lsc_oracle_goal.cpp) and tests/astar_model.py -- the model the kernels implement -- against the
REFERENCE's own Astar-3D build (oracle/Makefile ref -> oracle/_ref/libref_astar.so): verdict, path cell for cell, and the oracle's
expansion count against SearchResult::numberofsteps.  Live where oracle/_ref was built (it is kept out of git and does not travel);
everywhere against that build's answers on the same seeded grids, stored in tests/golden/astar_ref_searches.npz
(tests/golden/make_astar_golden.py).  Every grid is rebuilt from its seed and its CRC-32 asserted first, so the stored answers belong
to exactly these inputs.  All comparisons are integer or bit exact."""
import numpy as np
import pytest

import astar_model
import astar_ref_cases as C


@pytest.fixture(scope="module")
def searches():
    """(fixture arrays, metadata, recorded paths, the rebuilt cases) -- inputs checked against their recorded checksums."""
    z, meta, paths = C.load_searches()
    specs = C.search_specs()
    assert len(specs) == meta["cases"] == len(paths) == len(z["crc"])
    cases = [C.search_case(s) for s in specs]
    for t, c in enumerate(cases):
        assert c["crc"] == int(z["crc"][t]) and c["kind"] == str(z["kind"][t]) and c["seed"] == int(z["seed"][t]), (t, c["kind"])
        assert c["shape"] == tuple(z["shape"][t]) and c["start"] == list(z["start"][t]) and c["goal"] == list(z["goal"][t]), t
        assert c["density"] == z["density"][t], t
        assert bool(z["found"][t]) == (len(paths[t]) > 0), t
    return z, meta, paths, cases


def test_the_case_set_meets_its_conditions(searches):
    """Conditions, not measurements: at most a quarter of the searches unreachable, at least 10 of 1000 or more steps, at least 5 across a
    rehash; every shape of the list and every hand-made edge is there."""
    z, meta, paths, cases = searches
    C.check_search_conditions(z["found"], z["steps"])
    assert meta["unreachable"] == int((~z["found"]).sum()) and meta["steps_1000"] == int((z["steps"] >= 1000).sum())
    kinds = [c["kind"] for c in cases]
    assert kinds.count("random") == 400
    for shape in C.LARGE_SHAPES:
        assert sum(c["shape"] == shape and c["kind"] in ("empty", "dense", "blocky") for c in cases) == 6, shape
    assert {k[5:] for k in kinds if k.startswith("hand:")} == set(C.HAND)
    by = {c["kind"]: t for t, c in enumerate(cases)}
    # the edges say what they are meant to say
    assert len(paths[by["hand:start_is_goal"]]) == 1 and z["steps"][by["hand:start_is_goal"]] == 1
    t = by["hand:goal_cell_occupied"]
    assert z["found"][t] and paths[t][-1][2] != cases[t]["goal"][2]                    # reached one layer off (isearch.cpp:74)
    t = by["hand:goal_column_free_at_another_altitude"]
    assert z["found"][t] and tuple(paths[t][-1]) == (6, 5, 3)
    assert not z["found"][by["hand:goal_column_blocked"]]
    assert not z["found"][by["hand:walled_in_start"]] and z["steps"][by["hand:walled_in_start"]] == 1


def test_oracle_search_equals_the_reference(oracle, searches):
    """orc_astar on every case: the reference's verdict, path and step count -- the recorded ones, and where oracle/_ref is built also
    the live ones, which must equal the recorded ones."""
    z, meta, paths, cases = searches
    live = oracle.ref_astar_lib() is not None
    for t, c in enumerate(cases):
        got = oracle.astar(c["occ"], c["start"], c["goal"])
        steps = oracle.astar_last_expansions()
        assert got.shape == paths[t].shape and np.array_equal(got, paths[t]), (t, c["kind"], c["shape"], len(got), len(paths[t]))
        assert steps == int(z["steps"][t]), (t, c["kind"], c["shape"], steps, int(z["steps"][t]))
        if live:
            rp, rs = oracle.ref_astar(c["occ"], c["start"], c["goal"])
            assert rp.shape == paths[t].shape and np.array_equal(rp, paths[t]) and rs == int(z["steps"][t]), (t, c["kind"], c["shape"])


def test_the_search_hook_delegates_and_comes_off(oracle):
    """orc_set_astar_hook: while a hook is set the oracle's search IS the hook -- it is handed the same grid, start and goal and its
    path and step count come back --, and with NULL the oracle's own search is back.  (A hook of this test's own, so that the call is
    told apart from the oracle's search; reference_astar() installs the reference build the same way, in both segment builds.)"""
    import ctypes
    ip = ctypes.POINTER(ctypes.c_int)
    HOOK = ctypes.CFUNCTYPE(ctypes.c_int, ip, ctypes.c_int, ctypes.c_int, ctypes.c_int, ip, ip, ip, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong))
    c = C.search_case(("dense", 77, (20, 21, 4), 0.2))
    seen = {}

    def fake(grid, ni, nj, nk, s, g, out, max_len, steps):
        seen.update(occ=np.ctypeslib.as_array(grid, shape=(ni, nj, nk)).copy(), s=[s[0], s[1], s[2]], g=[g[0], g[1], g[2]], max_len=max_len)
        for k in range(3):
            out[k], out[3 + k] = s[k], g[k]
        steps[0] = 42
        return 2
    cb = HOOK(fake)
    own, own_steps = oracle.astar(c["occ"], c["start"], c["goal"]), oracle.astar_last_expansions()
    assert len(own) > 5 and own_steps > len(own)
    oracle.lib().orc_set_astar_hook(ctypes.cast(cb, ctypes.c_void_p))
    try:
        got, steps = oracle.astar(c["occ"], c["start"], c["goal"]), oracle.astar_last_expansions()
    finally:
        oracle.lib().orc_set_astar_hook(None)
    assert got.tolist() == [c["start"], c["goal"]] and steps == 42
    assert np.array_equal(seen["occ"], c["occ"]) and seen["s"] == c["start"] and seen["g"] == c["goal"] and seen["max_len"] >= c["occ"].size
    after = oracle.astar(c["occ"], c["start"], c["goal"])
    assert np.array_equal(after, own) and oracle.astar_last_expansions() == own_steps
    if oracle.ref_astar_lib() is not None:
        rp, rs = oracle.ref_astar(c["occ"], c["start"], c["goal"])
        with oracle.reference_astar():
            for m in (5, 4):
                with oracle.segments(m):
                    assert np.array_equal(oracle.astar(c["occ"], c["start"], c["goal"]), rp) and oracle.astar_last_expansions() == rs
        assert np.array_equal(rp, own) and rs == own_steps


def _model_paths(cases, idx):
    return [astar_model.astar(cases[t]["occ"], cases[t]["start"], cases[t]["goal"]) for t in idx]


def test_kernel_model_equals_the_reference(searches):
    """tests/astar_model.py (explicit bucket lists; what lsc_goal.hip implements) on the small cases: the reference's recorded verdict,
    path and step count."""
    z, meta, paths, cases = searches
    idx = np.nonzero(z["model"])[0]
    assert len(idx) == meta["model_cases"] >= 100
    assert [t for t, c in enumerate(cases) if C.in_model_subset(t, c)] == list(idx)
    for t, (got, nexp) in zip(idx, _model_paths(cases, idx)):
        assert got.shape == paths[t].shape and np.array_equal(got, paths[t]), (t, cases[t]["kind"], cases[t]["shape"])
        assert nexp == int(z["steps"][t]), (t, nexp, int(z["steps"][t]))


def test_the_recorded_paths_tell_the_order_rule_apart(searches):
    """The same model with a deliberately wrong rule (always insert at the front of the list): some recorded reference path must then
    differ -- as many as the recorder counted -- or the comparison above would not be checking the tie-breaking at all."""
    z, meta, paths, cases = searches
    idx = np.nonzero(z["model"])[0]
    orig = astar_model.Row._place
    astar_model.Row._place = lambda self, lst, nb, e: lst.insert(0, e)
    try:
        got = _model_paths(cases, idx)
    finally:
        astar_model.Row._place = orig
    diff = sum(not (g.shape == paths[t].shape and np.array_equal(g, paths[t])) for t, (g, _) in zip(idx, got))
    assert meta["front_insertion_diffs"] > 0
    assert diff == meta["front_insertion_diffs"], (diff, meta["front_insertion_diffs"])


# ------------------------------------------------------------------------------------- the goal stage with the reference in the loop
def _both(oracle, *args, **kw):
    kw = dict(kw, want_paths=True, want_expansions=True)
    own = oracle.goal_prior_based_map(*args, **kw)
    with oracle.reference_astar():
        ref = oracle.goal_prior_based_map(*args, **kw)
    return own, ref


def _assert_same_stage(own, ref, what):
    assert np.array_equal(own[0].view(np.uint32), ref[0].view(np.uint32)), what          # goals, bit for bit
    assert np.array_equal(own[2], ref[2]), what                                              # flags
    assert np.array_equal(own[3], ref[3]), (what, own[3], ref[3])                            # summed expansion counts
    assert len(own[1]) == len(ref[1])
    for q, (a, b) in enumerate(zip(own[1], ref[1])):
        assert a.shape == b.shape and np.array_equal(a, b), (what, q)


def test_goal_stage_with_the_reference_search_in_the_loop(oracle):
    """oracle.goal_prior_based_map with its own search and inside reference_astar(): goals, paths, flags and expansion counts bit for bit
    -- the forest with 16 agents over 6 closed-loop ticks (the oracle's own tick flies the swarm) and one tick of a blocky maze."""
    if oracle.ref_astar_lib() is None:
        pytest.skip("oracle/_ref/libref_astar.so not built (make -C oracle ref with the reference checkout)")
    from maputil import forest_leaves
    import lsc_planner_amd as L
    from lsc_planner_amd.planner import next_state_host
    leaves, res = forest_leaves()
    wmin, wmax = (-5, -5, 0), (5, 5, 2.5)
    dm = oracle.DistMap(leaves, res, wmin, wmax)
    prm = oracle.make_params(world_min=wmin, world_max=wmax, obs_f32=True)
    ms = L.random_swarm(16, world=wmin + wmax, seed=3, edt=dm.dist, edt_key_min=dm.key_min)
    sw = oracle.Swarm(prm, ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
    state = np.zeros((16, 9), np.float32)
    state[:, :3] = ms.start
    traj = np.zeros((16, 3, 30), np.float32)
    searched = second = 0
    for tick in range(1, 7):
        own, ref = _both(oracle, prm, dm, state, ms.goal, traj, tick, ms.radius, ms.downwash)
        _assert_same_stage(own, ref, ("forest", tick))
        searched += int((ref[3] > 0).sum())
        o = sw.tick(state, ref[0], traj, tick)
        traj = o["traj"]
        sw.stale[:] = traj
        state = next_state_host(traj)
    assert searched >= 6 * 8 and max(len(p) for p in ref[1]) >= 10
    # one tick of a blocky maze (the small_2 goal case: one of its agents takes the second, unprioritised search)
    sp, ms, dist, kmin, crc, state, traj = C.goal_inputs(L, "small_2", *_maze_seeds("small_2"))
    dm = oracle.DistMap.from_array(dist, kmin, C.FIELD_RES)
    prm = oracle.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True)
    own, ref = _both(oracle, prm, dm, state, ms.goal, traj, 1, ms.radius, ms.downwash, grid_margin=C.GRID_MARGIN)
    _assert_same_stage(own, ref, "maze")
    assert (ref[2] & 2).any() and (ref[3] > 0).sum() >= 8


def _maze_seeds(name):
    meta, cases = C.load_goal_cases()
    return cases[name]["field_seed"], cases[name]["swarm_seed"]


def test_recorded_goal_cases_belong_to_their_inputs_and_to_the_oracle(oracle):
    """tests/golden/astar_ref_goal_cases.npz (recorded with the reference's search in the loop; what tests/test_gpu_goal_reference.py holds
    the kernels to): inputs rebuilt from their seeds and checksummed, the conditions on the case set, and the oracle's own goal stage
    against every recorded answer -- flags, paths, summed expansion counts and goals, bit for bit.  Live too where oracle/_ref is built."""
    import lsc_planner_amd as L
    meta, cases = C.load_goal_cases()
    assert list(cases) == list(C.GOAL_SPECS)
    C.check_goal_conditions(cases)
    live = oracle.ref_astar_lib() is not None
    for name, c in cases.items():
        sp, ms, dist, kmin, crc, state, traj = C.goal_inputs(L, name, c["field_seed"], c["swarm_seed"])
        assert crc == c["field_crc"] and np.array_equal(state, c["state"]) and np.array_equal(traj, c["traj"]), name
        assert np.array_equal(ms.goal.astype(np.float32), c["goal"]), name
        with oracle.segments(sp["M"]):
            dm = oracle.DistMap.from_array(dist, kmin, C.FIELD_RES)
            prm = oracle.make_params(dt=sp["dt"], world_min=ms.world_min, world_max=ms.world_max, obs_f32=True, world_dimension=sp["dim"],
                                     world_z_2d=sp["z2d"])
            dims, _ = oracle.grid_dims(prm)
            assert tuple(int(v) for v in dims) == c["grid_dims"] == C.EXPECTED_GRID[name], name
            args = (prm, dm, state, ms.goal, traj, sp["planner_seq"], ms.radius, ms.downwash)
            if live:
                runs = _both(oracle, *args, grid_margin=C.GRID_MARGIN)
            else:
                runs = (oracle.goal_prior_based_map(*args, grid_margin=C.GRID_MARGIN, want_paths=True, want_expansions=True),)
        for goals, paths, flags, steps in runs:
            assert np.array_equal(goals.view(np.uint32), c["goals_out"].view(np.uint32)), name
            assert np.array_equal(flags, c["flags"]) and np.array_equal(steps, c["steps"]), (name, steps, c["steps"])
            for q in range(C.N_AGENTS):
                assert paths[q].shape == c["paths"][q].shape and np.array_equal(paths[q], c["paths"][q]), (name, q)
