"""-m gpu: the map built on the device from occupancy (lsc_set_occupancy, csrc/lsc_map.hip) and changed between ticks (lsc_map_update).

The yardstick is the parent's own path and it is exact: a twin context is fed lsc_set_distmap with the HOST distance field of the same
occupancy (lsc_edt_from_bt on the occupancy written out as a .bt file), and every product lsc_map_read serves -- the distance field, the
integral images, the goal planner's occupancy -- must be the twin's, byte for byte.  Small grids are held to the numpy restatement of
tests/map_reference.py as well.  Fields lie inside (or around) an ordinary 4 m world, so the planner's own limits do not interfere."""
import ctypes
import os

import numpy as np
import pytest

import corridor_worlds
import map_reference as MR
from harness import assert_tick_matches, start_inputs
from maputil import forest_leaves, write_bt
from test_gpu_octomap_batch import mission, suite  # noqa: F401  (the forest suite's fixture and reader)
from tolerances import ACTIVE_SET_TRAJ_ATOL, COST_ATOL

pytestmark = pytest.mark.gpu

RES = 0.1
WMIN, WMAX = np.array([-2.0, -2.0, 0.0], np.float32), np.array([2.0, 2.0, 2.0], np.float32)
PRODUCTS = ("edt", "integral", "goal_occupancy")


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    return L


def _mission(L, radii=(0.15, 0.15, 0.15), wmin=WMIN, wmax=WMAX):
    n = len(radii)
    start = np.array([[-1.5, -1.5 + 0.9 * q, 1.0] for q in range(n)], np.float32)
    goal = np.array([[1.5, 1.5 - 0.9 * q, 1.0] for q in range(n)], np.float32)
    return L.Mission(start, goal, np.asarray(wmin, np.float32), np.asarray(wmax, np.float32), np.asarray(radii, np.float64), np.full(n, 2.0),
                     np.tile([1.0, 1.0, 1.0], (n, 1)), np.tile([2.0, 2.0, 2.0], (n, 1)), np.full(n, 1.0), name="map_device")


def _cfg(L, **kw):
    kw.setdefault("goal_mode", "prior_based")
    return L.PlannerConfig(use_octomap=True, **kw)


def _centred(shape):
    """key_min of a field of `shape` cells around the middle of the 4 m world."""
    mid = (WMIN.astype(np.float64) + WMAX) / 2
    return np.array([int(np.floor(mid[a] / RES)) + 32768 - shape[a] // 2 for a in range(3)], np.int32)


def _host_edt(L, tmp, occ, kmin, maxdist=1.0):
    """lsc_edt_from_bt of the occupancy: written out as single-cell leaves, read back over the field's own box (its cells' centres)."""
    idx = np.argwhere(np.asarray(occ) != 0)
    leaves = np.concatenate([idx + np.asarray(kmin), np.ones((len(idx), 1), int)], 1).astype(np.int32)
    path = os.path.join(str(tmp), f"occ_{abs(hash((occ.shape, occ.tobytes(), tuple(kmin)))):x}.bt")
    write_bt(path, leaves, RES)
    lo = (np.asarray(kmin, np.float64) - 32768 + 0.5) * RES
    hi = (np.asarray(kmin, np.float64) + np.asarray(occ.shape) - 1 - 32768 + 0.5) * RES
    dist, km, res = L.edt_from_bt(path, lo, hi, maxdist)
    assert dist.shape == occ.shape and np.array_equal(km, kmin) and res == RES
    assert np.array_equal(dist == 0, np.asarray(occ) != 0)
    return dist


def _same_products(a, b, what=""):
    assert np.array_equal(a["dims"][:7], b["dims"][:7]), (what, a["dims"], b["dims"])
    for k in PRODUCTS:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k, int((a[k] != b[k]).sum()))


def _reference_products(pl, occ, kmin, maxdist, ms, cfg):
    dist = MR.edt(occ, RES, maxdist)
    radii, _ = MR.distinct_radii(ms.radius)
    planar = cfg.world_z_2d if cfg.world_dimension == 2 else None
    return dict(edt=dist, integral=MR.integral(dist, radii, cfg.world_resolution),
                goal_occupancy=MR.goal_occupancy(dist, kmin, RES, radii, ms.world_min, ms.world_max, cfg.grid_resolution, cfg.grid_margin, planar))


def _set_agents_again(pl):
    from lsc_planner_amd.planner import _dp
    ms = pl.mission
    pl._check(pl.L.lsc_set_agents(pl.ctx, pl.N, _dp(np.ascontiguousarray(ms.radius, np.float64)), _dp(np.ascontiguousarray(ms.downwash, np.float64)),
                                  _dp(np.ascontiguousarray(ms.max_vel, np.float64)), _dp(np.ascontiguousarray(ms.max_acc, np.float64)),
                                  _dp(np.ascontiguousarray(ms.nominal_velocity, np.float64))))


def _build_and_compare(L, tmp, occ, kmin, maxdist=1.0, ms=None, agents_after=False, **cfg_kw):
    """(device context, its products): occupancy -> device, against the twin (host field -> lsc_set_distmap) and, on small grids,
    against the numpy restatement."""
    ms = ms or _mission(L)
    cfg = _cfg(L, **cfg_kw)
    pl, twin = L.SwarmPlanner(ms, cfg), L.SwarmPlanner(ms, cfg)
    try:
        pl.set_occupancy(occ, kmin, RES, maxdist)
        twin.set_distmap(_host_edt(L, tmp, occ, kmin, maxdist), kmin, RES)
        if agents_after:
            _set_agents_again(pl); _set_agents_again(twin)
        got, want = pl.map_read(), twin.map_read()
        assert got["dims"][7] == 1 and want["dims"][7] == 0 and want["occupancy"] is None
        assert np.array_equal(got["occupancy"] != 0, np.asarray(occ) != 0)
        _same_products(got, want, (occ.shape, maxdist))
        assert got["integral"].shape[0] == len(set(ms.radius)) and got["goal_occupancy"].shape[0] == len(set(ms.radius))
        if occ.size <= 6000:
            ref = _reference_products(pl, occ, kmin, maxdist, ms, cfg)
            for k in PRODUCTS:
                assert got[k].tobytes() == ref[k].tobytes(), (occ.shape, k)
    finally:
        twin.close()
    return pl, got


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


# md = (int)(1.0 / 0.1 + 1) = 11: axes of md, md + 1 and 2 md - 1 cells; shorter than the window; wave (64 / 65 along z) and workgroup
# (257 along x) edges
SHAPES = [((3, 2, 1), 0.4), ((5, 40, 3), 0.03), ((11, 4, 3), 0.05), ((12, 4, 3), 0.05), ((21, 4, 3), 0.05), ((6, 5, 64), 0.01), ((6, 5, 65), 0.01),
          ((257, 6, 5), 0.01), ((24, 20, 12), 0.01), ((24, 20, 12), 0.3)]


@pytest.mark.parametrize("shape,density", SHAPES)
@pytest.mark.parametrize("maxdist", [1.0, 0.35])
def test_products_are_the_host_paths(L, tmp_path, shape, density, maxdist):
    occ = _random(shape, density, 7 + shape[0])
    if not occ.any():
        occ[tuple(s // 2 for s in shape)] = 1
    pl, _ = _build_and_compare(L, tmp_path, occ, _centred(shape), maxdist)
    pl.close()


@pytest.mark.parametrize("value", [0, 1])
def test_single_cell_empty_and_full_grids(L, tmp_path, value):
    for shape in ((1, 1, 1), (20, 20, 10)):
        occ = np.full(shape, value, np.uint8)
        pl, got = _build_and_compare(L, tmp_path, occ, _centred(shape))
        assert (got["edt"] == (np.float32(0.0) if value else np.float32(np.float64(np.float32(11.0)) * RES))).all()
        pl.close()


def test_a_voxel_at_each_corner(L, tmp_path):
    shape = (14, 13, 12)
    for c in range(8):
        occ = np.zeros(shape, np.uint8)
        occ[tuple((shape[a] - 1) if (c >> a) & 1 else 0 for a in range(3))] = 1
        pl, _ = _build_and_compare(L, tmp_path, occ, _centred(shape))
        pl.close()


def test_field_larger_than_the_world(L, tmp_path):
    w = corridor_worlds.field_larger_than_world(3)
    occ = (w.dist == 0).astype(np.uint8)
    assert occ.any() and occ.shape[0] > 41
    pl, _ = _build_and_compare(L, tmp_path, occ, w.key_min, ms=_mission(L, wmin=w.wmin, wmax=w.wmax))
    pl.close()


@pytest.fixture(scope="module")
def forest_bt(tmp_path_factory):
    leaves, res = forest_leaves()
    bt = os.path.join(str(tmp_path_factory.mktemp("forest")), "simple_forest.bt")
    write_bt(bt, leaves, res)
    return bt


FOREST_WORLD = (np.array([-5.0, -5.0, 0.0], np.float32), np.array([5.0, 5.0, 2.5], np.float32))


@pytest.mark.parametrize("segments", [5, 4])
def test_simple_forest_from_its_file(L, forest_bt, segments):
    """load_octomap(on_device=True) against load_octomap: the shipped map, 101 x 101 x 26 cells; once through the M = 4 library."""
    ms = _mission(L, radii=(0.15, 0.2, 0.15), wmin=FOREST_WORLD[0], wmax=FOREST_WORLD[1])
    kw = dict(dt=0.5, horizon=2.0) if segments == 4 else {}
    pl, twin = L.SwarmPlanner(ms, _cfg(L, **kw)), L.SwarmPlanner(ms, _cfg(L, **kw))
    assert pl.M == segments
    occ, kmin, res = pl.load_octomap(forest_bt, on_device=True)
    dist, kmin_t, _ = twin.load_octomap(forest_bt)
    assert np.array_equal(occ != 0, dist == 0) and np.array_equal(kmin, kmin_t)
    _same_products(pl.map_read(), twin.map_read(), "forest")
    pl.close(); twin.close()


def test_two_radii_agents_before_and_after_the_map_and_a_planar_world(L, tmp_path):
    shape = (41, 41, 21)
    occ, kmin = _random(shape, 0.004, 11), _centred(shape)
    ms = _mission(L, radii=(0.15, 0.25, 0.15, 0.25))
    for after in (False, True):
        pl, got = _build_and_compare(L, tmp_path, occ, kmin, ms=ms, agents_after=after)
        assert got["integral"].shape[0] == 2 and not np.array_equal(got["integral"][0], got["integral"][1])
        assert got["goal_occupancy"].shape[0] == 2 and not np.array_equal(got["goal_occupancy"][0], got["goal_occupancy"][1])
        pl.close()
    pl, got = _build_and_compare(L, tmp_path, occ, kmin, ms=ms, world_dimension=2, world_z_2d=1.0)
    assert got["goal_occupancy"].shape[1] == 1                                     # one grid layer
    pl.close()
    # static goals: the context plans no goals on the map and has no goal grid
    pl, got = _build_and_compare(L, tmp_path, occ, kmin, ms=ms, goal_mode="static")
    assert got["goal_occupancy"].size == 0 and got["integral"].shape[0] == 2
    pl.close()


# ---- updates ----------------------------------------------------------------------------------------------------------------------

def _fresh_products(L, ms, cfg, occ, kmin, maxdist=1.0):
    pl = L.SwarmPlanner(ms, cfg)
    pl.set_occupancy(occ, kmin, RES, maxdist)
    out = pl.map_read()
    pl.close()
    return out


def test_a_sequence_of_edits(L, tmp_path):
    """After every edit the products are those of a fresh context built from the edited occupancy (which test_products_are_the_host_paths
    holds to the host path) -- and, at the end, the twin's of the final occupancy."""
    import torch
    shape = (30, 28, 14)
    occ, kmin = _random(shape, 0.01, 5), _centred(shape)
    ms, cfg = _mission(L, radii=(0.15, 0.25, 0.15)), _cfg(L)
    pl, _ = _build_and_compare(L, tmp_path, occ, kmin, ms=ms)
    rng = np.random.default_rng(9)
    many = [[int(x), int(y), int(z), int(x) + 2, int(y) + 1, int(z) + 3] for x, y, z in zip(rng.integers(0, 28, 64), rng.integers(0, 27, 64), rng.integers(0, 11, 64))]
    edits = [
        ([[10, 12, 0, 13, 15, 14]], [1]),                                          # a 3 x 3 column of full height
        ([[10, 12, 0, 13, 15, 14]], [0]),                                          # ... removed
        ([[0, 5, 3, 1, 20, 9], [27, 0, 13, 30, 28, 14]], [1, 1]),                   # touching faces of the field
        (many, [int(v) for v in rng.integers(0, 2, 64)]),                          # 64 boxes in one call
        ([[4, 4, 2, 12, 12, 9], [6, 6, 0, 10, 10, 14], [5, 5, 3, 8, 8, 6]], [1, 0, 1]),   # overlapping, opposite values: the later one wins
        ([], []),                                                                   # no box: a rebuild of the same map
    ]
    for n, (boxes, values) in enumerate(edits):
        before = occ
        occ = MR.apply_boxes(occ, boxes, values)
        assert n in (1, 5) or not np.array_equal(occ, before)
        pl.map_update(boxes, values)
        got = pl.map_read()
        assert np.array_equal(got["occupancy"], occ), n
        _same_products(got, _fresh_products(L, ms, cfg, occ, kmin), n)
    assert occ[6, 6, 4] == 1 and occ[7, 7, 8] == 0 and occ[4, 4, 2] == 1            # (the overlap's three layers)
    twin = L.SwarmPlanner(ms, cfg)
    twin.set_distmap(_host_edt(L, tmp_path, occ, kmin), kmin, RES)
    _same_products(pl.map_read(), twin.map_read(), "final")
    # a whole grid from a torch tensor
    occ2 = _random(shape, 0.02, 6)
    pl.map_update(torch.from_numpy(occ2).cuda())
    got = pl.map_read()
    assert np.array_equal(got["occupancy"], occ2)
    twin.set_distmap(_host_edt(L, tmp_path, occ2, kmin), kmin, RES)
    _same_products(got, twin.map_read(), "device grid")
    pl.close(); twin.close()


def test_refusals_name_their_cause_and_the_context_plans_on(L, tmp_path):
    shape = (41, 41, 21)
    occ, kmin = _random(shape, 0.003, 21), _centred(shape)
    ms = _mission(L)
    pl = L.SwarmPlanner(ms, _cfg(L))
    state, traj = start_inputs(ms, pl.SEGV)
    with pytest.raises(L.LscError, match="-5.*lsc_map_update: the context's map is not a device occupancy"):
        pl.map_update([[0, 0, 0, 1, 1, 1]], [1])
    pl.set_distmap(_host_edt(L, tmp_path, occ, kmin), kmin, RES)
    with pytest.raises(L.LscError, match="-5.*not a device occupancy"):
        pl.map_update([[0, 0, 0, 1, 1, 1]], [1])
    for bad, why in ((dict(maxdist=0.0), "maxdist must be positive and finite"), (dict(maxdist=float("inf")), "maxdist must be positive and finite"),
                     (dict(maxdist=float("nan")), "maxdist must be positive and finite"), (dict(maxdist=12.8), "more than the 127"),
                     (dict(res=0.2), "lsc_set_occupancy: map resolution differs from world_resolution")):
        with pytest.raises(L.LscError, match="-1.*" + why):
            pl.set_occupancy(occ, kmin, bad.get("res", RES), bad.get("maxdist", 1.0))
    with pytest.raises(L.LscError, match="-1.*every dimension of the grid must be at least 1"):
        pl._check(pl.L.lsc_set_occupancy(pl.ctx, occ.ctypes.data, 0, 41, 21, kmin.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), RES, 1.0))
    assert pl.map_read()["occupancy"] is None                                      # still the map of lsc_set_distmap
    pl.set_occupancy(occ, kmin, RES, 12.6)                                         # md = 127 is served
    pl.set_occupancy(occ, kmin, RES, 1.0)
    before = pl.map_read()
    for boxes, values, why in (([[0, 0, 0, 42, 1, 1]], [1], "box 0, axis 0"), ([[0, -1, 0, 1, 1, 1]], [1], "box 0, axis 1"),
                               ([[0, 0, 0, 1, 1, 1], [3, 3, 5, 4, 4, 5]], [1, 1], "box 1, axis 2"), ([[5, 5, 5, 4, 6, 6]], [0], "box 0, axis 0"),
                               ([[0, 0, 0, 1, 1, 1]] * 65, [1] * 65, "n_boxes must be 0 .. 64"), ([[0, 0, 0, 1, 1, 1]], [2], "box 0: value must be 0")):
        with pytest.raises(L.LscError, match="-1.*lsc_map_update: " + why):
            pl.map_update(boxes, values)
    with pytest.raises(L.LscError, match="boxes need values"):
        pl.map_update([[0, 0, 0, 1, 1, 1]])
    with pytest.raises(L.LscError, match=r"boxes must be \[n\]\[6\]"):
        pl.map_update([[0, 0, 0, 1, 1]], [1])
    after = pl.map_read()
    _same_products(after, before, "a refused update changes nothing")
    assert np.array_equal(after["occupancy"], before["occupancy"])
    twin = L.SwarmPlanner(ms, _cfg(L))
    twin.set_distmap(_host_edt(L, tmp_path, occ, kmin), kmin, RES)
    for tick in range(1, 4):
        g, t = pl.plan(state, ms.goal, traj), twin.plan(state, ms.goal, traj)
        for k in ("traj", "cost", "status", "iters", "sfc"):
            assert np.array_equal(g[k], t[k]), (tick, k)
        assert np.array_equal(pl.last_goals(), twin.last_goals())
        traj = g["traj"]
    # lsc_set_distmap replaces the map and drops the occupancy
    pl.set_distmap(_host_edt(L, tmp_path, occ, kmin), kmin, RES)
    assert pl.map_read()["occupancy"] is None
    with pytest.raises(L.LscError, match="-5"):
        pl.map_update([], [])
    pl.close(); twin.close()


# ---- flights ----------------------------------------------------------------------------------------------------------------------

def _forest_occ(L, bt, ms):
    return L.occupancy_from_bt(bt, ms.world_min, ms.world_max)


def column_box(occ_shape, kmin, res, p0, p1, positions, clear=0.5, shift=0, free_in=None):
    """The 3 x 3-cell full-height column by rule: the cell on the straight line p0 -> p1 nearest its midpoint (then `shift` cells further
    along the walk) whose centre is at least `clear` metres (horizontally) from every position -- and, given an occupancy free_in, whose
    column is free in it.  Returns x0, y0, z0, x1, y1, z1."""
    p0, p1 = np.asarray(p0, np.float64)[:2], np.asarray(p1, np.float64)[:2]
    n = int(np.ceil(np.linalg.norm(p1 - p0) / (res / 2)))
    order = sorted(range(n + 1), key=lambda i: abs(i - n / 2))
    seen, found = set(), []
    for i in order:
        p = p0 + (p1 - p0) * (i / n)
        c = tuple(int(np.floor(p[a] / res)) + 32768 - int(kmin[a]) for a in range(2))
        if c in seen or not (1 <= c[0] < occ_shape[0] - 1 and 1 <= c[1] < occ_shape[1] - 1):
            continue
        seen.add(c)
        centre = (np.array(c) + np.asarray(kmin[:2]) - 32768 + 0.5) * res
        if free_in is not None and free_in[c[0] - 1:c[0] + 2, c[1] - 1:c[1] + 2].any():
            continue
        if np.linalg.norm(np.asarray(positions, np.float64)[:, :2] - centre, axis=1).min() >= clear:
            found.append(c)
            if len(found) > shift:
                return [c[0] - 1, c[1] - 1, 0, c[0] + 2, c[1] + 2, occ_shape[2]]
    raise AssertionError("no cell of the line is clear of the agents")


def _leaves_of(occ, kmin):
    idx = np.argwhere(occ != 0)
    return np.concatenate([idx + np.asarray(kmin), np.ones((len(idx), 1), int)], 1).astype(np.int32)


COLUMN_SHIFT = 0          # cells the column is moved along the line from the rule's first choice (0: the rule's own cell moves a box or a goal)
APPEARS, REMOVED, TICKS = 10, 20, 30


def test_closed_loop_with_a_column_that_appears_and_goes(L, oracle, suite):
    """The forest suite's first mission (multi_random_20agents_1 on forest1.bt; the suite counts from 1), 20 agents, prior_based goals, 30 ticks; a column appears at tick 10 on agent 0's line and is removed at tick 20.
    The device-updated context against: the oracle given DistMap(edited leaves) at the same ticks (boxes and goals bit for bit, plans
    within the active-set tolerance), the lsc_set_distmap twin (every output equal), and a context that never updates (must differ)."""
    from lsc_planner_amd.planner import next_state_host
    ms, bt = mission(L, suite, "forest", 1)
    cfg = _cfg(L)
    occ0, kmin, res = _forest_occ(L, bt, ms)
    pl, twin, never = (L.SwarmPlanner(ms, cfg) for _ in range(3))
    pl.set_occupancy(occ0, kmin, res)
    dist0, _, _ = twin.load_octomap(bt)
    never.load_octomap(bt)
    prm = oracle.make_params(world_min=ms.world_min, world_max=ms.world_max, use_sfc=True, obs_f32=True)
    sw = oracle.Swarm(prm, ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
    dm = oracle.DistMap(_leaves_of(occ0, kmin), res, ms.world_min, ms.world_max)
    assert dm.dist.tobytes() == dist0.tobytes()
    sw.set_distmap(dm)
    state, traj = start_inputs(ms, pl.SEGV)
    stale = np.zeros_like(traj)
    occ, box, differs = occ0, None, False
    for tick in range(1, TICKS + 1):
        if tick in (APPEARS, REMOVED):
            if tick == APPEARS:
                box = column_box(occ0.shape, kmin, res, ms.start[0], ms.goal[0], state[:, :3], shift=COLUMN_SHIFT)
            value = 1 if tick == APPEARS else 0
            # (removing restores the map as it was: the column's cells that the forest occupies come back)
            boxes, values = ([box], [1]) if value else ([box] + _restore(occ0, box), [0] + [1] * len(_restore(occ0, box)))
            occ = MR.apply_boxes(occ, boxes, values)
            assert np.array_equal(occ, occ0) == (value == 0)
            pl.map_update(boxes, values)
            dm = oracle.DistMap(_leaves_of(occ, kmin), res, ms.world_min, ms.world_max)
            twin.set_distmap(dm.dist, kmin, res)
            sw.set_distmap(dm)
        goals_ref = oracle.goal_prior_based_map(prm, dm, state, ms.goal, traj, tick, ms.radius, ms.downwash, grid_margin=cfg.grid_margin, grid_res=cfg.grid_resolution)
        g, t, n = pl.plan(state, ms.goal, traj, want_constraints=True), twin.plan(state, ms.goal, traj, want_constraints=True), never.plan(state, ms.goal, traj)
        for k in ("traj", "cost", "status", "iters", "sfc", "normal", "d"):
            assert np.array_equal(g[k], t[k]), (tick, k)
        assert np.array_equal(pl.last_goals(), twin.last_goals()), tick
        assert np.array_equal(pl.last_goals(), goals_ref), tick
        sw.stale[:] = stale
        o = sw.tick(state, goals_ref, traj, tick, want_lsc=True, nthreads=8)
        assert np.array_equal(g["sfc"], o["sfc"]), tick
        assert (g["status"] < 4).all(), (tick, g["status"])                         # no corridor or goal error
        assert_tick_matches(g, o, tick, rows="bits", cost_atol=COST_ATOL, traj_atol=ACTIVE_SET_TRAJ_ATOL)
        same_map_outputs = np.array_equal(g["sfc"], n["sfc"]) and np.array_equal(pl.last_goals(), never.last_goals())
        same = same_map_outputs and np.array_equal(g["traj"], n["traj"])
        assert same or tick >= APPEARS, tick
        differs = differs or not same_map_outputs                                # (a box or a planned goal, not a plan alone)
        stale = np.where((o["status"] == 0)[:, None, None], g["traj"], stale).astype(np.float32)
        traj = g["traj"]
        state = next_state_host(traj)
    assert differs, "the column never moved a box or a planned goal: the comparison would be vacuous"
    for p in (pl, twin, never):
        p.close()


def _restore(occ0, box):
    """Single-cell boxes that put the original occupancy back inside `box`."""
    x0, y0, z0, x1, y1, z1 = box
    idx = np.argwhere(occ0[x0:x1, y0:y1, z0:z1] != 0) + np.array([x0, y0, z0])
    return [[int(x), int(y), int(z), int(x) + 1, int(y) + 1, int(z) + 1] for x, y, z in idx]


def test_regrow_corridors(L, suite):
    """After an update with the flag every agent's next boxes are those of a fresh planner given the same map, state, plans and
    planner_seq (all M boxes regrown from the current position); without it the shifted boxes are the twin's."""
    from lsc_planner_amd.planner import next_state_host
    ms, bt = mission(L, suite, "forest", 1, 8)
    cfg = _cfg(L, goal_mode="static")
    occ0, kmin, res = _forest_occ(L, bt, ms)
    regrow, keep, twin = (L.SwarmPlanner(ms, cfg) for _ in range(3))
    regrow.set_occupancy(occ0, kmin, res); keep.set_occupancy(occ0, kmin, res)
    twin.load_octomap(bt)
    state, traj = start_inputs(ms, regrow.SEGV)
    for tick in range(1, 7):
        g = regrow.plan(state, ms.goal, traj)
        assert np.array_equal(keep.plan(state, ms.goal, traj)["sfc"], g["sfc"]) and np.array_equal(twin.plan(state, ms.goal, traj)["sfc"], g["sfc"])
        traj = g["traj"]; state = next_state_host(traj)
    box = column_box(occ0.shape, kmin, res, ms.start[0], ms.goal[0], state[:, :3])
    occ = MR.apply_boxes(occ0, [box], [1])
    regrow.map_update([box], [1], regrow=True)
    keep.map_update([box], [1])
    twin.set_distmap(_edt_of(occ, kmin, res, ms), kmin, res)
    fresh = L.SwarmPlanner(ms, cfg)
    fresh.set_occupancy(occ, kmin, res)
    fresh.planner_seq = regrow.planner_seq
    g, k, t, f = (p.plan(state, ms.goal, traj) for p in (regrow, keep, twin, fresh))
    assert np.array_equal(g["sfc"], f["sfc"])
    assert (g["sfc"] == g["sfc"][:, :1]).all()                                     # M copies of the box grown at the current position
    assert np.array_equal(k["sfc"], t["sfc"])
    assert not np.array_equal(k["sfc"], g["sfc"])                                  # boxes grown before the change stay as grown
    for p in (regrow, keep, twin, fresh):
        p.close()


def _edt_of(occ, kmin, res, ms):
    from oracle import oracle as O
    return O.DistMap(_leaves_of(occ, kmin), res, ms.world_min, ms.world_max).dist


def test_an_update_between_two_flights_on_one_stream(L, suite):
    """fly 5 ticks, map_update on the same stream with no synchronise, fly 5 more == the per-tick loop with the update in front of
    tick 6: the buffers and the rows of the flight log."""
    import torch
    ms, bt = mission(L, suite, "forest", 1, 8)
    occ0, kmin, res = _forest_occ(L, bt, ms)
    state0, _ = start_inputs(ms, 30)
    box = column_box(occ0.shape, kmin, res, ms.start[0], ms.goal[0], state0[:, :3], clear=0.3)
    dev = torch.device("cuda", 0)
    results = []
    for batched in (True, False):
        pl = L.SwarmPlanner(ms, _cfg(L))
        pl.set_occupancy(occ0, kmin, res)
        n, nv = ms.qn, pl.NV
        f32 = dict(dtype=torch.float32, device=dev)
        s0 = torch.zeros((n, 9), **f32); s0[:, :3] = torch.from_numpy(ms.start).to(dev)
        states, trajs = [s0, torch.zeros_like(s0)], [torch.zeros((n, nv), **f32), torch.zeros((n, nv), **f32)]
        goal = torch.from_numpy(ms.goal).to(dev).contiguous()
        cost, status, iters = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        pl.flight_begin([0.0, 0.1], 10)
        if batched:
            pl.fly(states, goal, trajs, 1, 5, cost, status, iters, stream)
            pl.map_update([box], [1], stream=stream)
            pl.fly([states[1], states[0]], goal, [trajs[1], trajs[0]], 6, 5, cost, status, iters, stream)
        else:
            for tick in range(1, 11):
                if tick == 6:
                    pl.map_update([box], [1], stream=stream)
                k = (tick - 1) % 2
                pl.fly([states[k], states[1 - k]], goal, [trajs[k], trajs[1 - k]], tick, 1, cost, status, iters, stream)
        torch.cuda.synchronize()
        log = pl.flight_read(0, 10)
        results.append([t.cpu().numpy().copy() for t in (*states, *trajs, cost, status, iters)] + [pl.last_goals(), log])
        pl.close()
    a, b = results
    for x, y in zip(a[:-1], b[:-1]):
        assert np.array_equal(x, y)
    for k in a[-1]:
        assert np.array_equal(a[-1][k], b[-1][k]), k


# ---- lsc_sim --map-on-device --world-events ---------------------------------------------------------------------------------------

SIM = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsc_planner_amd", "lsc_sim")


def _cells(rows):
    """The CSV as text without planning_time (column 11 of an agent's 15), the wall clock of that run's ticks."""
    return [[c for i, c in enumerate(row) if i % 15 != 11] for row in rows]


@pytest.fixture(scope="module")
def sim_flights(L, forest_bt, tmp_path_factory):
    """Three agents in the forest, flown by lsc_sim: without events, with a column that appears in front of tick 2 -- beyond what a plan made at the
    start reaches within its horizon, so that no plan in flight runs through it -- (per-tick loop and --device-loop 7: a batch of one tick,
    then batches of seven), and with the column and its inverse in front of the same tick."""
    import csv
    import json
    import subprocess
    assert os.path.exists(SIM), "lsc_sim not built"
    dist, kmin, res = L.edt_from_bt(forest_bt, FOREST_WORLD[0], FOREST_WORLD[1])
    ms = L.random_swarm(3, world=(-5.0, -5.0, 0.0, 5.0, 5.0, 2.5), seed=20260928, edt=dist, edt_key_min=kmin, edt_res=res)
    doc = {"quadrotors": {"crazyflie": {"max_vel": [1.0, 1.0, 1.0], "max_acc": [2.0, 2.0, 2.0], "radius": 0.15, "nominal_velocity": 1.0, "downwash": 2.0}},
           "world": [{"dimension": [-5, -5, 0, 5, 5, 2.5]}],
           "agents": [{"type": "crazyflie", "start": [float(v) for v in ms.start[q]], "goal": [float(v) for v in ms.goal[q]]} for q in range(3)]}
    box = column_box(dist.shape, kmin, res, ms.start[0], ms.goal[0], ms.start, clear=1.6, free_in=dist == 0)
    lo = [float((box[a] + kmin[a] - 32768 + 0.5) * res) for a in range(3)]
    hi = [float((box[3 + a] - 1 + kmin[a] - 32768 + 0.5) * res) for a in range(3)]
    appear = {"tick": 2, "box": lo + hi, "occupied": True, "regrow": False}
    events = {"plain": None, "events": [appear], "loop": [appear], "inverse": [appear, dict(appear, occupied=False)]}
    out = {}
    for run, ev in events.items():
        d = tmp_path_factory.mktemp(f"sim_{run}")
        (d / "m.json").write_text(json.dumps(doc))
        cmd = [SIM, "--mission", str(d / "m.json"), "--world", forest_bt, "--csv", str(d), "--quiet", "--max-iter", "100", "--map-on-device"]
        if ev is not None:
            (d / "events.json").write_text(json.dumps(ev))
            cmd += ["--world-events", str(d / "events.json")]
        if run == "loop":
            cmd += ["--device-loop", "7"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        f = d / "result_LSC_3agents.csv"
        out[run] = (r, list(csv.reader(open(f))) if f.exists() else [])
        if r.returncode < 0 or r.returncode > 3:                   # (killed or crashed: nothing more is started)
            break
    return out


def test_sim_world_events(sim_flights):
    for run, (r, rows) in sim_flights.items():
        assert r.returncode == 0, (run, r.stdout[-800:], r.stderr[-1500:])
        assert len(rows) > 20, run
    cells = {run: _cells(rows) for run, (r, rows) in sim_flights.items()}
    assert cells["events"] == cells["loop"]                        # the per-tick loop and --device-loop 7 write the same CSV
    assert cells["events"] != cells["plain"]                       # ... which is not the flight without the column
    assert cells["inverse"] == cells["plain"]                      # the column and its inverse in front of one tick: the plain flight


def test_sim_refuses_world_events_without_the_device_map(tmp_path):
    import subprocess
    (tmp_path / "e.json").write_text("[]")
    r = subprocess.run([SIM, "--mission", str(tmp_path / "m.json"), "--world", str(tmp_path / "w.bt"), "--world-events", str(tmp_path / "e.json")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--world-events needs --map-on-device" in r.stderr, (r.returncode, r.stderr)
