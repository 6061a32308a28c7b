"""-m gpu: goal planning on octomap worlds whose search grid outgrows LDS.  Grids of more than 131 071 cells (or whose cells and 16-entry
OPEN rows do not fit LDS) are searched with the OPEN rows in a per-agent HBM workspace, and an LDS search whose row outgrows its LDS
capacity restarts with its rows there.  Paths, flags, expansion counts (the oracle's, summed over an agent's one or two searches; the
oracle's search is pinned to the reference's Astar-3D, tests/test_oracle_astar_ref.py) and goals must be the oracle's, bit for bit, and
the HBM search must return exactly what the LDS searches return wherever both run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from harness import start_inputs

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


@pytest.fixture(scope="module")
def tiled4(L):
    from config_runs import forest_tiles
    bt, world = forest_tiles(4)
    dist, kmin, r = L.edt_from_bt(bt, np.asarray(world[:3], np.float32), np.asarray(world[3:], np.float32))
    return bt, world, dist, kmin, r


def _forest_bt(tmp):
    from maputil import forest_leaves, write_bt
    leaves, res = forest_leaves()
    bt = os.path.join(tmp, "forest.bt")
    write_bt(bt, leaves, res)
    return bt, (-5, -5, 0, 5, 5, 2.5)


def _prior(L, **kw):
    return L.PlannerConfig(use_octomap=True, goal_mode="prior_based", **kw)


def _against_oracle(L, O, ms, pl, dm, ticks, grid_margin=0.2, **world):
    """Closed loop on the host; every tick the planned goals, flags, paths and expansion counts against the oracle.  Returns (longest path,
    most expansions)."""
    from lsc_planner_amd.planner import next_state_host
    prm = O.make_params(world_min=ms.world_min, world_max=ms.world_max, obs_f32=True, **world)
    state, traj = start_inputs(ms, pl.SEGV)
    longest = most = 0
    for tick in range(1, ticks + 1):
        ref, paths, flags, steps = O.goal_prior_based_map(prm, dm, state, ms.goal, traj, tick, ms.radius, ms.downwash, grid_margin=grid_margin,
                                                          want_paths=True, want_expansions=True)
        g = pl.plan(state, ms.goal, traj)
        tr = pl.goal_trace()
        assert (g["status"] != 5).all(), (tick, np.nonzero(g["status"] == 5))
        assert np.array_equal(tr["expansions"], steps), (tick, tr["expansions"], steps)
        assert (pl.goal_storage() == 2).all(), tick
        for qi in range(ms.qn):
            assert tr["flags"][qi] == flags[qi], (tick, qi, tr["flags"][qi], flags[qi])
            if not (flags[qi] & 1):
                assert np.array_equal(tr["paths"][qi], paths[qi]), (tick, qi, len(tr["paths"][qi]), len(paths[qi]))
        assert np.array_equal(pl.last_goals(), ref), tick
        longest = max(longest, int(tr["path_len"].max()))
        most = max(most, int(tr["expansions"].max()))
        traj = g["traj"]
        state = next_state_host(traj)
    return longest, most


def test_tiled_forest_4x4_against_the_oracle(L, oracle, tiled4):
    """134 x 134 x 9 = 161 604 cells: refused at load before this feature; now the HBM search, the reference's paths bit for bit."""
    bt, world, dist, kmin, r = tiled4
    dm = oracle.DistMap.from_array(dist, kmin, r)
    ms = L.random_swarm(64, world=world, seed=21, edt=dist, edt_key_min=kmin, edt_res=r)
    pl = L.SwarmPlanner(ms, _prior(L))
    pl.load_octomap(bt)
    note = pl.L.lsc_last_note(pl.ctx).decode()
    assert "HBM search" in note and "MB of HBM workspace per agent" in note, note
    pl.set_goal_trace(2048)
    try:
        longest, most = _against_oracle(L, oracle, ms, pl, dm, 8)
    finally:
        pl.close()
    assert longest >= 40 and most >= 1000, (longest, most)          # real searches across the tiles happened


def test_large_planar_world_against_the_oracle(L, oracle):
    """world_dimension 2 on 120 m x 120 m: a 401 x 401 x 1 grid (160 801 cells) with the cell bytes in HBM too."""
    rng = np.random.default_rng(5)
    res, lo, hi, z2d = 0.1, (-60.0, -60.0, 0.0), (60.0, 60.0, 1.0), 0.5
    kmin = np.array([np.floor(lo[k] / res) + 32768 for k in range(3)], np.int32)
    dims = [int(np.floor(hi[k] / res) + 32768 - kmin[k] + 1) for k in range(3)]
    coarse = rng.random((dims[0] // 15 + 1, dims[1] // 15 + 1)) < 0.12            # 1.5 m pillars
    col = np.kron(coarse, np.ones((15, 15), bool))[:dims[0], :dims[1]]
    dist = np.repeat(np.where(col, 0.0, 1.0).astype(np.float32)[:, :, None], dims[2], axis=2)
    dm = oracle.DistMap.from_array(dist, kmin, res)
    ms = L.random_swarm(24, world=lo + hi, seed=8, edt=dist, edt_key_min=kmin, min_clearance=0.5)
    ms.start[:, 2] = ms.goal[:, 2] = np.float32(z2d)
    pl = L.SwarmPlanner(ms, _prior(L, grid_margin=0.05, world_dimension=2, world_z_2d=z2d))
    pl.set_distmap(dist, kmin, res)
    pl.set_goal_trace(2048)
    try:
        longest, most = _against_oracle(L, oracle, ms, pl, dm, 4, grid_margin=0.05, world_dimension=2, world_z_2d=z2d)
        assert pl.goal_trace()["grid_dims"].tolist() == [401, 401, 1]
    finally:
        pl.close()
    assert longest >= 15, longest


def _same_ticks(L, ms, bt, cfgs, ticks, trace=True):
    """Fly every configuration closed loop from the first one's plans; per tick the outputs of all of them."""
    from lsc_planner_amd.planner import next_state_host
    pls = [L.SwarmPlanner(ms, c) for c in cfgs]
    for pl in pls:
        pl.load_octomap(bt)
        if trace:
            pl.set_goal_trace(2048)
    state, traj = start_inputs(ms, pls[0].SEGV)
    out = []
    try:
        for _ in range(ticks):
            tick = []
            for pl in pls:
                g = pl.plan(state, ms.goal, traj)
                tr = pl.goal_trace() if trace else None
                tick.append(dict(g=g, tr=tr, goals=pl.last_goals(), where=pl.goal_storage()))
            out.append(tick)
            traj = tick[0]["g"]["traj"]
            state = next_state_host(traj)
    finally:
        for pl in pls:
            pl.close()
    return out


def _assert_identical(a, b, what):
    for k in ("traj", "status", "cost", "iters"):
        assert np.array_equal(a["g"][k], b["g"][k]), (what, k)
    assert np.array_equal(a["goals"], b["goals"]), what
    if a["tr"] is not None:
        for k in ("flags", "expansions", "path_len"):
            assert np.array_equal(a["tr"][k], b["tr"][k]), (what, k)
        for q, (p, r) in enumerate(zip(a["tr"]["paths"], b["tr"]["paths"])):
            assert np.array_equal(p, r), (what, q)


@pytest.mark.parametrize("which", ["forest", "tiles2"])
def test_hbm_search_equals_the_lds_searches(L, tmp_path, which):
    """goal_search "hbm" against "general" and "auto", tick after tick: paths, flags, expansions, goals, statuses, trajectories."""
    if which == "forest":
        bt, world = _forest_bt(str(tmp_path))
        n, seed, ticks = 40, 4, 10
    else:
        from config_runs import forest_tiles
        bt, world = forest_tiles(2)
        n, seed, ticks = 96, 7, 5
    dist, kmin, r = L.edt_from_bt(bt, np.asarray(world[:3], np.float32), np.asarray(world[3:], np.float32))
    ms = L.random_swarm(n, world=world, seed=seed, edt=dist, edt_key_min=kmin, edt_res=r)
    out = _same_ticks(L, ms, bt, [_prior(L, goal_search=s) for s in ("hbm", "general", "auto")], ticks)
    most = 0
    for t, tick in enumerate(out):
        assert (tick[0]["where"] == 2).all() and (tick[1]["where"] != 2).all()
        assert (tick[0]["g"]["status"] != 5).all()
        for other in tick[1:]:
            _assert_identical(tick[0], other, (which, t))
        most = max(most, int(tick[0]["tr"]["expansions"].max()))
    assert most >= 1000, most


def test_restart_in_hbm_after_an_lds_row_overflow(L, tmp_path):
    """goal_lds_row_cap = 30 on the shipped forest (goal_row_cap = 30 gives status 5 there): the overflowing searches restart with their
    rows in HBM and return what the uncapped search returns."""
    bt, world = _forest_bt(str(tmp_path))
    dist, kmin, r = L.edt_from_bt(bt, np.asarray(world[:3], np.float32), np.asarray(world[3:], np.float32))
    ms = L.random_swarm(16, world=world, seed=4, edt=dist, edt_key_min=kmin, edt_res=r)
    for search in ("auto", "general"):
        out = _same_ticks(L, ms, bt, [_prior(L, goal_search=search), _prior(L, goal_search=search, goal_lds_row_cap=30)], 6)
        where = np.concatenate([tick[1]["where"] for tick in out])
        assert (where == 1).any() and (where == 0).any(), (search, np.bincount(where))
        for t, tick in enumerate(out):
            assert (tick[0]["where"] == 0).all()
            assert (tick[1]["g"]["status"] != 5).all(), (search, t)
            _assert_identical(tick[0], tick[1], (search, t))


def test_batch_mixes_large_and_small_worlds(L, tmp_path, tiled4):
    """lsc_replan_tick_batch over a 4 x 4 tiled context (HBM search), a shipped forest context and an office context with a small LDS
    row capacity (restarts): each context plans the bits it plans alone."""
    from lsc_planner_amd.planner import next_state_host
    bt4, world4, dist4, kmin4, r4 = tiled4
    btf, worldf = _forest_bt(str(tmp_path))
    maps = np.load(os.path.join(GOLDEN, "reference_maps.npz"))
    bto = str(tmp_path / "office.bt")
    with open(bto, "wb") as f:
        f.write(maps["office.bt"].tobytes())
    mo = json.loads(json.load(open(os.path.join(GOLDEN, "testall_missions_20agents.json")))["office"]["multi_random_20agents_2.json"])
    po = tmp_path / "office.json"
    po.write_text(json.dumps(mo))
    distf, kminf, rf = L.edt_from_bt(btf, np.asarray(worldf[:3], np.float32), np.asarray(worldf[3:], np.float32))
    specs = [(L.random_swarm(32, world=world4, seed=3, edt=dist4, edt_key_min=kmin4, edt_res=r4), bt4, _prior(L)),
             (L.random_swarm(20, world=worldf, seed=9, edt=distf, edt_key_min=kminf, edt_res=rf), btf, _prior(L)),
             (L.load_mission(str(po)), bto, _prior(L, goal_lds_row_cap=30))]

    def run(batch, ticks=6):
        pls = []
        for ms, bt, cfg in specs:
            pl = L.SwarmPlanner(ms, cfg)
            pl.load_octomap(bt)
            pls.append(pl)
        st = [list(start_inputs(ms, pl.SEGV)) for (ms, _, _), pl in zip(specs, pls)]
        res = []
        try:
            for _ in range(ticks):
                if batch:
                    for pl in pls:
                        pl.planner_seq += 1
                    outs = L.replan_tick_batch(pls, [s[0] for s in st], [ms.goal for ms, _, _ in specs], [s[1] for s in st],
                                               [pl.planner_seq for pl in pls])
                else:
                    outs = []
                    for pl, (ms, _, _), s in zip(pls, specs, st):
                        g = pl.plan(s[0], ms.goal, s[1])
                        outs.append((g["traj"], g["cost"], g["status"], g["iters"]))
                tick = []
                for pl, s, o in zip(pls, st, outs):
                    tick.append([x.copy() for x in o] + [pl.last_goals(), pl.goal_storage()])
                    s[1] = o[0].copy()
                    s[0] = next_state_host(o[0])
                res.append(tick)
        finally:
            for pl in pls:
                pl.close()
        return res

    solo, bat = run(False), run(True)
    for t, (ta, tb) in enumerate(zip(solo, bat)):
        for m, (ma, mb) in enumerate(zip(ta, tb)):
            for k, (x, y) in enumerate(zip(ma, mb)):
                assert np.array_equal(x, y), f"tick {t} context {m} output {k}"
    where = [np.concatenate([t[m][5] for t in solo]) for m in range(3)]
    assert (where[0] == 2).all() and (where[1] == 0).all() and (where[2] == 1).any()
    assert all((t[m][2] != 5).all() for t in solo for m in range(3))


def test_lsc_sim_on_the_tiled_forest(tmp_path, tiled4):
    """lsc_sim --world tiled.bt: no flag, no capacity report, a result CSV."""
    import lsc_planner_amd as L
    sim = os.path.join(ROOT, "lsc_planner_amd", "lsc_sim")
    assert os.path.exists(sim), "lsc_sim not built (python -c 'import __graft_entry__ as g; g.build()')"
    bt, world, dist, kmin, r = tiled4
    ms = L.random_swarm(16, world=world, seed=31, edt=dist, edt_key_min=kmin, edt_res=r)
    quad = {"max_vel": [1.0, 1.0, 1.0], "max_acc": [2.0, 2.0, 1.0], "radius": 0.15, "nominal_velocity": 1.0, "downwash": 2.0}
    doc = {"quadrotors": {"default": quad}, "world": [{"dimension": list(map(float, world))}], "obstacles": [],
           "agents": [{"type": "default", "start": [float(v) for v in s], "goal": [float(v) for v in g]} for s, g in zip(ms.start, ms.goal)]}
    mpath = tmp_path / "m.json"
    mpath.write_text(json.dumps(doc))
    out = tmp_path / "csv"
    out.mkdir()
    r = subprocess.run([sim, "--mission", str(mpath), "--world", bt, "--max-iter", "30", "--csv", str(out), "--quiet"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "capacity" not in (r.stdout + r.stderr).lower()
    assert any(f.startswith("result_") for f in os.listdir(out)), os.listdir(out)


def test_poison_build_large_worlds():
    """Tests 1, 3 and 4 once more through the LDS-poison build (LDS and the HBM workspace start as 0xff bytes)."""
    lib = os.path.join(ROOT, "lsc_planner_amd", "liblsc_hip_poison.so")
    assert os.path.exists(lib), "liblsc_hip_poison.so not built (make -C lsc_planner_amd/csrc poison)"
    me = os.path.join(ROOT, "tests", "test_gpu_large_world_goals.py")
    ids = [me + "::test_tiled_forest_4x4_against_the_oracle", me + "::test_hbm_search_equals_the_lds_searches",
           me + "::test_restart_in_hbm_after_an_lds_row_overflow"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu"] + ids, env=dict(os.environ, LSC_HIP_LIB=lib), cwd=ROOT,
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "4 passed" in r.stdout, r.stdout[-1000:]
