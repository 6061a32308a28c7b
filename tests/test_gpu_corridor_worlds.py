"""-m gpu: the corridor kernel (sfc_expand / sfc_blocked, csrc/lsc_kernels.hip) on every kind of world the host accepts, and the host's
refusal of the worlds beyond.

The kernel is the one stage that replaces the reference's algorithm: per axis it turns the nudged lattice samples of a slab into one cell
a0 plus one contiguous range [b0, b1] and answers the slab from an integral image.  The other corridor tests all fly world_resolution
0.1, bounds on the lattice within +-5 m (+-60 m) and real distance fields, whose obstacles are several cells thick.  Here the field is
synthetic (tests/corridor_worlds.py): 0 in an occupied voxel, 1.0 elsewhere, so a single cell blocks and one cell more or less in a slab
test changes a box.

Pattern of test_sfc_box_growth_bitwise_on_random_seeds: one context per world, N agents as N independent seeds, static goals, one
first-tick plan(); every box against the oracle's literal loops.  No tolerance anywhere: float32 words are compared as integers.
"""
import numpy as np
import pytest

import corridor_worlds as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    L.load_library()
    return L


def _context(L, w, use_octomap=True):
    N = w.N
    ms = L.Mission(w.start, w.goal, w.wmin, w.wmax, np.full(N, w.radius), np.full(N, 2.0), np.ones((N, 3)), np.full((N, 3), 2.0), np.ones(N))
    return L.SwarmPlanner(ms, L.PlannerConfig(use_octomap=use_octomap, world_resolution=w.res, goal_mode="static"))


def fly(L, w):
    """First-tick corridor boxes of the world's seeds on the device: (status [N], sfc [N][M][6])."""
    pl = _context(L, w)
    try:
        pl.set_distmap(w.dist, w.key_min, w.res)
        state = np.zeros((w.N, 9), np.float32); state[:, :3] = w.start
        g = pl.plan(state, w.goal, np.zeros((w.N, 3, 30), np.float32))
    finally:
        pl.close()
    return g["status"], g["sfc"]


def mismatches(status, sfc, rc, box):
    """Seeds whose verdict or box differs from the oracle's: (verdicts that differ, accepted boxes that differ, accepted seeds)."""
    verdict = int(((status == 4) != (rc != 0)).sum())
    ok = (rc == 0) & (status != 4)
    differ = (sfc[:, 0].view(np.uint32) != box.view(np.uint32)).any(axis=1) & ok
    return verdict, int(differ.sum()), int(ok.sum())


def check(L, O, w, random_world=True):
    rc, box = W.oracle_boxes(O, w)
    status, sfc = fly(L, w)
    rejected = int((rc != 0).sum())
    print(f"{w.name}: {w.N} seeds, oracle verdicts 0/1/2 = {[int((rc == v).sum()) for v in (0, 1, 2)]}")
    assert np.array_equal(status == 4, rc != 0), (w.name, np.flatnonzero((status == 4) != (rc != 0)))
    ok = rc == 0
    got, want = sfc[ok, 0].view(np.uint32), box[ok].view(np.uint32)
    assert np.array_equal(got, want), (w.name, np.flatnonzero(ok)[(got != want).any(axis=1)], sfc[ok, 0][(got != want).any(axis=1)],
                                       box[ok][(got != want).any(axis=1)])
    for m in range(1, sfc.shape[1]):                                   # flag_initialize_sfc: the first box fills the whole history
        assert np.array_equal(sfc[ok, m].view(np.uint32), want), (w.name, m)
    if random_world:
        assert 0 < rejected < w.N // 2, (w.name, rejected)
    return rc, box


@pytest.mark.parametrize("res,seed", [(0.05, 1), (0.2, 2), (0.25, 3), (0.15, 4)])
def test_resolutions_and_the_seed_snapping_branch(L, oracle, res, seed):
    """world_resolution = map resolution other than 0.1, with seeds either side of the 0.01 m snap (and exactly on the lattice)."""
    w = W.resolution_world(res, seed)
    off = np.abs(w.start[:44].astype(np.float64) - np.round(w.start[:44].astype(np.float64) / res) * res)
    assert (off < 0.01).sum() > 40 and (off >= 0.01).sum() > 20        # both branches of :25, per axis
    check(L, oracle, w)


def test_world_bounds_off_the_lattice(L, oracle):
    w = W.off_lattice_world(5)
    rc, box = check(L, oracle, w)
    ok = rc == 0
    # no face beyond the world, and some box on the last lattice plane inside each face
    assert (box[ok, :3] >= w.wmin - np.float32(0.1)).all() and (box[ok, 3:] <= w.wmax + np.float32(0.1)).all()
    assert (rc[:48] == 2).any() and (rc[:48] == 0).any()                # seeds next to a face: boxes that start outside it, and boxes that do not


def test_field_larger_than_the_world(L, oracle):
    """Seeds inside the field but outside the world: `return 2` (the reference's loop never runs: undefined there, refused here), next to
    seeds whose box touches an obstacle, `return 1`.  Status 4 for both."""
    w = W.field_larger_than_world(6)
    rc, _ = check(L, oracle, w)
    assert (rc[:24] == 2).sum() >= 16 and (rc[24:] == 1).any() and not (rc[24:] == 2).any()


def test_empty_field_every_box_is_the_world(L, oracle):
    """128 cells along x and y: whole rounds in which all 64 speculative steps pass (fm == 0), the fresh / not-fresh hand-over between
    rounds, and every ncand from 6 down to 1 as the faces reach the world's one after the other.  The answer is known without the oracle."""
    w = W.empty_world()
    rc, box = check(L, oracle, w, random_world=False)
    assert (rc == 0).all()
    world = np.concatenate([w.wmin, w.wmax]).astype(np.float32)
    assert np.array_equal(box.view(np.uint32), np.tile(world, (w.N, 1)).view(np.uint32))     # (and check() held the device's boxes to these)


def test_goal_ties_in_the_axis_order(L, oracle):
    w = W.goal_tie_world(7)
    d = W.goal_deltas(w)
    kind = np.arange(w.N) % 4
    ad = np.abs(d)
    two_equal = (ad[:, 0] == ad[:, 1]) | (ad[:, 1] == ad[:, 2]) | (ad[:, 0] == ad[:, 2])
    assert (d[kind == 0] == 0).all()
    assert (two_equal & (ad > 0).all(axis=1))[kind == 1].sum() >= 16    # (float32: not every constructed tie survives the addition)
    assert ((d == 0).sum(axis=1) == 1)[kind == 2].sum() >= 24
    assert (d[kind == 3] < 0).all()
    check(L, oracle, w)


@pytest.mark.parametrize("res,seed", [(0.1, 8), (0.2, 9)])
def test_far_from_the_origin_inside_the_bound(L, oracle, res, seed):
    """World centred at x = 250 m, y = -200 m: accepted by lsc_set_distmap (max |bound| + res < 256) and bit-equal."""
    check(L, oracle, W.far_world(res, 250.0, seed))


def test_thin_world_three_cells_high(L, oracle):
    w = W.thin_world(10)
    rc, box = check(L, oracle, w)
    assert (rc[:24] == 0).any()                                         # seeds on the floor grow
    assert (rc[24:48] != 0).all()                                       # on the ceiling the upper sample leaves the field: getDistance() = -1
    assert (rc[48:] == 0).sum() > 30


def _tiny(L, res, wmin, wmax, use_octomap=True):
    """A context over the given world with two agents and a 4 x 4 x 4 field at the world's lower corner (the host checks need no more)."""
    wmin, wmax = np.asarray(wmin, np.float64), np.asarray(wmax, np.float64)
    mid = 0.5 * (wmin + wmax)
    pos = np.stack([mid - [1.0, 0, 0], mid + [1.0, 0, 0]])
    w = W.World("tiny", res, wmin, wmax, pos, pos[::-1], density=0.0, fmin=wmin, fmax=wmin + 3 * res, radius=0.15)
    return w, _context(L, w, use_octomap)


def test_worlds_beyond_256_m_are_refused(L):
    """From |x| >= 256 m the float32 step (3.05e-5 m) is more than twice the reference's 1e-5 nudge: `float(x) + 1e-5f` rounds back to
    float(x), the reference's samples skip cells, and the kernel's contiguous [b0, b1] tests cells the reference never visits (measured:
    tests/test_sfc_axis_cells.py on the host; on the device, differing boxes at x = 300 m).  lsc_set_distmap refuses such worlds."""
    for res, cx in ((0.1, 300.0), (0.2, 300.0), (0.1, -300.0)):
        w = W.far_world(res, cx, 8)
        pl = _context(L, w)
        with pytest.raises(L.LscError, match="256"):
            pl.set_distmap(w.dist, w.key_min, w.res)
        pl.close()
    # the bound is max(|world_min|, |world_max|) + world_resolution < 256 on every axis
    for wmin, wmax, refused in (((250.0, -2.0, 0.0), (255.95, 2.0, 2.0), True), ((250.0, -2.0, 0.0), (255.8, 2.0, 2.0), False),
                                ((-2.0, -255.95, 0.0), (2.0, -250.0, 2.0), True), ((-2.0, -2.0, 250.0), (2.0, 2.0, 255.8), False)):
        w, pl = _tiny(L, 0.1, wmin, wmax)
        if refused:
            with pytest.raises(L.LscError, match="256"):
                pl.set_distmap(w.dist, w.key_min, w.res)
        else:
            pl.set_distmap(w.dist, w.key_min, w.res)
        pl.close()
    # without use_octomap no corridor is grown: the field is taken as before
    w, pl = _tiny(L, 0.1, (296.0, -2.0, 0.0), (304.0, 2.0, 2.0), use_octomap=False)
    pl.set_distmap(w.dist, w.key_min, w.res)
    pl.close()


def test_more_than_3400_steps_per_axis_are_refused(L):
    """20 m at resolution 0.005: 4000 steps, more than the face tables hold in LDS."""
    w, pl = _tiny(L, 0.005, (-10.0, 0.0, 1.0), (10.0, 0.1, 1.1))
    pl.set_distmap(w.dist, w.key_min, w.res)
    state = np.zeros((2, 9), np.float32); state[:, :3] = w.start
    with pytest.raises(L.LscError, match="3400"):
        pl.plan(state, w.goal, np.zeros((2, 3, 30), np.float32))
    pl.close()
