"""The continuous-time separation certificate (tests/safety_certificate.py) on the CPU: the hull distance against the oracle's GJK and on
degenerate hulls, the certificate on the oracle's own closed loops -- the reference algorithm keeps the promise, tightly, so the
certificate is neither wrong nor vacuous --, and its teeth: a segment moved 1 mm towards its partner, and the pair downwash of a mixed pair
misread as one agent's own, both fail it.

The missions here are the ones tests/test_gpu_safety_certificate.py flies on the GPU: this file is where their premises are held without
one -- nobody excluded (status 0 everywhere), ticks with a pair within 1 mm of touching, and the reference's own shortfall, part (b) of the
bound (tests/tolerances.py).  Run with -s for the figures.
"""
import numpy as np
import pytest

from safety_certificate import NC, hull_distance, pair_certificate, starts_apart, storage_bound
from tolerances import ORACLE_SEPARATION_SHORTFALL, separation_shortfall_bound

TIGHT = 1e-3            # a pair "within 1 mm of touching"


# ------------------------------------------------------------------------------------------------ missions (shared with the GPU file)
def circle(n, radius):
    from harness import circle as harness_circle
    import lsc_planner_amd as L
    return harness_circle(L, n, radius)


def mixed_swarm(n, half, seed=7):
    """random_swarm in a (2 half)^2 x 2.5 m world with radii U(0.1, 0.2) (seed 3) and downwash U(1, 2.5) (seed 4)."""
    import lsc_planner_amd as L
    ms = L.random_swarm(n, world=(-half, -half, 0, half, half, 2.5), seed=seed)
    ms.radius = np.random.default_rng(3).uniform(0.1, 0.2, n)
    ms.downwash = np.random.default_rng(4).uniform(1.0, 2.5, n)
    return ms


def mixed_at_density(n):
    """n mixed agents at the density of the 24-agent mission: one agent per m^3 of the box the sampler draws from (the world shrunk by 0.5 m)."""
    return mixed_swarm(n, (np.sqrt(n / 1.5) + 1.0) / 2.0)


def forest_mission(dist, key_min):
    """12 agents among the trees of the packaged forest.  (Seed 3, the mission of test_oracle_sfc.py, never brings two agents within
    1.6 cm of touching in 45 ticks; seed 7 does within 1 mm at ticks 9 to 12.)"""
    import lsc_planner_amd as L
    return L.random_swarm(12, world=(-5, -5, 0, 5, 5, 2.5), seed=7, edt=dist, edt_key_min=key_min)


FOREST_TICKS = 12
THROUGHPUT_TICKS = 10         # (the first pair within 1 mm comes at tick 8; the first three ticks stay 1.2 mm clear)
BATCH_CIRCLES = (1.2, 1.5, 2.0, 2.5)           # four 8-agent circles of one batched launch

# name: (mission, ticks, oracle keywords, ticks with a pair within 1 mm that the oracle must show at least)
MISSIONS = {
    "circle16_r3.0": (lambda: circle(16, 3.0), 60, {}, 1),
    "circle8_r1.2": (lambda: circle(8, 1.2), 60, {}, 56),
    "mixed48": (lambda: mixed_swarm(48, 3.0, seed=31), 40, {}, 1),
    "mixed24": (lambda: mixed_swarm(24, 2.5), 40, {}, 3),
    "mixed24_bvc": (lambda: mixed_swarm(24, 2.5), 40, dict(planner="bvc"), 0),
    "circle8_r2.0_bvc": (lambda: circle(8, 2.0), 50, dict(planner="bvc"), 47),
    "circle8_r1.2_planar": (lambda: circle(8, 1.2), 60, dict(planar=True), 1),
    "circle8_r1.2_m4": (lambda: circle(8, 1.2), 60, dict(M=4, dt=0.5), 1),
    "circle8_r1.5": (lambda: circle(8, 1.5), 30, {}, 1),
    "circle8_r2.0": (lambda: circle(8, 2.0), 30, {}, 1),
    "circle8_r2.5": (lambda: circle(8, 2.5), 30, {}, 1),
    "forest12": (None, FOREST_TICKS, dict(forest=True), 1),
    "mixed257": (lambda: mixed_at_density(257), THROUGHPUT_TICKS, dict(nthreads=16), 3),
    "mixed512": (lambda: mixed_at_density(512), 2, dict(nthreads=16), 1),
}


class Flight:
    """An oracle closed loop with its certificate: per tick the plans, the statuses and the certificate's worst margin."""

    def __init__(self, ms, M, planar):
        self.ms, self.M, self.planar = ms, M, planar
        self.traj, self.status, self.worst, self.where = [], [], [], []

    def tight_ticks(self):
        return [t + 1 for t, w in enumerate(self.worst) if w < TIGHT]


def fly_oracle(O, name):
    from lsc_planner_amd.planner import next_state_host
    make, ticks, kw, _ = MISSIONS[name]
    M, dt, planar = kw.get("M", 5), kw.get("dt", 0.2), kw.get("planar", False)
    with O.segments(M):
        O.lib()
        dm = None
        if kw.get("forest"):
            from maputil import forest_leaves
            leaves, res = forest_leaves()
            dm = O.DistMap(leaves, res, [-5, -5, 0], [5, 5, 2.5])
            ms = forest_mission(dm.dist, dm.key_min)
        else:
            ms = make()
        prm = O.make_params(dt=dt, world_min=ms.world_min, world_max=ms.world_max, obs_f32=True, use_sfc=dm is not None,
                            **(dict(world_dimension=2, world_z_2d=1.0) if planar else {}))
        agents = (ms.radius, ms.downwash, ms.max_vel, ms.max_acc, ms.nominal_velocity)
        sw = O.SwarmEx(prm, O.make_modes(planner=kw["planner"]), *agents) if "planner" in kw else O.Swarm(prm, *agents)
        if dm is not None:
            sw.set_distmap(dm)
        n = ms.qn
        state = np.zeros((n, 9), np.float32); state[:, :3] = ms.start
        traj = np.zeros((n, 3, NC * M), np.float32)
        f = Flight(ms, M, planar)
        for tick in range(1, ticks + 1):
            o = sw.tick(state, ms.goal, traj, tick, nthreads=kw.get("nthreads", 8))
            c = pair_certificate(o["traj"], ms.radius, ms.downwash, M, status=o["status"], planar=planar)
            f.traj.append(o["traj"]); f.status.append(o["status"]); f.worst.append(c.worst); f.where.append(c.where)
            traj = o["traj"]; state = next_state_host(traj, dt=dt)
            if planar:
                state[:, 2] = 1.0; state[:, 5] = 0.0; state[:, 8] = 0.0
    return f


@pytest.fixture(scope="module")
def flown(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = fly_oracle(oracle, name)
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------------ hull_distance
def test_hull_distance_equals_the_oracles_gjk_on_random_hulls(oracle):
    """200 seeded hulls, a third of them around the origin (distance 0), the others up to a few units off.  The bound: the nearest point is
    evaluated as a weighted sum of at most four vertices and its norm taken -- each a handful of roundings of numbers no larger than the
    hull's farthest vertex R, and an error of the weights along the face moves the distance only in second order --, so both methods are
    within 16 eps R of the truth and within 32 eps R of each other (measured: 1.4e-15, 2.2 eps R)."""
    rng = np.random.default_rng(0)
    P = rng.normal(size=(200, NC, 3)) + (np.arange(200) % 3)[:, None, None] * rng.normal(size=(200, 1, 3))
    h = hull_distance(P)
    g = np.array([oracle.gjk_origin(p)[0] for p in P])
    R = np.linalg.norm(P, axis=2).max(axis=1)
    err = np.abs(h - g)
    print(f"hull_distance vs gjk_origin: worst {err.max():.3g}, worst / (eps R) {(err / (np.finfo(float).eps * R)).max():.3g}; "
          f"{int((g < 1e-12).sum())} hulls hold the origin")
    assert (err <= 32 * np.finfo(float).eps * R).all(), err.max()
    assert (g < 1e-12).sum() >= 20 and (g > 0.5).sum() >= 20


def test_hull_distance_on_degenerate_hulls():
    eps = np.finfo(float).eps
    p = np.array([0.3, -0.4, 1.2])
    assert hull_distance(np.tile(p, (NC, 1))) == pytest.approx(1.3, abs=4 * eps)                        # all six points equal
    # collinear: six points of the line x = 1 in the plane z = 0, the nearest one strictly between two vertices
    line = np.array([[1.0, t, 0.0] for t in (-2.0, -1.0, -0.25, 0.5, 1.5, 3.0)])
    assert hull_distance(line) == pytest.approx(1.0, abs=4 * eps)
    assert hull_distance(line + [0.0, 5.0, 0.0]) == pytest.approx(np.hypot(1.0, 3.0), abs=8 * eps)      # ... and beyond its end: a vertex
    # coplanar: a hexagon in the plane z = 2 over the origin (the face), and moved aside (a vertex)
    th = 2 * np.pi * np.arange(NC) / NC
    hexagon = np.stack([np.cos(th), np.sin(th), np.full(NC, 2.0)], 1)
    assert hull_distance(hexagon) == pytest.approx(2.0, abs=8 * eps)
    edge = np.cos(np.pi / NC)                                                                            # the hexagon's inradius
    assert hull_distance(hexagon + [3.0, 0.0, 0.0]) == pytest.approx(np.hypot(3.0 - 1.0, 2.0), abs=8 * eps)
    assert hull_distance(hexagon * [1, 1, 0]) <= 4 * eps                                                  # planar, around the origin
    assert hull_distance(hexagon * [1, 1, 0] + [0.0, 2.0, 0.0]) == pytest.approx(2.0 - edge, abs=8 * eps)
    # origin inside an octahedron; origin on one of its faces, on an edge and at a vertex
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], float)
    assert hull_distance(octa) <= 4 * eps
    assert hull_distance(octa + np.array([1, 1, 1]) / 3.0) <= 4 * eps                                    # the face x + y + z = 1 ... moved through 0
    assert hull_distance(octa + [0.5, 0.5, 0.0]) <= 4 * eps
    assert hull_distance(octa + [1.0, 0.0, 0.0]) == 0.0
    assert hull_distance(octa + np.array([1, 1, 1]) * (1 / 3.0 + 0.1)) == pytest.approx(0.1 * np.sqrt(3.0), abs=8 * eps)
    # the batch axes are kept
    assert hull_distance(np.stack([octa, hexagon, line]).reshape(3, 1, NC, 3)).shape == (3, 1)


def test_the_box_prefilter_never_certifies_more_than_the_hull():
    """A (pair, segment) certified by its boxes carries the boxes' distance: no larger than the hull's, and beyond r_i + r_j."""
    rng = np.random.default_rng(5)
    n, M = 40, 5
    traj = (rng.uniform(-3, 3, (n, 3, 1, 1)) + 0.3 * rng.normal(size=(n, 3, M, NC))).reshape(n, 3, M * NC)
    r, dw = rng.uniform(0.1, 0.2, n), rng.uniform(1.0, 2.5, n)
    full, fast = pair_certificate(traj, r, dw, M, prefilter=False), pair_certificate(traj, r, dw, M, prefilter=True)
    assert full.boxed == 0 and 0 < fast.boxed < fast.margin.size
    boxed = fast.margin != full.margin
    assert boxed.sum() == fast.boxed
    assert (fast.margin[boxed] > 0.01).all() and (fast.margin[boxed] <= full.margin[boxed] + 1e-12).all()
    assert (fast.worst, fast.where) == (full.worst, full.where)


def test_agents_without_a_plan_are_masked_and_counted():
    traj = np.zeros((4, 3, 30))
    traj[:, 0] = np.arange(4)[:, None] * 0.25                   # hovering 0.25 m apart: neighbours overlap at r = 0.15
    r, dw = np.full(4, 0.15), np.full(4, 2.0)
    c = pair_certificate(traj, r, dw, 5)
    assert c.excluded_agents == 0 and c.excluded_pairs == 0 and c.worst == pytest.approx(-0.05) and c.where == (0, 1, 0)
    c = pair_certificate(traj, r, dw, 5, status=[0, 1, 0, 0])
    assert c.excluded_agents == 1 and c.excluded_pairs == 3 and c.margin.count() == 3 * 5
    assert c.worst == pytest.approx(-0.05) and c.where == (2, 3, 0)                                      # 1-2 is masked, 2-3 is not
    assert c.of_pair(3, 0).min() == pytest.approx(0.45)
    c = pair_certificate(traj, r, dw, 5, status=[0, 1, 0, 3])
    assert c.excluded_agents == 2 and c.worst == pytest.approx(0.2) and c.where == (0, 2, 0)


def test_the_planar_certificate_ignores_z_and_the_downwash_divides_it():
    traj = np.zeros((2, 3, 30))
    traj[1, 0] = 0.4; traj[1, 2] = 0.8
    r = np.full(2, 0.15)
    assert pair_certificate(traj, r, [2.0, 2.0], 5).worst == pytest.approx(np.hypot(0.4, 0.4) - 0.3)
    assert pair_certificate(traj, r, [1.0, 3.0], 5).worst == pytest.approx(np.hypot(0.4, 0.4) - 0.3)      # equal radii: the mean
    assert pair_certificate(traj, [0.1, 0.2], [1.0, 4.0], 5).worst == pytest.approx(np.hypot(0.4, 0.8 / 3.0) - 0.3)
    assert pair_certificate(traj, r, [2.0, 2.0], 5, planar=True).worst == pytest.approx(0.1)


def test_storage_bound_of_a_world_box():
    """+-5 m x +-5 m x 0..2.5 m: float32 ulps 2^-21, 2^-21 and 2^-22 at the extent; z through a downwash of 2."""
    want = np.sqrt(2 * 2.0 ** -42 + (2.0 ** -22 / 2.0) ** 2)
    assert storage_bound([-5, -5, 0], [5, 5, 2.5], [2.0, 2.5]) == pytest.approx(want, rel=1e-12)
    assert want == pytest.approx(6.85e-7, rel=1e-3)
    assert separation_shortfall_bound([-5, -5, 0], [5, 5, 2.5], [2.0]) == pytest.approx(want + ORACLE_SEPARATION_SHORTFALL, rel=1e-12)


# ------------------------------------------------------------------------------------------------ the oracle's closed loops
@pytest.mark.parametrize("name", list(MISSIONS))
def test_the_oracles_plans_keep_the_promise_and_tightly(flown, name):
    """Every mission of the certificate tests, flown by the oracle: the starts are apart (the premise of the induction), no agent ever
    fails its QP (nobody is excluded), every pair's every segment is certified down to the reference's own shortfall -- part (b) of the
    bound, measured here and nowhere else --, and the mission has ticks with a pair within 1 mm of touching."""
    f = flown(name)
    ms = f.ms
    assert starts_apart(ms.start, ms.radius, ms.downwash) >= 0.0
    bad = sum(int((s != 0).sum()) for s in f.status)
    tight = f.tight_ticks()
    t = int(np.argmin(f.worst))
    print(f"{name}: worst dist - (r_i + r_j) {f.worst[t]:+.3g} m at tick {t + 1}, (i, j, segment) {f.where[t]}; {len(tight)} of {len(f.worst)} "
          f"ticks with a pair within 1 mm: {tight}; agent-ticks with status != 0: {bad}; storage bound "
          f"{storage_bound(ms.world_min, ms.world_max, ms.downwash):.3g} m")
    assert bad == 0
    assert min(f.worst) >= -ORACLE_SEPARATION_SHORTFALL, (min(f.worst), f.where[t])
    assert len(tight) >= MISSIONS[name][3], tight


# ------------------------------------------------------------------------------------------------ teeth
TEETH_TICK = 30                 # of circle8_r1.2: every pair of neighbours within 1 mm from tick 5 on


def test_a_segment_moved_one_millimetre_towards_its_partner_fails(flown):
    f = flown("circle8_r1.2")
    ms, traj = f.ms, f.traj[TEETH_TICK - 1].astype(np.float64)
    bound = separation_shortfall_bound(ms.world_min, ms.world_max, ms.downwash)
    c = pair_certificate(traj, ms.radius, ms.downwash, 5)
    i, j, m = c.where
    assert -bound <= c.worst < TIGHT
    cp = traj.reshape(8, 3, 5, NC)
    # towards the partner: along the nearest point of the hull of the differences, found here by the gradient of the distance
    D = np.moveaxis(cp[i, :, m] - cp[j, :, m], 0, 1) / [1, 1, 2.0]
    step, grad = 1e-6, np.zeros(3)
    for k in range(3):
        e = np.zeros(3); e[k] = step
        grad[k] = (hull_distance(D + e) - hull_distance(D - e)) / (2 * step)
    grad /= np.linalg.norm(grad)
    moved = cp.copy()
    moved[i, :, m] -= (1e-3 * grad * [1, 1, 2.0])[:, None]
    c2 = pair_certificate(moved.reshape(8, 3, 30), ms.radius, ms.downwash, 5)
    assert c2.where == (i, j, m) and c2.worst == pytest.approx(c.worst - 1e-3, abs=2e-5), (c2.where, c2.worst)
    assert c2.worst < -bound
    # ... for that pair and segment, and for nothing the move did not touch (the agent's other tight neighbour in that segment may fail too)
    failing = [(int(c2.i[p]), int(c2.j[p]), int(s)) for p, s in np.argwhere(c2.margin < -bound)]
    assert (i, j, m) in failing and all(i in (a, b) and s == m for a, b, s in failing), failing


MISREAD_TICK, MISREAD_PAIR, MISREAD_OWN = 11, (15, 21), 21      # of mixed24: downwash 1.55 and 2.41, radii 0.15 and 0.11


def test_the_pair_downwash_misread_as_the_agents_own_fails(flown):
    """The misreading the certificate exists for: agent 21 scaling z by its own downwash (2.41) where the pair's is the radius-weighted mean
    (1.92).  Plans made under the one rule are not safe under the other -- tick 11 of the 24 mixed agents: the pair (15, 21) is 1.1 mm clear
    as the reference reads it and 4.3 cm inside each other as the misreading does --, so a kernel and an oracle that shared the misreading
    would fail the certificate where they agree with each other."""
    f = flown("mixed24")
    ms, traj = f.ms, f.traj[MISREAD_TICK - 1]
    bound = separation_shortfall_bound(ms.world_min, ms.world_max, ms.downwash)
    i, j = MISREAD_PAIR
    assert abs(ms.downwash[i] - ms.downwash[j]) > 0.5
    right = pair_certificate(traj, ms.radius, ms.downwash, 5)
    assert 0.0 <= right.of_pair(i, j).min() < 2e-3 and right.worst >= -bound
    dw = ms.downwash.copy()
    dw[[k for k in MISREAD_PAIR if k != MISREAD_OWN]] = ms.downwash[MISREAD_OWN]        # the mean of two equal values: the agent's own
    wrong = pair_certificate(traj, ms.radius, dw, 5)
    print(f"pair {MISREAD_PAIR} at tick {MISREAD_TICK}: {right.of_pair(i, j).min():+.3g} m by the pair's downwash, "
          f"{wrong.of_pair(i, j).min():+.3g} m by agent {MISREAD_OWN}'s own")
    assert wrong.of_pair(i, j).min() < -1e-2 and wrong.worst < -bound
