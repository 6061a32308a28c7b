"""The inequality the neighbour lists of large swarms rest on (lsc_planner_amd/csrc/lsc_neigh.hip), checked numerically on the CPU:
the sphere test of the grid query keeps every (obstacle, segment) unit that phase B's own pre-cull keeps (lsc_kernels.hip,
"spatial pre-cull"), whatever the control points, the downwash and the reach B_m are.  (That the pre-cull in turn keeps every unit with a
row the exact per-row test keeps -- the test's box lies inside the pre-cull's sphere -- is checked on the GPU by prune = 1 against
prune = 3, bit for bit.  That the exact per-row test itself drops redundant rows only is proven by LP in tests/test_prune_soundness.py, and
every kernel's copy of it is held by its row counts in tests/test_gpu_prune_rule.py.)"""
import numpy as np

from neighbour_reference import reach_closed_form_f32, reach_sums, unit_test_keeps as _unit_test_keeps, unit_test_keeps_all

F = np.float32


def _sphere(points):
    """lsc_neigh_build_kernel: float32; centre = mean, radius around the stored centre, rounded up by 1e-5 r + 1e-5"""
    pts = points.astype(F)
    c = (pts.sum(axis=0, dtype=F) * F(1.0 / 6.0)).astype(F)
    d = pts - c
    rad = F(np.sqrt((d * d).sum(axis=1, dtype=F).max())) * F(1.0 + 1e-5) + F(1e-5)
    return c, F(rad)


def _sphere_test_keeps(ca, ra, co, ro, idw, B, r):
    """lsc_neigh_query_kernel: float32; keep unless |S (C_a - C_o)| >= (s (2 B + 3 (rho_a + rho_o)) + r) (1 + 2e-5) + 5e-4, with B as the
    build kernel stores it (rounded up by 1e-5 B + 1e-3)"""
    idw, r = F(idw), F(r)
    Bf = F(B) * F(1.0 + 1e-5) + F(1e-3)
    d = (ca - co) * np.array([1.0, 1.0, idw], F)
    need = (max(F(1.0), idw) * (F(2.0) * Bf + F(3.0) * (ra + ro)) + r) * F(1.0 + 2e-5) + F(5e-4)
    return not (F((d * d).sum(dtype=F)) >= need * need)


def test_sphere_test_of_the_grid_query_keeps_what_the_unit_test_keeps():
    rng = np.random.default_rng(6)
    kept_unit = kept_sphere = 0
    for trial in range(12000):
        scale = rng.choice([0.05, 0.3, 1.0, 3.0])
        p = (rng.normal(size=3) * 3 + rng.normal(size=(6, 3)) * scale * rng.uniform(0, 1)).astype(np.float32).astype(np.float64)
        off = rng.normal(size=3) * rng.choice([0.5, 2.0, 6.0])
        q = (p.mean(axis=0) + off + rng.normal(size=(6, 3)) * scale * rng.uniform(0, 1)).astype(np.float32).astype(np.float64)
        idw = 1.0 / rng.choice([0.5, 1.0, 2.0, 3.7])
        B = rng.uniform(0.0, 2.5)
        r = rng.uniform(0.1, 0.6)
        ku = _unit_test_keeps(p, q, idw, B, r)
        ca, ra = _sphere(p)
        co, ro = _sphere(q)
        ks = _sphere_test_keeps(ca, ra, co, ro, idw, B, r)
        assert ks or not ku, (trial, p, q, idw, B, r)
        kept_unit += ku
        kept_sphere += ks
    assert 0.2 < kept_unit / 12000 < 0.9 and kept_sphere >= kept_unit          # the trials straddle the bound
    assert kept_sphere < 1.4 * kept_unit                                       # ... which is not much looser than the test it replaces


def test_vectorised_unit_test_is_the_scalar_one():
    """tests/neighbour_reference.py states phase B's pre-cull twice, one unit at a time and for all units of an agent: the same decisions."""
    rng = np.random.default_rng(7)
    n, m = 40, 5
    p = rng.normal(size=(m, 6, 3)) * 0.4
    Q = p[None] + rng.normal(size=(n, 1, 1, 3)) * 2.5 + rng.normal(size=(n, m, 6, 3)) * 0.3
    idw, B, r = 1.0 / rng.choice([0.5, 1.0, 2.0, 3.7], n), rng.uniform(0.0, 1.5, m), rng.uniform(0.2, 0.6, n)
    keep = unit_test_keeps_all(p, Q, idw, B, r)
    want = np.array([[_unit_test_keeps(p[k], Q[o, k], idw[o], B[k], r[o]) for k in range(m)] for o in range(n)])
    assert np.array_equal(keep, want) and 0 < keep.sum() < keep.size


def test_closed_form_reach_dominates_the_sums_of_phase_b():
    """The build kernel's closed form of the reach (reach_hi / reach_lo: float32, the number of unclamped steps by a floor) against the
    running sums phase B forms in float64 (S.reachL / reachU), for K = 1..27: with the pads B_m carries -- 1e-5 of itself + 1e-3 -- the
    closed form is never below the sums, and the two differ by rounding only.  Draws: |v| and |a| up to 1.4 times their limits, v exactly
    at +-vmax, a = 0 (measured: smallest slack 1.0e-3, the pad itself; largest difference 3.7e-7)."""
    rng = np.random.default_rng(20)
    n, dt = 20000, 0.2
    vmax, amax = rng.uniform(0.3, 2.5, n), rng.uniform(0.5, 6.0, n)
    v, a = rng.uniform(-1.4, 1.4, n) * vmax, rng.uniform(-1.4, 1.4, n) * amax
    v[:2000] = np.where(rng.random(2000) < 0.5, -1.0, 1.0) * vmax[:2000]
    a[1000:4000] = 0.0
    v, a = v.astype(F), a.astype(F)                                   # (the state is float32)
    hv, ha = dt / 5, dt * dt / 20
    d0_32 = (v * F(hv) + a * F(ha)).astype(F)
    d0_64 = v.astype(np.float64) * hv + a.astype(np.float64) * ha
    e32 = reach_closed_form_f32(d0_32, (vmax * hv).astype(F), (amax * ha).astype(F)).astype(np.float64)
    e64 = reach_sums(d0_64, vmax * hv, amax * ha)[..., 1:]
    print("closed form against sums: smallest slack", (e32 * (1 + 1e-5) + 1e-3 - e64).min(), "largest difference", np.abs(e32 - e64).max())
    assert (e32 * (1.0 + 1e-5) + 1e-3 >= e64).all()
    assert (np.abs(e32 - e64) <= 1e-5 * e64 + 1e-6).all(), np.abs(e32 - e64).max()
