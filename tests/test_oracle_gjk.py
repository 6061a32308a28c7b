"""Oracle GJK restatement vs. the reference's own openGJK (golden vectors generated from oracle/_ref)."""
import ctypes
import os

import numpy as np


def test_oracle_gjk_matches_reference_golden_bitwise(oracle, gjk_golden):
    pts = gjk_golden["pts"].astype(np.float64)
    for i in range(len(pts)):
        d, v, nv, it = oracle.gjk_origin(pts[i])
        assert d == gjk_golden["dist"][i]
        assert np.array_equal(v, gjk_golden["v"][i])
        assert nv == gjk_golden["nvrtx"][i]


def test_oracle_gjk_live_against_reference_build(oracle):
    """Live where oracle/_ref was built (it is kept out of git: the reference's GPLv3 openGJK does not travel); elsewhere against that
    build's answers on the same 3000 hulls, stored in tests/golden/gjk_live_vectors.npz (tests/golden/make_gjk_live_golden.py)."""
    rng = np.random.default_rng(5)
    hulls = [(rng.normal(size=(6, 3)) * (0.2 + (t % 5))).astype(np.float32).astype(np.float64) for t in range(3000)]
    ref = oracle.ref_gjk_lib()
    if ref is None:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gjk_live_vectors.npz"))
        assert np.array_equal(z["pts"].astype(np.float64), np.asarray(hulls))       # the stored answers are for exactly these hulls
        for i, p in enumerate(hulls):
            d1, v1, n1, _ = oracle.gjk_origin(p)
            assert d1 == z["dist"][i] and np.array_equal(v1, z["v"][i]) and n1 == z["nvrtx"][i]
        return
    zero = np.zeros(3)
    dp = ctypes.POINTER(ctypes.c_double)
    saved = os.dup(1); devnull = os.open(os.devnull, os.O_WRONLY); os.dup2(devnull, 1)
    try:
        for p in hulls:
            v2 = np.zeros(3); n2 = ctypes.c_int()
            d2 = ref.ref_gjk(p.ctypes.data_as(dp), 6, zero.ctypes.data_as(dp), 1, v2.ctypes.data_as(dp), ctypes.byref(n2))
            d1, v1, n1, _ = oracle.gjk_origin(p)
            assert d1 == d2 and np.array_equal(v1, v2) and n1 == n2.value
    finally:
        os.dup2(saved, 1); os.close(devnull); os.close(saved)


def test_gjk_geometry_properties(oracle):
    """Witness is the closest hull point: inside-origin -> 0, single point -> the point, and v.(p - v) >= 0."""
    rng = np.random.default_rng(11)
    p = np.tile(np.array([0.3, -0.2, 0.1]), (6, 1))
    d, v, nv, _ = oracle.gjk_origin(p)
    assert np.allclose(v, p[0]) and nv == 1
    for _ in range(200):
        pts = rng.normal(size=(6, 3)) + np.array([2.5, 0, 0])
        d, v, nv, _ = oracle.gjk_origin(pts)
        assert abs(np.linalg.norm(v) - d) < 1e-12
        assert ((pts - v) @ v >= -1e-9).all()       # supporting-plane optimality condition
    cube = np.array([[1, 1, 1], [-1, -1, 1], [-1, 1, -1], [1, -1, -1], [1, 1, -1], [-1, -1, -1]], float)
    d, v, nv, _ = oracle.gjk_origin(cube)
    assert d < 1e-9


def test_tetra_edge_fall_backs_oracle_and_host_header_vs_reference_bitwise(oracle):
    """Two statements of reduce_tetra (csrc/lsc_gjk.hpp) -- the set_edge fall-backs of the `nface == 1`, `nkeep == 2` arms -- are reached
    by none of the 27 000 hulls of the tests above.  tests/golden/gjk_tetra_edges.npz holds 16 hulls for each, found by search, with the
    answers of the reference's own openGJK (tests/golden/make_gjk_tetra_edges.py): the oracle and the device header compiled for the
    host give them bit for bit, and where oracle/_ref is built the reference gives them again."""
    import subprocess
    from golden.make_gjk_tetra_edges import hulls
    here = os.path.dirname(os.path.abspath(__file__))
    z = np.load(os.path.join(here, "golden", "gjk_tetra_edges.npz"))
    pts32, statement = hulls()
    assert np.array_equal(z["pts"].view(np.uint32), pts32.view(np.uint32)) and np.array_equal(z["statement"], statement)
    assert np.bincount(statement).tolist() == [16, 16]
    pts = np.ascontiguousarray(z["pts"].astype(np.float64))
    n = len(pts)
    for i in range(n):
        d, v, nv, _ = oracle.gjk_origin(pts[i])
        assert d == z["dist"][i] and np.array_equal(v, z["v"][i]) and nv == z["nvrtx"][i], i
    so = os.path.join(here, "native", "libgjk_host_check.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.dirname(so)])
    H = ctypes.CDLL(so)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    v = np.zeros((n, 3)); d = np.zeros(n); nv = np.zeros(n, np.int32)
    H.gjkhdr_batch(pts.ctypes.data_as(dp), n, v.ctypes.data_as(dp), d.ctypes.data_as(dp), nv.ctypes.data_as(ip))
    assert np.array_equal(d, z["dist"]) and np.array_equal(v, z["v"]) and np.array_equal(nv, z["nvrtx"])
    # every hull ends on an edge or a triangle next to its newest vertex: none has the origin inside, none ends on a vertex
    assert set(np.unique(z["nvrtx"]).tolist()) <= {2, 3} and (z["dist"] > 0).all()
    ref = oracle.ref_gjk_lib()
    if ref is not None:
        zero = np.zeros(3)
        saved = os.dup(1); devnull = os.open(os.devnull, os.O_WRONLY); os.dup2(devnull, 1)
        try:
            for i in range(n):
                v2 = np.zeros(3); n2 = ctypes.c_int()
                d2 = ref.ref_gjk(pts[i].ctypes.data_as(dp), 6, zero.ctypes.data_as(dp), 1, v2.ctypes.data_as(dp), ctypes.byref(n2))
                assert d2 == z["dist"][i] and np.array_equal(v2, z["v"][i]) and n2.value == z["nvrtx"][i], i
        finally:
            os.dup2(saved, 1); os.close(devnull); os.close(saved)
