"""The corridor kernel's per-axis cell rule (rule_sfc_axis_cells, csrc/lsc_rules.hpp), compiled for the host (tests/native/sfc_host_check.cpp),
against the reference's literal lattice samples (include/corridor_constructor.hpp:81-122) -- without a GPU.

The kernel answers a slab from an integral image, so per axis it needs the visited cells as one cell a0 plus one contiguous range [b0, b1].
The reference visits floor(rf * float(float(lo + j res) +- 1e-5f)) for j = 0 .. max(size, 2) - 1, one float at a time.  The two are the same
set only while the nudge survives the float32 addition: below 256 m.  That bound is what lsc_set_distmap refuses worlds at; this test holds
it by the product's own text: every lattice index and every slab length, the first disagreement at or beyond SFC_WORLD_REACH_MAX."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

RESOLUTIONS = (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.5)
WALK_TO = 300.0            # metres: beyond the bound, to see the disagreement that the bound keeps out
KMIN = 32768 - 7000        # key of the field's cell 0 (any value: it shifts both sides alike)


def _host_check():
    so = os.path.join(ROOT, "tests", "native", "libsfc_host_check.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.dirname(so)])
    H = ctypes.CDLL(so)
    H.sfchdr_world_reach_max.restype = ctypes.c_double
    return H


def _kernel_cells(H, lo, hi, res, wmin):
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    lo, hi, wmin = (np.ascontiguousarray(a, np.float64) for a in (lo, hi, wmin))
    out = np.zeros((len(lo), 3), np.int32)
    H.sfchdr_axis_cells(len(lo), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), ctypes.c_double(res), ctypes.c_double(1.0 / res), KMIN,
                        wmin.ctypes.data_as(dp), out.ctypes.data_as(ip))
    return out


def _literal_cells(lo, size, res, wmin):
    """The cells isObstacleInBox visits along one axis, [n][max(size, 2)]: box_iter = 0 .. max(size, 2) - 1, search_point and delta in float32."""
    n = max(size, 2)
    j = np.arange(n, dtype=np.float64)[None, :]
    sp = (lo[:, None] + j * res).astype(np.float32)                             # search_point(i) = box[i] + box_iter[i] * resolution
    if size == 1:
        sp[:, 1:] = lo[:, None].astype(np.float32)                              # box_size == 1 and box_iter > 0: box[i]
    delta = np.full(sp.shape, np.float32(1e-5), np.float32)
    delta[:, 0] = np.where(lo > wmin + 1e-5, np.float32(-1e-5), np.float32(1e-5))
    sample = sp + delta                                                         # float32 + float32
    assert sample.dtype == np.float32
    return np.floor((1.0 / res) * sample.astype(np.float64)).astype(np.int64) + 32768 - KMIN


def _disagree(cells, abc):
    """Rows where the literal set of cells is not {a0} u [b0, b1]."""
    a0, b0, b1 = (abc[:, k].astype(np.int64) for k in range(3))
    inside = (cells == a0[:, None]) | ((cells >= b0[:, None]) & (cells <= b1[:, None]))
    s = np.sort(cells, axis=1)
    distinct = 1 + (np.diff(s, axis=1) != 0).sum(axis=1)
    a_apart = (a0 < b0) | (a0 > b1)
    want = (b1 - b0 + 1) + a_apart
    lo_k = np.minimum(a0, b0)
    hi_k = np.maximum(a0, b1)
    return ~(inside.all(axis=1) & (distinct == want) & (s[:, 0] == lo_k) & (s[:, -1] == hi_k))


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_axis_cells_equal_the_literal_samples_below_256_m(res):
    H = _host_check()
    bound = H.sfchdr_world_reach_max()
    assert bound == 256.0
    K = int(np.ceil(WALK_TO / res))
    k = np.arange(-K, K + 1, dtype=np.float64)
    lo = k * res
    first, beyond = np.inf, 0
    for size in range(1, 13):                                                   # lattice points of the slab
        hi = lo + (size - 1) * res
        reach = np.maximum(np.abs(lo), np.abs(hi))                              # the slab's farthest lattice point
        for wmin in (np.full(len(lo), -1e9), lo.copy()):                        # a box inside the world, a box on the world's boundary
            bad = _disagree(_literal_cells(lo, size, res, wmin), _kernel_cells(H, lo, hi, res, wmin))
            if bad.any():
                first = min(first, reach[bad].min())
                beyond += int(bad.sum())
            assert not bad[reach < bound].any(), (res, size, lo[bad & (reach < bound)][:5])
    print(f"res {res}: first disagreement at {first:.4f} m, {beyond} slabs between there and {WALK_TO} m")
    assert first >= bound, (res, first)
    # ... and the bound is not idle: where the lattice points are no float32 numbers themselves (0.25 k and 0.5 k are, and never lose their
    # cell) the two rules part ways within the first metre beyond it
    if res not in (0.25, 0.5):
        assert first < bound + 1.0, (res, first)
