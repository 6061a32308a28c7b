"""The reference's openGJK on the 3000 seeded hulls of tests/test_oracle_gjk.py::test_oracle_gjk_live_against_reference_build, stored so
that the test checks the oracle against the reference's answers where oracle/_ref has not been built.

Needs oracle/_ref (make -C oracle ref REF=<reference checkout>):  python tests/golden/make_gjk_live_golden.py
Inputs are generated exactly as the test generates them (default_rng(5), float32-valued); outputs: distance, witness v, simplex size.
"""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from oracle import oracle as O  # noqa: E402


def hulls():
    rng = np.random.default_rng(5)
    return np.asarray([(rng.normal(size=(6, 3)) * (0.2 + (t % 5))).astype(np.float32) for t in range(3000)])


def main():
    ref = O.ref_gjk_lib()
    if ref is None:
        raise SystemExit("oracle/_ref/libref_opengjk.so missing: run `make -C oracle ref` with the reference checkout")
    pts = hulls()
    zero = np.zeros(3)
    dp = ctypes.POINTER(ctypes.c_double)
    v = np.zeros((len(pts), 3)); d = np.zeros(len(pts)); nv = np.zeros(len(pts), np.int32)
    # the reference prints a debug line on some degenerate inputs; silence fd 1 while it runs
    sys.stdout.flush()
    saved = os.dup(1); devnull = os.open(os.devnull, os.O_WRONLY); os.dup2(devnull, 1)
    try:
        for i, p in enumerate(pts.astype(np.float64)):
            n = ctypes.c_int()
            d[i] = ref.ref_gjk(p.ctypes.data_as(dp), 6, zero.ctypes.data_as(dp), 1, v[i].ctypes.data_as(dp), ctypes.byref(n))
            nv[i] = n.value
    finally:
        os.dup2(saved, 1); os.close(devnull); os.close(saved)
    np.savez_compressed(os.path.join(os.path.dirname(__file__), "gjk_live_vectors.npz"), pts=pts, v=v, dist=d, nvrtx=nv)
    print("wrote", len(pts), "vectors; simplex sizes:", np.bincount(nv))


if __name__ == "__main__":
    main()
