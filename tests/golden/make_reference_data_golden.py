"""Copies the reference's DATA files that the CPU suite reads into tests/golden, so that no test needs the reference checkout:

  * every octomap binary tree it ships (world/*.bt, world/forest/*.bt) -> reference_maps.npz, one uint8 array per file, keyed by
    its path under world/ (tests/test_map_assumptions.py writes them back out to a temporary directory);
  * its QP fixture log/QPmodel.lp -> QPmodel.lp, verbatim (tests/test_oracle_pins.py hands it to HiGHS's own LP-file reader).

Data only, byte for byte.   python tests/golden/make_reference_data_golden.py <reference checkout>
"""
import glob
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    world = os.path.join(ref, "world")
    maps = sorted(glob.glob(os.path.join(world, "*.bt")) + glob.glob(os.path.join(world, "forest", "*.bt")))
    if not maps:
        raise SystemExit(f"no world/*.bt under {ref}")
    arrays = {os.path.relpath(p, world): np.frombuffer(open(p, "rb").read(), np.uint8) for p in maps}
    np.savez_compressed(os.path.join(HERE, "reference_maps.npz"), **arrays)
    shutil.copyfile(os.path.join(ref, "log", "QPmodel.lp"), os.path.join(HERE, "QPmodel.lp"))
    print(len(arrays), "maps,", sum(a.size for a in arrays.values()), "bytes; QPmodel.lp")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
