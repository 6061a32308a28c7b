"""Copies the reference's two 20-agent octomap mission suites into tests/golden, so that no test needs the reference checkout:

  * missions/forest/20agents/*.json (30 missions, flown by launch/testall_forest.launch on world/forest/forest{i}.bt, one world each)
  * missions/office/20agents/*.json (30 missions, flown by launch/testall_office.launch on the one world/office.bt)

-> testall_missions_20agents.json: {"forest": {file name: file text}, "office": {...}}, every mission file verbatim (its text, byte for
byte), keyed by its name.  The worlds are already in reference_maps.npz (make_reference_data_golden.py).

Data only.   python tests/golden/make_testall_missions_golden.py <reference checkout>
"""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SUITES = ("forest", "office")


def main(ref):
    out = {}
    for suite in SUITES:
        files = sorted(glob.glob(os.path.join(ref, "missions", suite, "20agents", "*.json")))
        if not files:
            raise SystemExit(f"no missions/{suite}/20agents/*.json under {ref}")
        out[suite] = {os.path.basename(p): open(p, encoding="utf-8", newline="").read() for p in files}
    with open(os.path.join(HERE, "testall_missions_20agents.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(", ".join(f"{s}: {len(out[s])} missions" for s in SUITES))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
