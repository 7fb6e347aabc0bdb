#!/usr/bin/env python3
"""Parent against change from alternated bench.py runs:  tools/ab_compare.py DIR OUT.json CONFIG [CONFIG ...]

DIR holds the JSON result lines of the runs, <config>_<side>_<round>.json with side = parent | change (each run itself the median of its --repeats timed
regions).  Per config and side: the runs' ms_per_step, their median, and the same-build difference of medians (largest minus smallest run of that side).
Rule: the change passes a config if its median lies within three times the larger of the two same-build differences of the parent's median, or below it."""
import glob
import json
import os
import statistics
import sys

d, out, configs = sys.argv[1], sys.argv[2], sys.argv[3:]
res = {"what": "bench.py per config, parent and change alternated on one MI355X in one session; ms_per_step of each run (the median of its timed regions)",
       "rule": "change median <= parent median + 3 x max(same-build difference of medians of the parent's runs, of the change's runs)", "configs": {}}
ok = True
for c in configs:
    cell = {}
    for side in ("parent", "change"):
        runs = []
        for f in sorted(glob.glob(os.path.join(d, f"{c}_{side}_*.json"))):
            line = [l for l in open(f) if l.startswith("{")][-1]
            runs.append(json.loads(line)["ms_per_step"])
        cell[side + "_ms_per_step"] = runs
        cell[side + "_median"] = statistics.median(runs)
        cell[side + "_spread"] = max(runs) - min(runs)
    allowed = 3.0 * max(cell["parent_spread"], cell["change_spread"])
    cell["allowed_difference"] = allowed
    cell["difference"] = cell["change_median"] - cell["parent_median"]
    cell["relative_difference"] = cell["difference"] / cell["parent_median"]
    cell["verdict"] = "within" if cell["difference"] <= allowed else "outside"
    ok &= cell["verdict"] == "within"
    res["configs"][c] = cell
    print(f"{c}: parent {cell['parent_median']:.5f} ms/step (spread {cell['parent_spread']:.5f}), change {cell['change_median']:.5f} (spread {cell['change_spread']:.5f}), "
          f"difference {cell['difference']:+.5f} ({100 * cell['relative_difference']:+.2f} %), allowed {allowed:.5f}: {cell['verdict']}")
json.dump(res, open(out, "w"), indent=1)
sys.exit(0 if ok else 1)
