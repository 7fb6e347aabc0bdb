#!/usr/bin/env python3
"""Per dimension set the largest figures of tests/test_wv_directions.py, from the output of `pytest -m gpu -s tests/test_wv_directions.py`
(its `wvdir` lines): fit residual of the wave and of the lane solver, step-length deviation, errors of the reported bound residual and
complementarity.  `python tools/wv_direction_report.py LOG [LOG ...]` prints the table of profiles/wv_direction_parity.txt;
`--by-horizon` the fit residuals per set and horizon (the tables of the edited kernels there: which horizons an edit shows at)."""
import re
import sys
from collections import defaultdict

LINE = re.compile(r"^wvdir (\S+?)-(finite|mixed)-N(\d+)-B(\d+) (wave|lane) j=(\d) resid=(\S+) dalpha=(\S+) dres_p=(\S+) dmu=(\S+) acond=(\S+)")


def report(paths, by_horizon=False):
    worst = defaultdict(lambda: defaultdict(float))
    for path in paths:
        with open(path) as fh:
            for line in fh:
                m = LINE.match(line.lstrip(".FEsx"))
                if not m:
                    continue
                dims, _, N, _, solver, _, resid, dalpha, dres_p, dmu, acond = m.groups()
                key = (dims, int(N)) if by_horizon else (dims,)
                for k, v in (("resid", resid), ("dalpha", dalpha), ("dres_p", dres_p), ("dmu", dmu), ("acond", acond)):
                    for kk in (key, ("all",) * len(key)):
                        x = float(v)
                        worst[kk][solver + "_" + k] = max(worst[kk][solver + "_" + k], x if x == x else float("inf"))      # nan: an iterate of nans
    cols = [s + "_" + k for k in (("resid",) if by_horizon else ("resid", "dalpha", "dres_p", "dmu", "acond")) for s in ("wave", "lane")]
    print(f"{'set':<22}" + "".join(f"{c:>13}" for c in cols))
    for key in sorted(worst, key=lambda k: (k[0] == "all", k)):
        print(f"{' N='.join(str(v) for v in key):<22}" + "".join(f"{worst[key][c]:>13.2e}" for c in cols))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--by-horizon"]
    report(args, by_horizon="--by-horizon" in sys.argv)
