#!/usr/bin/env python3
"""Measurement: the cost of a user inequality row on the non-linear tracking path (User_g_ineq): closed-loop steps/s of the
wave-autonomous kernel (3) and the split pipeline (4) for examples/cstr_nmpc.py against examples/cstr_nmpc_rows.py (stage state 3 -> 4), at 4096 and 16384
instances, 20 timed steps from t = 0 after a warm-up run.  The two models alternate within one process, the median over the repeats is reported.
   tools/nmpc_rows_cost.py [out.json] [repeats]                    (GPU box)
Kernel times come from a separate run under the profiler, one timed pass per case:
   rocprofv3 --kernel-trace --stats -d DIR -- python tools/nmpc_rows_cost.py --trace"""
import json, os, sys, time
import warnings
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mpc_code_amd as m
from mpc_code_amd import nmpc

CASES = [("plain", "cstr_nmpc.py"), ("rows", "cstr_nmpc_rows.py")]
BATCHES, KERNELS, NSTEPS = (4096, 16384), (3, 4), 20


def one(s, p, x0, kernel):
    s.set_kernel(kernel)
    s.alloc(x0.shape[0], NSTEPS); s.set_state(x0, x0); s.set_schedule(p.schedules(NSTEPS))
    s.sync()
    t0 = time.perf_counter()
    s.run(0, NSTEPS, 1, 1e-9); s.sync()
    wall = time.perf_counter() - t0
    st = s.get_log("STATUS_DYN")
    return dict(kernel_ms=float(s.last_kernel_ms()), wall_ms=wall * 1e3, status=np.bincount(st.ravel(), minlength=3).tolist())


def main():
    trace = "--trace" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--trace"]
    out_path = args[0] if args else None
    repeats = 1 if trace else (int(args[1]) if len(args) > 1 else 5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        probs = {c: m.load_problem(m.example_path(ex)) for c, ex in CASES}
    solvers = {c: nmpc.NmpcSolver(probs[c]) for c, _ in CASES}
    rng = np.random.default_rng(7)
    res = []
    try:
        for B in BATCHES:
            x0 = np.tile(probs["plain"].x0_p, (B, 1)); x0[1:] *= 1.0 + 0.02 * rng.uniform(-1, 1, size=(B - 1, 3))
            for kern in KERNELS:
                for c, _ in CASES:      # warm-up (library load, first launch)
                    one(solvers[c], probs[c], x0, kern)
                runs = {c: [] for c, _ in CASES}
                for _ in range(repeats):      # the two models alternate
                    for c, _ in CASES:
                        runs[c].append(one(solvers[c], probs[c], x0, kern))
                for c, _ in CASES:
                    ms = float(np.median([r["kernel_ms"] for r in runs[c]]))
                    row = dict(case=c, batch=B, kernel=kern, steps=NSTEPS, repeats=repeats, median_ms=ms, msteps_per_s=B * NSTEPS / ms / 1e3,
                               all_ms=[r["kernel_ms"] for r in runs[c]], status=runs[c][-1]["status"])
                    res.append(row)
                    print(json.dumps(row), flush=True)
                a, b = res[-2], res[-1]
                print(json.dumps(dict(batch=B, kernel=kern, rows_over_plain=b["median_ms"] / a["median_ms"])), flush=True)
    finally:
        for s in solvers.values():
            s.close()
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
