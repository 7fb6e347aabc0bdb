#!/usr/bin/env python3
"""Measurement: the cost of the target's user rows (User_g_ineq_SS / User_h_eq_SS) on the wave-autonomous closed loop (loop_kernel = 3):
LMPC-CSTR against examples/cstr_lmpc_ss_rows.py, 4096 instances x 20 steps from t = 0 (one launch, best of five), each with the estimator and target on 16 lanes per
instance (target_row16, the product) and on one lane per instance (target_lane, a diagnostic build with -DMPC_ROW16_OFF).
   tools/target_rows_cost.py build          (here: compiles csrc/jit/rowcost_*.so)
   tools/target_rows_cost.py [out.json]     (GPU box)"""
import json, os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mpc_code_amd as m
from mpc_code_amd import capi
CSRC = capi.CSRC
CASES = [("cstr", "cstr_lmpc.py", (3, 2, 3, 3, 3, 0, 0)), ("ss_rows", "cstr_lmpc_ss_rows.py", (3, 2, 3, 3, 3, 0, 0, 1, 1))]
FORMS = [("row16", []), ("lane", ["-DMPC_ROW16_OFF"])]
lib = lambda case, form: os.path.join(CSRC, "jit", f"rowcost_{case}_{form}.so")


def build():
    from concurrent.futures import ThreadPoolExecutor
    jobs = [["/opt/rocm/bin/hipcc", *capi.HIPCC_FLAGS, *fl, "-DMPC_DIM_LIST(X)=X(" + ",".join(map(str, dims)) + ")", "-o", lib(case, form), os.path.join(CSRC, "mpc_amd.hip")]
            for case, _ex, dims in CASES for form, fl in FORMS]
    os.makedirs(os.path.join(CSRC, "jit"), exist_ok=True)
    with ThreadPoolExecutor(4) as ex:
        list(ex.map(lambda c: subprocess.check_call(c, cwd=CSRC), jobs))
    print("built", [os.path.basename(j[j.index("-o") + 1]) for j in jobs])


def run(case, ex, form, B=4096, nsteps=20):
    from mpc_code_amd.driver import run_closed_loop
    p = m.load_problem(m.example_path(ex))
    x0 = np.random.default_rng(20250614).uniform([-0.5, -8.0, -5.0], [0.5, 8.0, 5.0], size=(B, 3))
    s = capi.Solver(p, lib_path=lib(case, form))
    try:
        s.set_option("loop_kernel", 3)
        s.set_option("steps_per_launch", nsteps)
        best, r = None, None
        for _ in range(6):
            r = run_closed_loop(p, x0, x0, nsteps, solver=s)
            ms, _n = s.last_kernel_ms()
            best = ms if best is None else min(best, ms)
    finally:
        s.close()
    return dict(case=case, form=form, batch=B, steps=nsteps, kernel_ms=best, msteps_per_s=B * nsteps / best / 1e3,
                status_ss=np.bincount(r["STATUS_SS"].ravel(), minlength=3).tolist()), r


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
        sys.exit(0)
    out, logs = [], {}
    for case, ex, _dims in CASES:
        for form, _fl in FORMS:
            row, r = run(case, ex, form)
            logs[(case, form)] = r
            out.append(row)
            print(json.dumps(row), flush=True)
    for case, _ex, _dims in CASES:      # the two forms compute the same loop (sums over rows in another order: rounding apart)
        a, b = logs[(case, "row16")], logs[(case, "lane")]
        print(json.dumps(dict(case=case, same_status=bool(np.array_equal(a["STATUS_SS"], b["STATUS_SS"])), max_du=float(np.abs(a["U"] - b["U"]).max()))), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
