#!/usr/bin/env python3
"""Measurement: what the white noise of the resident closed loop (mpc_loop_set_noise) costs.  LMPC-CSTR, N = 50, 4096 instances from the
benchmark's start states, 20 and 100 steps from t = 0, noise-free and with R_wn = 1e-4 I, G_wn = I, Q_wn = 1e-4 I (noise_seed = 7): steps per second from the device
events of mpc_last_kernel_ms (best of five runs) and the mean of ITERS_DYN.  The noisy loop takes more interior-point iterations - the warm-start test
delta <= kWsDelta fails more often -, which is the algorithm's answer to a noisier estimate, not the price of reading 8 (ny + nxp) bytes per instance-step.
   tools/noise_cost.py [out.json]     (GPU box)"""
import json, os, sys, warnings
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mpc_code_amd as m
from mpc_code_amd import capi
from mpc_code_amd.driver import run_closed_loop


def run(p, B, nsteps, seed, runs=5):
    x0 = np.random.default_rng(20250614).uniform([-0.5, -8.0, -5.0], [0.5, 8.0, 5.0], size=(B, 3))
    s = capi.Solver(p)
    try:
        best, r = None, None
        for _ in range(runs + 1):      # (the first run pays for the first launch)
            r = run_closed_loop(p, x0, x0, nsteps, solver=s, noise_seed=seed)
            ms, launches = s.last_kernel_ms()
            best = ms if best is None else min(best, ms)
        kernel = int(s.get_option("loop_kernel"))
    finally:
        s.close()
    return dict(noise=seed is not None, batch=B, steps=nsteps, loop_kernel=kernel, launches=launches, kernel_ms=best, msteps_per_s=B * nsteps / best / 1e3,
                iters_dyn_mean=float(r["ITERS_DYN"].mean()), status_dyn=np.bincount(r["STATUS_DYN"].ravel(), minlength=3).tolist())


if __name__ == "__main__":
    I = (1e-4 * np.eye(3)).tolist()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = m.load_problem(m.example_path("cstr_lmpc.py"), overrides={"R_wn": I, "G_wn": np.eye(3).tolist(), "Q_wn": I})
    out = []
    for nsteps in (20, 100):
        for seed in (None, 7):
            out.append(run(p, 4096, nsteps, seed))
            print(json.dumps(out[-1]), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
