#!/usr/bin/env python3
"""Outputs of the instance-per-lane kernels of the linear library, one directory of .npy per case: tools/lane_step_dump.py OUT_DIR

For tools/dump_compare.py: run this script on two checkouts (it uses nothing but mpc_code_amd.load_problem, capi.Solver and
driver.run_closed_loop) and compare OUT_DIR/<case> pairwise; a refactoring of csrc/ has to leave every array as it was, to the bit.

Closed loops - loop_kernel, loop_kernel_soft, loop_kernel_pxy (option loop_kernel = 1 where the problem has a choice): 70 instances (one
full wave and six lanes), 6 steps at steps_per_launch = 4 (the state goes through HBM once, with the warm-start flags), N = 20; every
float log and the four status / iteration logs.  One case per branch of the step: Kalman filter and warm start, Delta-u cost, bounds on
Delta-u, fixed-gain estimator, saturated disturbance estimate, terminal equality (further passes), user rows of the target, a general
output row with the user plant, soft output constraints, def_px / def_py (both, def_px alone, def_py alone).
Per call - kf_kernel, ocp_kernel, ocp_kernel_pxy, ocp_kernel_soft on 70 instances: mpc_kf_update with both estimators, mpc_ocp_solve
(option ocp_kernel = 1) in the three bound modes, with px / py, and of the soft problem with its slacks.

The script asserts that the hold rule ran (an instance-step with STATUS_DYN = 2) and that a previous target was kept (STATUS_SS = 2) in
at least one case each, and prints which."""
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mpc_code_amd as m  # noqa: E402
from mpc_code_amd import capi  # noqa: E402
from mpc_code_amd.driver import run_closed_loop  # noqa: E402

B, NSTEPS, SPL, N = 70, 6, 4, 20
LOGS = ("U", "X_HAT", "XS", "US", "YS", "Xp", "D_HAT", "Sl", "STATUS_DYN", "STATUS_SS", "ITERS_DYN", "ITERS_SS")


def load(ex, **over):
    over.setdefault("N", N)
    return m.load_problem(m.example_path(ex), overrides=over)


def cstr_x0(seed, spread=(0.5, 8.0, 5.0)):
    """the benchmark's starts: part of them outside the output bounds (hold rule over the first steps)"""
    return np.random.default_rng(seed).uniform(-np.array(spread), spread, size=(B, 3))


def def_px(t):
    return [np.array([0.02 * np.sin(0.3 * t), 0.15 * np.cos(0.2 * t), 0.05 * np.sin(0.1 * t + 1.0)])]


def def_py(t):
    return [np.array([0.03 * np.cos(0.25 * t), 0.4 * np.sin(0.15 * t), 0.0])]


def loop_cases():
    """name -> (problem, x0_p, x0_m)"""
    rng = np.random.default_rng(20251020)
    cases = {}
    cstr = load("cstr_lmpc.py")
    cases["cstr"] = (cstr, cstr_x0(1), cstr_x0(1))
    wb = load("wood_berry_lmpc.py")
    xw = 0.3 * rng.standard_normal((B, wb.nxp))
    cases["wood_berry"] = (wb, xw, xw)
    du = copy.copy(cstr); du.Dumin = np.array([-0.5, -1.0]); du.Dumax = np.array([0.5, 1.0])
    cases["du_bounds"] = (du, cstr_x0(2, (0.5, 2.4, 3.0)), cstr_x0(2, (0.5, 2.4, 3.0)))
    K = np.vstack([0.5 * np.eye(3), 0.2 * np.eye(3)])
    cases["fixed_gain"] = (load("cstr_lmpc.py", kal=False, lue=True, K=K), cstr_x0(3), cstr_x0(3) + 0.1 * rng.standard_normal((B, 3)))
    # the plant's disturbance is beyond dmax: the estimate runs into the bound within the first steps
    cases["dsat"] = (load("cstr_lmpc.py", dmin=[-0.02, -0.02, -0.02], dmax=[0.02, 0.02, 0.02]), cstr_x0(4), cstr_x0(4) + 0.2 * rng.standard_normal((B, 3)))
    cases["term_cons"] = (load("cstr_lmpc.py", TermCons=True), cstr_x0(5, (0.3, 4.0, 3.0)), cstr_x0(5, (0.3, 4.0, 3.0)))
    ss = load("cstr_lmpc_ss_rows.py")
    xss = np.array([3.0, 3.0, 3.0]) + rng.uniform(-1.0, 1.0, size=(B, 3)) * np.array([0.5, 2.0, 1.0])
    xss[0] = ss.x0_p      # (the example's own start: its third step has no feasible target)
    cases["ss_rows"] = (ss, xss, xss)
    # x_0 >= 5 d_0 - 1 next to the example's equality row: no steady state where the disturbance estimate d_0 is beyond about 0.32 - initial
    # estimates on both sides of it (tests/test_target_rows.py: the hold rule of the target)
    hold = load("cstr_lmpc_ss_rows.py", User_g_ineq_SS=lambda x, u, y, d, t, px, py: -x[0] + 5.0 * d[0] - 1.0)
    hold.dhat0 = np.column_stack([rng.uniform(0.2, 0.45, B), np.zeros(B), np.zeros(B)])
    cases["ss_rows_hold"] = (hold, xss, xss)
    xp = load("cstr_xp_nlplant_lmpc.py")
    xpp = xp.x0_p + rng.normal(size=(B, xp.nxp)) * [2e-4, 0.02, 2e-4]
    xpm = np.hstack([xpp, np.zeros((B, xp.nx - xp.nxp))])
    cases["xp_nlplant"] = (xp, xpp, xpm)
    soft = load("cstr_lmpc_soft.py")
    xso = np.vstack([soft.x0_p[None], soft.x0_p[None] + rng.uniform(-1.0, 1.0, size=(B - 1, soft.nxp))])
    cases["soft"] = (soft, xso, xso[:, :soft.nx])
    xm = cstr_x0(6, (0.3, 4.0, 3.0)); xm[:8] *= 2.5      # (eight starts outside the output bounds)
    cases["pxy_both"] = (load("cstr_lmpc.py", def_px=def_px, def_py=def_py), xm, xm)
    cases["pxy_px_only"] = (load("cstr_lmpc.py", def_px=def_px, def_py=None), xm, xm)
    cases["pxy_py_only"] = (load("cstr_lmpc.py", def_px=None, def_py=def_py), xm, xm)
    return cases


def save(out_dir, case, arrays):
    d = os.path.join(out_dir, case)
    os.makedirs(d, exist_ok=True)
    for k, v in arrays.items():
        if v is not None:
            np.save(os.path.join(d, k + ".npy"), np.asarray(v))


def run_loops(out_dir):
    hold, kept = [], []
    for name, (p, x0p, x0m) in loop_cases().items():
        s = capi.Solver(p, device=0)
        try:
            s.set_option("steps_per_launch", SPL)
            if not (getattr(p, "slacks", False) or p.has_model_params):      # (those two have one loop kernel each)
                s.set_option("loop_kernel", 1)
            r = run_closed_loop(p, x0p, x0m, NSTEPS, solver=s, fused=True)
        finally:
            s.close()
        save(out_dir, "loop_" + name, {k: r[k] for k in LOGS if k in r})
        n_hold, n_kept = int((r["STATUS_DYN"] == 2).sum()), int((r["STATUS_SS"] == 2).sum())
        print(f"loop_{name:12s} STATUS_DYN: {np.bincount(r['STATUS_DYN'].ravel(), minlength=3).tolist()}  STATUS_SS: {np.bincount(r['STATUS_SS'].ravel(), minlength=3).tolist()}"
              + (f"  D_HAT at its bound: {int((np.abs(r['D_HAT']) == 0.02).sum())}" if name == "dsat" else ""), flush=True)
        if name == "dsat":
            assert (np.abs(r["D_HAT"]) == 0.02).any(), "the disturbance estimate did not saturate"
        if n_hold:
            hold.append(name)
        if n_kept:
            kept.append(name)
    assert hold, "no case with STATUS_DYN == 2: the hold rule did not run"
    assert kept, "no case with STATUS_SS == 2: no previous target was kept"
    print("hold rule ran in:", ", ".join(hold))
    print("previous target kept in:", ", ".join(kept), flush=True)


def run_calls(out_dir):
    rng = np.random.default_rng(77)
    cstr = load("cstr_lmpc.py")
    xh = cstr_x0(7); d = 0.02 * rng.standard_normal((B, 3)); up = rng.uniform(-1.0, 1.0, (B, 2))
    xs = 0.05 * rng.standard_normal((B, 3)); us = 0.05 * rng.standard_normal((B, 2))
    y = xh + 0.05 * rng.standard_normal((B, 3))
    Pm = np.broadcast_to(1e-3 * np.eye(6), (B, 6, 6)).copy()
    fixed = load("cstr_lmpc.py", kal=False, lue=True, K=np.vstack([0.5 * np.eye(3), 0.2 * np.eye(3)]))
    for name, p, P0 in (("kf_kalman", cstr, Pm), ("kf_fixed_gain", fixed, None)):
        s = capi.Solver(p, device=0)
        try:
            xi, Pk = s.kf_update(y, np.hstack([xh, d]), P0)
            s.set_model_offsets(B, None, def_py(3.0)[0])
            xi2, Pk2 = s.kf_update(y, np.hstack([xh, d]), P0)
        finally:
            s.close()
        save(out_dir, "call_" + name, dict(xi=xi, P=Pk, xi_py0=xi2, P_py0=Pk2))
    # the three bound modes of ocp_kernel: inputs only | inputs and states, all finite | some absent
    inf = np.inf
    modes = (("ocp_inputs_only", load("cstr_lmpc.py", xmin=[-inf] * 3, xmax=[inf] * 3, ymin=[-inf] * 3, ymax=[inf] * 3)),
             ("ocp_all_bounds", cstr),
             ("ocp_masked", load("cstr_lmpc.py", xmin=[-inf, -10.0, -inf], xmax=[inf, 10.0, 6.0], ymin=[-inf, -8.0, -inf], ymax=[inf, 10.0, 6.0])))
    for name, p in modes:
        s = capi.Solver(p, device=0)
        try:
            s.set_option("ocp_kernel", 1)
            r = s.ocp_solve(xh, xs, us, d, up)
        finally:
            s.close()
        print(f"call_{name:16s} status: {np.bincount(r['status'], minlength=3).tolist()}", flush=True)
        save(out_dir, "call_" + name, {k: r[k] for k in ("u0", "x1", "status", "iters", "res")})
    pxy = load("cstr_lmpc.py", def_px=def_px, def_py=def_py)
    PX = np.stack([pxy.horizon_params(0.7 * b)[0] for b in range(B)]); PY = np.stack([pxy.horizon_params(0.7 * b)[1] for b in range(B)])
    s = capi.Solver(pxy, device=0)
    try:
        for name, kw in (("ocp_pxy", dict(px=PX, py=PY)), ("ocp_px", dict(px=PX)), ("ocp_py", dict(py=PY))):
            r = s.ocp_solve(xh * [0.6, 0.5, 0.6], xs, us, d, up, **kw)
            print(f"call_{name:16s} status: {np.bincount(r['status'], minlength=3).tolist()}", flush=True)
            save(out_dir, "call_" + name, {k: r[k] for k in ("u0", "x1", "status", "iters", "res")})
    finally:
        s.close()
    soft = load("cstr_lmpc_soft.py")
    xso = np.vstack([np.array([[3.0, 3.0, 3.0]]), rng.uniform([-1, -8, -5], [1, 12, 12], size=(B - 1, 3))])
    s = capi.Solver(soft, device=0)
    try:
        r = s.ocp_solve(xso, 4.0 * xs, 4.0 * us, 5.0 * d, np.zeros((B, 2)))
    finally:
        s.close()
    print(f"call_ocp_soft         status: {np.bincount(r['status'], minlength=3).tolist()}", flush=True)
    save(out_dir, "call_ocp_soft", {k: r[k] for k in ("u0", "x1", "status", "iters", "res", "sl")})


if __name__ == "__main__":
    out = sys.argv[1]
    run_loops(out)
    run_calls(out)
    print("dumped", len(os.listdir(out)), "cases to", out)
