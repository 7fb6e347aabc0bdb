#!/usr/bin/env python3
"""Outputs of the three closed-loop kernels of the non-linear tracking library, one directory of .npy per case and kernel: tools/nmpc_step_dump.py OUT_DIR

For tools/dump_compare.py: run this script on two checkouts (it uses nothing but mpc_code_amd.load_problem, tests/nmpc_family.load_product and
mpc_code_amd.nmpc) and compare OUT_DIR/<case> pairwise; a refactoring of csrc/mpc_nmpc.hip has to leave every array as it was, to the bit.

Closed loops: 70 instances (a ragged last block for the 64 lanes of the lane kernels and for the four instances of a wave), 6 steps in two launches of 3
(the state goes through HBM once, with the warm-start flags) and a third launch of one step, whose logs show the state the second launch left; every float log and
the five status / iteration logs, per kernel (1 instance per lane, 3 wave-autonomous, 4 split pipeline) that takes the model.  One case per branch of the step's
scalar phases: extended Kalman filter with one real-time iteration and iterated to the KKT point, white noise on the measurements, N = 33 (the unpaired wave
variants), user rows, the fixed gain with saturated disturbance estimate and pxp / pyp schedules (family member c22), the input-move form (no wave kernels), starts
so far apart that steps are held and previous targets kept.  Per call: two steps through nmpc_ekf_update, nmpc_target_solve, nmpc_ocp_solve, nmpc_plant_step.

The script asserts that the hold rule ran (an instance-step with STATUS_DYN = 2) and that a previous target was kept (STATUS_SS = 2) in at least one case each,
and prints which."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mpc_code_amd as m  # noqa: E402
from mpc_code_amd import nmpc  # noqa: E402
import nmpc_family  # noqa: E402

B, LAUNCHES = 70, ((0, 3), (3, 3), (6, 1))
NSTEPS = sum(n for _, n in LAUNCHES)
ALL, LANE_ONLY, WAVE_ONLY = (1, 3, 4), (1,), (3, 4)


def spread_starts(p, seed, sp, sm=None):
    """plant and model starts about the example's x0_p: apart from each other by the same spread, or the model about the plant's by sm"""
    rng = np.random.default_rng(seed)
    assert p.nx == p.nxp
    x0 = p.x0_p * (1.0 + sp * rng.uniform(-1, 1, size=(B, p.nx)))
    xm = p.x0_p * (1.0 + sp * rng.uniform(-1, 1, size=(B, p.nx))) if sm is None else x0 * (1.0 + sm * rng.uniform(-1, 1, size=(B, p.nx)))
    return x0, xm


def loop_cases():
    """name -> (problem, x0_p, x0_m, max_sqp, kernels, noise seed or None)"""
    cases = {}
    cstr = m.load_problem(m.example_path("cstr_nmpc.py"))
    x0, xm = spread_starts(cstr, 1, 0.02)
    cases["ekf_rti"] = (cstr, x0, xm, 1, ALL, None)
    cases["ekf_sqp20"] = (cstr, x0, xm, 20, ALL, None)
    cases["noise"] = (cstr, x0, xm, 1, ALL, 31)
    cases["noise_sqp20"] = (cstr, x0, xm, 20, ALL, 31)
    n33 = m.load_problem(m.example_path("cstr_nmpc.py"), overrides={"N": 33})
    cases["N33"] = (n33, x0, xm, 1, WAVE_ONLY, None)
    rows = m.load_problem(m.example_path("cstr_nmpc_rows.py"))
    cases["rows"] = (rows,) + spread_starts(rows, 9, 0.02) + (1, ALL, None)
    c22 = nmpc_family.load_product("c22")
    cases["c22_fixed_gain_dsat"] = (c22,) + spread_starts(c22, 22, *nmpc_family.SPREAD["c22"]) + (1, ALL, None)
    duv = m.load_problem(m.example_path("quadtank_nmpc_dis.py"))
    cases["duv_quadtank"] = (duv,) + spread_starts(duv, 4, 0.02) + (1, LANE_ONLY, None)
    # tests/test_nmpc.py:test_gpu_kernels_agree_under_mismatch_holds_and_divergence, seed 6: its spread for the first half of the batch, twice as wide beyond
    hx, hm = spread_starts(cstr, 6, 0.05)
    wx, wm = spread_starts(cstr, 6, 0.10)
    hx[B // 2:], hm[B // 2:] = wx[B // 2:], wm[B // 2:]
    cases["hold_cstr"] = (cstr, hx, hm, 1, ALL, None)
    # the held starts of the family (tests/nmpc_family.py:starts): from 6.0 the target is infeasible too and the previous one is kept, from 4.0 the OCP alone is held
    d22 = nmpc_family.load_product("d22")
    h3, _ = nmpc_family.starts("d22_hold", d22.x0_p)
    hd = np.tile(h3, (B // 3 + 1, 1))[:B] * (1.0 + 0.01 * np.random.default_rng(8).uniform(-1, 1, size=(B, 2)))
    cases["hold_d22"] = (d22, hd, hd.copy(), 1, ALL, None)
    return cases


def save(out_dir, case, arrays):
    d = os.path.join(out_dir, case)
    os.makedirs(d, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(d, k + ".npy"), np.asarray(v))


def run_loops(out_dir):
    hold, kept = [], []
    solvers = {}
    try:
        for name, (p, x0, xm, max_sqp, kernels, noise_seed) in loop_cases().items():
            s = solvers.get(id(p))
            if s is None:
                s = solvers[id(p)] = nmpc.NmpcSolver(p, device=0)
            for kern in kernels:
                s.set_kernel(kern)
                s.alloc(B, NSTEPS)
                s.set_state(x0, xm)
                s.set_schedule(p.schedules(NSTEPS))
                s.set_noise(nmpc.measurement_noise(p, NSTEPS, B, noise_seed) if noise_seed is not None else None)
                for k0, n in LAUNCHES:
                    s.run(k0, n, max_sqp, 1e-9)
                s.sync()
                r = {k: s.get_log(k) for k in list(s.LOGS) + list(s.ILOGS) if not (k == "D_HAT" and p.nd == 0)}
                s.set_noise(None)
                case = f"loop_{name}_k{kern}"
                save(out_dir, case, r)
                n_hold, n_kept = int((r["STATUS_DYN"] == 2).sum()), int((r["STATUS_SS"] == 2).sum())
                print(f"{case:30s} STATUS_DYN: {np.bincount(r['STATUS_DYN'].ravel(), minlength=3).tolist()}  STATUS_SS: {np.bincount(r['STATUS_SS'].ravel(), minlength=3).tolist()}"
                      f"  SQP_DYN max {int(r['SQP_DYN'].max())}" + (f"  D_HAT at a bound: {int(np.isin(r['D_HAT'], np.concatenate([p.dmin, p.dmax])).sum())}" if name.startswith("c22") else ""), flush=True)
                if n_hold:
                    hold.append(case)
                if n_kept:
                    kept.append(case)
    finally:
        for s in solvers.values():
            s.close()
    assert hold, "no case with STATUS_DYN == 2: the hold rule did not run"
    assert kept, "no case with STATUS_SS == 2: no previous target was kept"
    print("hold rule ran in:", ", ".join(hold))
    print("previous target kept in:", ", ".join(kept), flush=True)


def run_calls(out_dir):
    cstr = m.load_problem(m.example_path("cstr_nmpc.py"))
    x0, xm = spread_starts(cstr, 3, 0.02)
    for name, seed in (("seam", None), ("seam_noise", 31)):
        r = nmpc.run_nmpc_stepwise(cstr, x0, xm, nsteps=2, max_sqp=1, noise_seed=seed)
        print(f"call_{name:25s} STATUS_DYN: {np.bincount(r['STATUS_DYN'].ravel(), minlength=3).tolist()}", flush=True)
        save(out_dir, "call_" + name, r)


if __name__ == "__main__":
    out = sys.argv[1]
    run_loops(out)
    run_calls(out)
    print("dumped", len(os.listdir(out)), "cases to", out)
