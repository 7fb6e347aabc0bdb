#!/usr/bin/env python3
"""Generate tests/golden/reference_examples.npz from a checkout of the reference (CPCLAB-UNIPI/MPC-code); a few seconds.

    python tests/golden/make_reference_golden.py <reference checkout>

The tests that hold the shipped examples under mpc-code_amd/examples/ against the reference's own Ex-files read these
vectors instead of the reference tree, so the suite runs without it.  What is stored is what those tests read of the
reference's side: the problem data the product's loader (and the oracle's own loaders) make of each unmodified Ex-file,
its set points, plant and model functions at sample points, and the oracle's closed loops on it.  Nothing of the
repository's own examples goes into the file: the tests compute that side when they run.

  ex_<file>_*     Ex_LMPC_CSTR / Ex_LMPC_WB / Ex_LMPC_nlplant / Ex_LMPCxp_nlplant: FIELDS, defSP, flags, plant steps (tests/test_exfile.py)
  kinds_*         the problem class of every Ex_*.py and the overrides of Ex_ENMPC.py the loader refuses
  enmpc_*         Ex_ENMPC.py: the NumPy oracle's 3-step loop, the product's loader at N = 40, N_mhe = 20 (tests/test_enmpc.py)
  ekf_*           Ex_ENMPC.py with its estimator switch (mhe_mod) off: both loaders and the oracle's loop
  nmpc_*          Ex_NMPC.py at N = 30: problem data, model and plant functions at sample points (tests/test_nmpc.py)
  dis_*           Ex_NMPC_dis.py at N = 20: likewise, with set points and the plant parameter schedule
  rx_fx           Ex_ENMPC.py's User_fxm_Cont traced and evaluated at one point
"""
import glob
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mpc_code_amd as pkg        # noqa: E402
import enmpc_oracle as eo         # noqa: E402
import nmpc_oracle as no          # noqa: E402
from reference_golden import DIS_FIELDS, DIS_TIMES, EX_FIELDS, EX_SP_TIMES, KIND_REFUSALS, LMPC_EX, NMPC_FIELDS, RX_POINT      # noqa: E402


def nlplant_points(p):
    """Five plant states and inputs around the operating point of a non-linear plant."""
    rng = np.random.default_rng(0)
    return p.x0_p + rng.normal(size=(5, p.nxp)) * [0.01, 2.0, 0.01], p.u0 + rng.normal(size=(5, p.nu)) * [2.0, 0.01]


def nmpc_points(p):
    """Four (x, u, d) around the continuous CSTR's start."""
    rng = np.random.default_rng(2)
    x = p.x0_m + rng.normal(size=(4, p.nx)) * [0.02, 3.0, 0.02]
    u = p.u0 + rng.normal(size=(4, p.nu)) * [2.0, 0.02]
    d = p.dhat0 + rng.normal(size=(4, p.nd)) * [0.01, 0.01]
    return x, u, d


def dis_points(p):
    """Five (x, u) of the four-tank example: three around its start, two with a level at or beyond a clamp of the model."""
    rng = np.random.default_rng(1)
    x = [p.x0_m + rng.normal(size=6) * [3, 3, 2, 2, 0.5, 0.5] for _ in range(3)] + [np.array([50, 50, 25.0, -1.0, 0.2, 19.99]), np.array([50, 50, 19.9, 0.01, 22, 0.0])]
    u = [p.u0 + rng.normal(size=2) * 5 for _ in x]
    return np.array(x), np.array(u)


def oracle_problem(path, overrides):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return no.load_problem(path, overrides)


def fields(out, pre, obj, names):
    """Each named attribute under <pre><name>; the names of those that are None under <pre>none."""
    none = []
    for f in names:
        v = getattr(obj, f)
        if v is None:
            none.append(f)
        else:
            out[pre + f] = np.asarray(v)
    out[pre + "none"] = np.array(none, dtype=str)


def main(ref):
    out = {}
    for theirs in LMPC_EX:
        b = pkg.load_problem(os.path.join(ref, theirs))
        pre = "ex_" + theirs[:-3] + "_"
        fields(out, pre, b, EX_FIELDS)
        for t in EX_SP_TIMES:
            for i, v in enumerate(b.defSP(t)):
                out[f"{pre}sp{t}_{i}"] = np.ravel(v)
        out[pre + "estimator"] = np.array(b.estimator)
        out[pre + "flags"] = np.array([b.DUForm, b.N, b.plant_is_linear])
        if not b.plant_is_linear:
            x, u = nlplant_points(b)
            out[pre + "plant_x"], out[pre + "plant_u"] = x, u
            out[pre + "plant"] = b.plant_step(x, u, 0.4, np.zeros(b.nxp))

    kinds = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for f in sorted(glob.glob(os.path.join(ref, "Ex_*.py"))):
            kinds[os.path.basename(f)] = type(pkg.load_problem(f)).__name__
        refused = []
        for over in KIND_REFUSALS:
            try:
                pkg.load_problem(os.path.join(ref, "Ex_ENMPC.py"), overrides=over)
                refused.append(False)
            except pkg.UnsupportedProblem:
                refused.append(True)
    out["kinds_files"] = np.array(list(kinds), dtype=str)
    out["kinds_types"] = np.array(list(kinds.values()), dtype=str)
    out["kinds_refused"] = np.array(refused)

    ex = os.path.join(ref, "Ex_ENMPC.py")
    r = eo.closed_loop(eo.load_problem(ex), 3)
    for k in ("U", "XS", "US", "X_ES", "P_K"):
        out["enmpc_loop_" + k] = r[k]
    q = pkg.load_problem(ex, overrides={"N": 40, "N_mhe": 20})
    out["enmpc_N40"] = np.array([q.N, q.N_mhe, q.nx, q.nu, q.n_w, q.max_iter])

    src = open(ex).read()
    assert src.count("mhe_mod = 'on'") == 1
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "Ex_ENMPC_ekf.py")
        open(f, "w").write(src.replace("mhe_mod = 'on'", "mhe_mod = 'off'"))
        e = eo.load_problem(f)
        out["ekf_flags"] = np.array([e.ekf, e.mhe])
        fields(out, "ekf_", e, ("Q_kf", "R_kf", "P0"))
        r = eo.closed_loop(e, 3)
        for k in ("U", "XS", "US", "X_ES", "P_K"):
            out["ekf_loop_" + k] = r[k]
        q = pkg.load_problem(f, overrides={"N": 40})
        out["ekf_pkg_estimator"] = np.array(q.estimator)
        out["ekf_pkg_dims"] = np.array([q.N, q.nx, q.nu])
        out["ekf_pkg_Q_kf"], out["ekf_pkg_R_kf"] = q.Q_kf, q.R_kf

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ex = os.path.join(ref, "Ex_NMPC.py")
        p = pkg.load_problem(ex, overrides={"N": 30})
        fields(out, "nmpc_", p, NMPC_FIELDS)
        out["nmpc_dims"] = np.array([p.nx, p.nu, p.ny, p.nd, p.nxp, p.h, p.Mx, p.Nsim], dtype=float)
        out["nmpc_ycols"] = np.asarray(p.ycols)
        op = oracle_problem(ex, {"N": 30})
        x, u, d = nmpc_points(p)
        out["nmpc_x"], out["nmpc_u"], out["nmpc_d"] = x, u, d
        out["nmpc_model_fx"] = np.array([no.model_fx(op, x[i], u[i], d[i]) for i in range(len(x))])
        out["nmpc_plant_fx"] = np.array([[no.plant_fx(op, x[i], u[i], t) for t in (0.0, 7.0, 30.0)] for i in range(len(x))])

        ex = os.path.join(ref, "Ex_NMPC_dis.py")
        p = pkg.load_problem(ex, overrides={"N": 20})
        fields(out, "dis_", p, DIS_FIELDS)
        out["dis_estimator"] = np.array(p.estimator)
        out["dis_flags"] = np.array([p.DUForm, p.DUssForm, p.Nsim, p.discrete])
        out["dis_ycols"] = np.asarray(p.ycols)
        op = oracle_problem(ex, {"N": 20})
        x, u = dis_points(p)
        out["dis_x"], out["dis_u"] = x, u
        out["dis_model_fx"] = np.array([no.model_fx(op, x[i], u[i], np.zeros(2)) for i in range(len(x))])
        out["dis_plant_fx"] = np.array([no.plant_fx(op, x[i], u[i], 100.0) for i in range(len(x))])
        for t in DIS_TIMES:
            for i, v in enumerate(p.defSP(t)):
                out[f"dis_sp{t}_{i}"] = np.asarray(v)
            out[f"dis_pxp{t}"] = np.asarray(p.def_pxp(t)[0])

    from mpc_code_amd import symtrace as st
    ns = pkg.load_exfile(os.path.join(ref, "Ex_ENMPC.py"))
    fx = ns["User_fxm_Cont"](st.symvec("x", 2), st.symvec("u", 1), st.symvec("d", 2), st.Sym.var("t"), None)
    out["rx_fx"] = np.array([float(v) for v in st.evaluate(list(fx), RX_POINT)])

    path = os.path.join(HERE, "reference_examples.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "Ex_ENMPC.py")):
        sys.exit(__doc__)
    main(sys.argv[1])
