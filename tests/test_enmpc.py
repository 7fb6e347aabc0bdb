"""Economic NMPC with the moving-horizon estimator (BASELINE configs[3] and [4]).

CPU tests: the oracle against its committed vectors and against independent solvers / integrators; the product's host side (loader,
generated derivative code compiled for the host) against the oracle's complex-step derivatives; the C-ABI's exports.
GPU tests (-m gpu): the HIP path through the C-ABI against the oracle's golden vectors and, at the BASELINE sizes, through
size-independent properties plus instances re-run by the oracle.
"""
import ctypes as ct
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from reference_golden import assert_fields

import enmpc_oracle as eo

EX = os.path.join(ROOT, "mpc-code_amd", "examples", "reactor_enmpc.py")
GOLD = os.path.join(ROOT, "tests", "golden", "enmpc_reactor.npz")
EX_ROWS = os.path.join(ROOT, "mpc-code_amd", "examples", "reactor_enmpc_rows.py")      # the example with user inequality rows in the OCP
EX_EKF = os.path.join(ROOT, "mpc-code_amd", "examples", "reactor_enmpc_ekf.py")      # the example with the other position of its estimator switch
GOLD_EKF = os.path.join(ROOT, "tests", "golden", "enmpc_reactor_ekf.npz")
TOL_U = 1e-7          # GPU against the oracle on u*, xs, us, [x; d]: both stop at a scaled KKT error of 1e-8 (measured: 1e-13)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def oprob():
    return eo.load_problem(EX)


@pytest.fixture(scope="module")
def prob(pkg):
    return pkg.load_problem(EX)


# ---------------------------------------------------------------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def test_golden_vectors_certify_themselves(gold):
    for pre in ("ship_", "c4_", "c5_"):
        assert int(gold[pre + "STATUS_DYN"].max()) == 0 and int(gold[pre + "STATUS_SS"].max()) == 0
        for k in ("KKT_DYN", "KKT_SS", "KKT_MHE"):      # every NLP's own first-order conditions: what IPOPT terminates on (tol 1e-8) - on the problem as IPOPT
            # scales it: the OCP's cost is multiplied by df = 100 / |grad f(w0)|_inf (0.07 - 0.2 on the cold steps), so its unscaled residual may reach 1e-8 / df
            # ... and at the point IPOPT RETURNS: the solve runs on bounds relaxed by 1e-8 max(1, |b|) and the final point is projected back into the caller's bounds
            # (honor_original_bounds), so a variable on a bound moves by that much and the equality rows it enters see it through the model's sensitivities
            assert float(gold[pre + k].max()) < 2e-7, (pre, k)
    # the economics: the loop settles at the profit-optimal steady state of the reactor (u = 1.0430, cB = 0.4671)
    assert abs(gold["ship_U"][-1, 0, 0] - 1.04297536) < 1e-7 and abs(gold["ship_XS"][-1, 0, 1] - 0.46708998) < 1e-7


def test_oracle_reproduces_its_vectors(oprob, gold):
    r = eo.closed_loop(oprob, 5)
    for k in ("U", "XS", "US", "X_ES"):
        assert np.abs(r[k] - gold["ship_" + k][:5, 0]).max() < 1e-12, k
    assert r["ITERS_DYN"].tolist() == gold["ship_ITERS_DYN"][:5, 0].tolist()


def test_c_restatement_follows_the_golden_loops(gold):
    """oracle/enmpc_oracle.c - hand-written functions, complex-step derivatives, null-space (QR + Cholesky) Newton steps - against the vectors of
    the NumPy oracle (dense LU): the same loops to rounding and the same interior-point iteration counts, at the shipped and both BASELINE sizes."""
    import enmpc_oracle_c as ec
    for pre, over, ns in (("ship_", None, 21), ("c4_", {"N": 40}, 10), ("c5_", {"N_mhe": 20}, 24), ("flt_", {"mhe_up": "filter", "N_mhe": 6}, 16)):
        r = ec.OracleEC(eo.load_problem(EX, overrides=over)).closed_loop(ns, gold[pre + "x0"])
        for k in ("U", "XS", "US", "X_ES", "Xp"):
            assert np.abs(r[k] - gold[pre + k][:ns]).max() < 1e-11, (pre, k, np.abs(r[k] - gold[pre + k][:ns]).max())
        for k in ("ITERS_DYN", "ITERS_SS", "ITERS_MHE", "STATUS_DYN", "STATUS_SS"):
            assert np.array_equal(r[k], gold[pre + k][:ns]), (pre, k)


def test_restatements_agree_where_a_slack_rounds_to_zero():
    """dmin / dmax as bounds of the estimator (MPC_code.py:657-664) and an estimate of step 0 that ends on its bound with a vanishing multiplier: the
    last Newton steps leave a slack below the spacing of the doubles at the bound.  Round 3's restatement ended such a solve "failed" with an infinite
    multiplier; with IPOPT's safe slack - the slack lifted, the bound of the solve moved along - it ends solved, on the bound, in
    NumPy (dense LU) and C (null space) with the same iterates and iteration counts."""
    import warnings
    import enmpc_oracle_c as ec
    from enmpc_cases import draw
    for seed, inst in ((15, 3), (17, 2)):
        over, x0 = draw(seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            q = eo.load_problem(EX, overrides=over)
        c = ec.OracleEC(q).closed_loop(3, x0[inst:inst + 1], nthreads=1)
        o = eo.closed_loop(q, 3, x0_p=x0[inst])
        assert c["STATUS_MHE"][:, 0].tolist() == [0, 0, 0] == o["STATUS_MHE"].tolist()
        assert c["ITERS_MHE"][:, 0].tolist() == o["ITERS_MHE"].tolist()
        for k in ("U", "XS", "X_ES"):
            assert np.abs(o[k] - c[k][:, 0]).max() < 1e-11, (seed, k)
        assert min(abs(c["X_ES"][0, 0, 2] - (-0.05)), abs(c["X_ES"][0, 0, 3] - (-0.02)), abs(c["X_ES"][0, 0, 2] - 0.03), abs(c["X_ES"][0, 0, 3] - 0.05)) < 1e-8      # on its bound (to the estimator's tolerance)


@pytest.mark.parametrize("seed", [7, 13, 19, 23])
def test_restatements_agree_on_the_models_that_need_the_line_search(seed):
    """The randomised models on which round 3's full-step iteration and IPOPT parted (tests/enmpc_cases.py): model 13 - an OCP of 153 / 173 full steps,
    42 with the line search -, models 19 and 23 - target problems that jam on a state bound and leave through the restoration phase -, model 7 - the
    longest target solve left.  NumPy (dense LU on all variables, restoration problem in (x, n, p)) and C (null-space steps) take the same iterations to the
    same points, every status word is "solved"."""
    import warnings
    import enmpc_oracle_c as ec
    from enmpc_cases import draw
    over, x0 = draw(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        q = eo.load_problem(EX, overrides=over)
    ns = 4
    c = ec.OracleEC(q).closed_loop(ns, x0[:2], nthreads=2)
    for b in range(2):
        o = eo.closed_loop(q, ns, x0_p=x0[b])
        for k in ("STATUS_DYN", "STATUS_SS", "STATUS_MHE"):
            assert o[k].tolist() == c[k][:, b].tolist() == [0] * ns, (seed, b, k)
        for k in ("ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
            assert np.abs(o[k].astype(int) - c[k][:, b].astype(int)).max() <= 1, (seed, b, k, o[k].tolist(), c[k][:, b].tolist())
        for k in ("U", "XS", "US", "X_ES"):
            assert np.abs(o[k] - c[k][:, b]).max() < 1e-8, (seed, b, k)


def test_interval_integration_is_within_the_reference_integrators_tolerance(oprob):
    """20 Runge-Kutta steps per shooting interval against a tight adaptive integration of the same augmented system: below the
    tolerances CasADi hands IDAS by default (reltol 1e-6), for state and cost quadrature over the whole input range."""
    from scipy.integrate import solve_ivp
    import exnum
    p = oprob
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(12):
        x0 = rng.uniform([0.0, 0.0], [1.0, 1.0]); u = rng.uniform(0.0, 2.0, 1); d = rng.uniform(-0.1, 0.1, 2)

        def rhs(t, z):
            xd = np.asarray(p.fxm(z[:2], u, d, 0.0, np.zeros(2)), dtype=float)
            return np.concatenate([xd, [p.fobj(z[:2], u, z[:2] + p.Cd @ d, None, None, None)]])
        ex = solve_ivp(rhs, (0.0, p.h), np.concatenate([x0, [0.0]]), rtol=1e-12, atol=1e-14, method="DOP853").y[:, -1]
        xn, q = eo.ocp_stage(p, x0.reshape(-1, 1), u.reshape(-1, 1), d.reshape(-1, 1), np.zeros((2, 1)), np.zeros((1, 1)))
        worst = max(worst, float(np.abs(np.concatenate([xn[:, 0], q]) - ex).max()))
    assert worst < 1e-6, worst


def test_ocp_minimum_is_found_by_an_independent_solver(oprob):
    """SciPy's SLSQP on the same NLP (short horizon), started at the oracle's answer perturbed: it returns to the same point, and its
    cost is not lower anywhere it goes - the oracle's KKT point is a local minimum, not a saddle."""
    from scipy.optimize import minimize
    p = eo.load_problem(EX, overrides={"N": 6})
    n, m, N = p.nx, p.nu, p.N
    nz = n + m
    ts = eo.target_solve(p, np.zeros(2))
    xhat = np.array([0.8, 0.3])
    wg = np.zeros(nz * N + n)
    for k in range(1, N + 1):
        wg[k * nz - m:k * nz] = p.u0; wg[k * nz:k * nz + n] = p.x0_m
    sol = eo.ocp_solve(p, xhat, ts["xs"], ts["us"], np.zeros(2), wg)
    # (the tolerance applies to the problem as IPOPT scales it: the unscaled residual may reach 1e-8 / df, df = 0.036 here)
    assert sol["status"] == 0 and max(eo.kkt_nlp(sol["evalf"], sol, sol["lo"], sol["hi"]).values()) < 1.05e-8 / sol["df"]
    evalf, lo, hi = sol["evalf"], sol["lo"], sol["hi"]
    free = lo != hi
    w0 = sol["w"].copy()

    def full(v):
        w = w0.copy(); w[free] = v
        return w
    fun = lambda v: evalf(full(v), np.zeros(0))[0]
    jac = lambda v: evalf(full(v), np.zeros(0))[1][free]
    con = {"type": "eq", "fun": lambda v: evalf(full(v), np.zeros(0))[2][n:], "jac": lambda v: evalf(full(v), np.zeros(0))[3][n:][:, free]}
    rng = np.random.default_rng(0)
    start = np.clip(w0[free] + 0.02 * rng.standard_normal(free.sum()), lo[free] + 1e-6, hi[free] - 1e-6)
    r = minimize(fun, start, jac=jac, constraints=[con], bounds=list(zip(lo[free], hi[free])), method="SLSQP", options={"ftol": 1e-14, "maxiter": 400})
    assert np.abs(r.x - w0[free]).max() < 1e-5, np.abs(r.x - w0[free]).max()
    assert abs(r.fun - fun(w0[free])) < 1e-8


def test_estimator_nlp_of_this_example_is_a_convex_qp_with_the_oracles_answer(oprob):
    """With the input known the reactor is linear in its state, so mhe_opt's NLP is a strictly convex QP here: solved once more
    by the dense Mehrotra solver of the linear path's oracle (another algorithm, another file) - same estimate."""
    import mpc_oracle as o
    p = oprob
    S = eo.MheState(p)
    y = [np.array([0.9, 0.1]), np.array([0.6, 0.4]), np.array([0.55, 0.45])]
    us = [np.array([0.0]), np.array([0.4]), np.array([0.7])]
    for k in range(3):
        xes = eo.mhe_step(p, S, k, y[k], us[k])
    sol = S.last
    f, gf, g, J, H = sol["evalf"](sol["w"] * 0.0, np.zeros(len(sol["lam"])))      # a QP: data at the origin define it
    lo, hi = sol["lo"], sol["hi"]
    bounded = np.isfinite(lo) | np.isfinite(hi)
    qp = o.qp_ipm_dense(H, gf, J, -g, np.eye(len(lo))[bounded], lo[bounded], hi[bounded], tol=1e-12)
    assert qp["status"] == 0
    assert np.abs(qp["w"] - sol["w"]).max() < 1e-8


def test_repo_example_is_the_reference_example(oprob, pkg, ref_gold):
    """mpc-code_amd/examples/reactor_enmpc.py poses the problem of the reference's Ex_ENMPC.py: the oracle gives the loops it gave on the
    reference's file (tests/golden/reference_examples.npz; to rounding, as the vectors were computed on another host), and the product's
    loader read the reference file unmodified to what it reads of this one."""
    a = eo.closed_loop(oprob, 3)
    for k in ("U", "XS", "US", "X_ES", "P_K"):
        assert np.abs(a[k] - ref_gold["enmpc_loop_" + k]).max() < 1e-12, k
    q = pkg.load_problem(EX, overrides={"N": 40, "N_mhe": 20})
    assert (q.N, q.N_mhe, q.nx, q.nu, q.n_w, q.max_iter) == tuple(ref_gold["enmpc_N40"].tolist()) == (40, 20, 2, 1, 4, 200)


def test_extended_kalman_filter_variant_restatements_agree_and_reproduce_their_vectors():
    """The example's other estimator (Ex_ENMPC.py:109-123, mhe_mod = 'off': ekf() of Estimator.py:313-386 on [x; d], driven as MPC_code.py:640-650): the golden loops
    certify themselves, NumPy and C restatement agree to rounding, the saturation of the disturbance estimate (MPC_code.py:657-664) is active in the second set."""
    import enmpc_oracle_c as ec
    g = np.load(GOLD_EKF)
    for pre in ("ekf_", "sat_"):
        assert int(g[pre + "STATUS_DYN"].max()) == 0 and int(g[pre + "STATUS_SS"].max()) == 0
        assert float(g[pre + "KKT_DYN"].max()) < 2e-7 and float(g[pre + "KKT_SS"].max()) < 1e-8
    assert float(g["sat_D_HAT"].min()) == -0.05 and float(g["ekf_D_HAT"].min()) < -0.2      # the filter moves the disturbance, the box holds it
    assert abs(g["ekf_U"][-1, 0, 0] - 1.04297536) < 1e-6      # the same economic steady state as with the moving-horizon estimator
    for pre, over, n in (("ekf_", None, 8), ("sat_", {"dmin": g["sat_dmin"], "dmax": g["sat_dmax"]}, 12)):
        q = eo.load_problem(EX_EKF, overrides=over)
        assert q.ekf and not q.mhe
        r = eo.closed_loop(q, n, x0_p=g[pre + "x0"][1])
        c = ec.OracleEC(q).closed_loop(n, g[pre + "x0"], nthreads=0)
        for k in ("U", "XS", "US", "X_ES", "Xp"):
            assert np.abs(r[k] - g[pre + k][:n, 1]).max() < 1e-12, (pre, k)
            assert np.abs(c[k] - g[pre + k][:n]).max() < 1e-9, (pre, k)
        for k in ("STATUS_DYN", "STATUS_SS", "ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
            assert np.array_equal(c[k], g[pre + k][:n]), (pre, k)


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "tests", "golden", "ipopt_enmpc.npz")), reason="no IPOPT vectors (tools/make_ipopt_vectors.py econ needs CasADi)")
def test_ipopt_vectors_if_present(oprob):
    """Where a machine with CasADi has written tests/golden/ipopt_enmpc.npz: the restated interior point against IPOPT itself on the same discretised NLPs from the
    same guesses - solutions to 1e-6, return status, and the iteration counts side by side (equal where the restatement is faithful; reported, and required within 2)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "ipopt_enmpc.npz"), allow_pickle=True)
    n, m, N = oprob.nx, oprob.nu, oprob.N
    w0 = np.concatenate([np.concatenate([oprob.x0_m, oprob.u0])] * N + [oprob.x0_m])
    for i in range(len(g["D"])):
        ts = eo.target_solve(oprob, g["D"][i])
        assert (ts["status"] == 0) == (str(g["STATUS_T"][i]) == "Solve_Succeeded") and np.abs(ts["w"] - g["WT"][i]).max() < 1e-6
        assert abs(int(ts["iters"]) - int(g["ITERS_T"][i])) <= 2, (i, ts["iters"], g["ITERS_T"][i])
        sol = eo.ocp_solve(oprob, g["XHAT"][i], g["WT"][i][:n], g["WT"][i][n:n + m], g["D"][i], w0)
        assert (sol["status"] == 0) == (str(g["STATUS"][i]) == "Solve_Succeeded") and np.abs(sol["w"] - g["W"][i]).max() < 1e-6
        assert abs(int(sol["iters"]) - int(g["ITERS"][i])) <= 2, (i, sol["iters"], g["ITERS"][i])
    for i in range(len(g["MHE_N"]) if "MHE_N" in g.files else 0):      # the estimator's NLP (mhe_opt), windows of 1 .. N_mhe stages
        Nw = int(g["MHE_N"][i])
        Us, Ys = [np.asarray(r, dtype=float) for r in g["MHE_U"][i]], [np.asarray(r, dtype=float) for r in g["MHE_Y"][i]]
        evalf, lo, hi = eo.mhe_eval(oprob, Nw, Us, Ys, np.asarray(g["MHE_XBAR"][i], dtype=float), np.linalg.inv(np.asarray(g["MHE_P"][i], dtype=float)))
        sol = eo.ipm_dense(evalf, np.asarray(g["MHE_W0"][i], dtype=float), lo, hi, tol=1e-10, max_iter=oprob.max_iter)
        assert (sol["status"] == 0) == (str(g["MHE_STATUS"][i]) == "Solve_Succeeded") and np.abs(sol["w"] - np.asarray(g["MHE_W"][i], dtype=float)).max() < 1e-6, i
        assert abs(int(sol["iters"]) - int(g["MHE_ITERS"][i])) <= 2, (i, sol["iters"], g["MHE_ITERS"][i])


WHITE_NOISE = {"R_wn": 1e-6 * np.eye(2), "G_wn": 1e-2 * np.eye(2), "Q_wn": 1e-3 * np.eye(2), "N": 12, "N_mhe": 6}      # (Ex_ENMPC.py:68-69 carries G_wn / Q_wn commented out)


def test_white_noise_on_measurement_and_state_restatements_agree(pkg):
    """The reference's white noises of the loop (MPC_code.py:537-541 on the measurement, :822-827 on the plant state; unseeded there): handed the same draws, the NumPy and the C
    restatement give the same loop, the noise is in it, and the loader keeps the covariances (and says that the resident loop runs without them)."""
    import enmpc_oracle_c as ec
    from mpc_code_amd import enmpc
    with pytest.warns(UserWarning, match="simulated only on request"):
        p = pkg.load_problem(EX, overrides=WHITE_NOISE)
    assert np.array_equal(p.R_wn, WHITE_NOISE["R_wn"]) and np.array_equal(p.G_wn, WHITE_NOISE["G_wn"])
    V, W = enmpc.loop_noise(p, 8, 1, seed=5)
    assert V.shape == (8, 1, 2) and W.shape == (8, 1, 2) and abs(V.std() - 1e-3) < 5e-4 and abs(W.std() - 1e-2 * np.sqrt(1e-3)) < 2e-4
    q = eo.load_problem(EX, overrides={"N": 12, "N_mhe": 6})
    r, r0 = eo.closed_loop(q, 8, v_wn=V[:, 0], w_wn=W[:, 0]), eo.closed_loop(q, 8)
    c = ec.OracleEC(q).closed_loop(8, q.x0_p[None], nthreads=1, v_wn=V, w_wn=W)
    for k in ("U", "XS", "US", "X_ES", "Xp"):
        assert np.abs(r[k] - c[k][:, 0]).max() < 1e-9, k
    assert np.array_equal(r["STATUS_DYN"], c["STATUS_DYN"][:, 0]) and np.abs(r["X_ES"] - r0["X_ES"]).max() > 1e-4
    with pytest.raises(pkg.UnsupportedProblem):
        pkg.load_problem(EX, overrides={"G_wn": np.eye(2)})      # the state noise needs its covariance


W_BOUNDS = {"wmin": np.array([-1e-3, -1e-3, -0.02, -0.02]), "wmax": np.array([1e-3, 1e-3, 0.02, 0.02]), "N": 12, "N_mhe": 6}


def test_estimator_with_bounded_state_noise_restatements_agree():
    """mhe_opt's boxes on the state noise (wmin / wmax, Utilities.py:881-884,974-977): both restatements solve the estimator's NLP with them - the same loop to
    rounding - and the boxes matter (the estimate moves by 0.08 against the unbounded estimator's)."""
    import enmpc_oracle_c as ec
    q, q0 = eo.load_problem(EX, overrides=W_BOUNDS), eo.load_problem(EX, overrides={"N": 12, "N_mhe": 6})
    r, r0 = eo.closed_loop(q, 8), eo.closed_loop(q0, 8)
    c = ec.OracleEC(q).closed_loop(8, q.x0_p[None], nthreads=1)
    for k in ("U", "XS", "US", "X_ES", "Xp"):
        assert np.abs(r[k] - c[k][:, 0]).max() < 1e-9, k
    for k in ("STATUS_DYN", "STATUS_SS", "STATUS_MHE", "ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
        assert np.array_equal(r[k], c[k][:, 0]), k
    assert int(r["STATUS_MHE"].max()) == 0 and np.abs(r["X_ES"] - r0["X_ES"]).max() > 0.05


def test_reference_example_with_its_estimator_switch_off_is_the_filter_variant(pkg, ref_gold):
    """The switch is a source line of the reference's file (mhe_mod = 'on', Ex_ENMPC.py:109), evaluated while the file runs: a copy with that one line changed
    loaded in both loaders as the extended-Kalman-filter problem (tests/golden/make_reference_golden.py) and gives the loops of
    mpc-code_amd/examples/reactor_enmpc_ekf.py (to rounding: the stored loops were computed on another host)."""
    own = eo.load_problem(EX_EKF)
    assert ref_gold["ekf_flags"].tolist() == [True, False] and own.ekf and not own.mhe
    assert_fields(own, ref_gold, "ekf_", ("Q_kf", "R_kf", "P0"))
    a = eo.closed_loop(own, 3)
    for k in ("U", "XS", "US", "X_ES", "P_K"):
        assert np.abs(a[k] - ref_gold["ekf_loop_" + k]).max() < 1e-12, k
    q = pkg.load_problem(EX_EKF, overrides={"N": 40})
    assert (q.estimator, q.N, q.nx, q.nu) == (str(ref_gold["ekf_pkg_estimator"]), *ref_gold["ekf_pkg_dims"].tolist()) == ("ekf", 40, 2, 1)
    assert np.array_equal(q.Q_kf, ref_gold["ekf_pkg_Q_kf"]) and np.array_equal(q.R_kf, ref_gold["ekf_pkg_R_kf"])


# ---------------------------------------------------------------------------------------------------------------------------------
# product, host side
# ---------------------------------------------------------------------------------------------------------------------------------
def test_loader_classifies_and_refuses(pkg, prob):
    from mpc_code_amd import EconomicMPCProblem, UnsupportedProblem
    assert isinstance(prob, EconomicMPCProblem) and (prob.N, prob.N_mhe, prob.quad_steps, prob.max_iter) == (25, 10, 20, 200)
    assert np.array_equal(prob.xmax_mhe, [1.0, 1.0, np.inf, np.inf]) and np.array_equal(prob.x_bar, [1.2, 0.5, 0.0, 0.0])
    assert pkg.load_problem(EX, overrides={"mhe_up": "filter"}).mhe_up == "filter" and prob.mhe_up == "smooth"
    for over in ({"mhe_up": "window"}, {"slacks": True}, {"N": 80}, {"N_mhe": 64}, {"StateFeedback": False}, {"TermCons": True}, {"ekf": True}, {"mhe": False}):
        with pytest.raises(UnsupportedProblem):      # (the last two: both estimators, none)
            pkg.load_problem(EX, overrides=over)
    pw = pkg.load_problem(EX, overrides=W_BOUNDS)
    assert np.array_equal(pw.wmax, W_BOUNDS["wmax"]) and np.all(np.isinf(prob.wmin)) and np.all(np.isinf(prob.wmax))
    with pytest.raises(UnsupportedProblem):      # the output noise is eliminated from the estimator's NLP here: no boxes on it
        pkg.load_problem(EX, overrides={"vmax": np.array([0.1, 0.1])})
    pe = pkg.load_problem(EX_EKF)
    assert prob.estimator == "mhe" and pe.estimator == "ekf" and np.array_equal(np.diag(pe.Q_kf), [1e-8, 1e-8, 1.0, 1.0]) and np.array_equal(pe.P0, 1e-8 * np.eye(4))
    with pytest.raises(UnsupportedProblem):
        pkg.load_problem(EX_EKF, overrides={"Q_kf": None})


@pytest.fixture(scope="module")
def shim(prob, tmp_path_factory):
    """the generated model code + the Runge-Kutta sensitivity driver of the product, compiled for the host"""
    from mpc_code_amd import econcodegen
    d = tmp_path_factory.mktemp("enmpc_shim")
    hdr = os.path.join(d, "model.hpp")
    with open(hdr, "w") as fh:
        fh.write(econcodegen.emit_econ_header(prob))
    so = os.path.join(d, "shim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-D__device__=", "-D__host__=", "-D__forceinline__=inline", f'-DMPC_EC_MODEL_HEADER="{hdr}"',
                           "-o", so, os.path.join(ROOT, "tests", "enmpc_host_shim.cpp")])
    return ct.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_double))


def test_generated_sensitivities_match_complex_step_derivatives(shim, oprob):
    """What the kernels integrate - state, cost quadrature, first and second forward sensitivities through the Runge-Kutta stages, from
    the traced and generated code - against the oracle's complex-step / finite-difference derivatives of the Ex-file's own functions."""
    p = oprob
    n, m = p.nx, p.nu
    NP, NPP = n + m, (n + m) * (n + m + 1) // 2
    rng = np.random.default_rng(5)
    for _ in range(5):
        x = rng.uniform(0.05, 0.95, n); u = rng.uniform(0.05, 1.9, m); d = rng.uniform(-0.1, 0.1, p.nd); xs = rng.uniform(0.2, 0.8, n); us = rng.uniform(0.2, 1.5, m)
        xn = np.zeros(n + 1); S = np.zeros((n + 1, NP)); T = np.zeros((n + 1, NPP))
        shim.shim_ocp(_ptr(x), _ptr(u), _ptr(d), _ptr(xs), _ptr(us), ct.c_double(p.h), ct.c_int(p.quad_steps), _ptr(xn), _ptr(S), _ptr(T))
        D = d.reshape(-1, 1)
        fun = lambda Zc: np.vstack(eo.ocp_stage(p, Zc[:n], Zc[n:], D, xs.reshape(-1, 1), us.reshape(-1, 1)))
        v, J = eo.jac_cs(fun, np.concatenate([x, u]))
        assert np.abs(xn - v).max() < 1e-13 and np.abs(S - J).max() < 1e-12
        for r in range(n + 1):
            H = eo.hess_fd(lambda Zc: fun(Zc)[r], np.concatenate([x, u]))
            Hp = np.zeros((NP, NP)); Hp[np.triu_indices(NP)] = T[r]; Hp = Hp + np.triu(Hp, 1).T
            assert np.abs(Hp - H).max() < 5e-8 * max(1.0, np.abs(H).max()), (r, np.abs(Hp - H).max())
        # the model alone (target, hold rule) and the plant
        xm = np.zeros(n); Sm = np.zeros((n, NP)); Tm = np.zeros((n, NPP))
        shim.shim_mdl(_ptr(x), _ptr(u), _ptr(d), ct.c_double(p.h), _ptr(xm), _ptr(Sm), _ptr(Tm))
        fm = lambda Zc: eo.fx_model(p, Zc[:n], Zc[n:], np.zeros((p.nd, 1)))      # (Bd d is added outside the integrator)
        v, J = eo.jac_cs(fm, np.concatenate([x, u]))
        assert np.abs(xm - v).max() < 1e-13 and np.abs(Sm - J).max() < 1e-12
        xpn = np.zeros(n)
        shim.shim_plant(_ptr(x), _ptr(u), ct.c_double(p.h), _ptr(xpn))
        assert np.abs(xpn - eo.fx_plant(p, x.reshape(-1, 1), u.reshape(-1, 1))[:, 0]).max() < 1e-14
        # estimator model: sensitivities with respect to the state only
        xe = np.zeros(n); Se = np.zeros((n, n)); Te = np.zeros((n, n * (n + 1) // 2))
        shim.shim_mhe(_ptr(x), _ptr(u), ct.c_double(p.h), _ptr(xe), _ptr(Se), _ptr(Te))
        fe = lambda Zc: eo.fx_mhe(p, np.vstack([Zc, np.zeros_like(Zc)]), u.reshape(-1, 1), np.zeros((p.n_w, 1)))[:n]
        v, J = eo.jac_cs(fe, x)
        assert np.abs(xe - v).max() < 1e-13 and np.abs(Se - J).max() < 1e-12


def test_generated_cost_functions_match_the_example(shim, oprob):
    p = oprob
    rng = np.random.default_rng(6)
    w = rng.uniform(0.1, 1.0, 5); f = np.zeros(1); g = np.zeros(5); H = np.zeros((5, 5))
    shim.shim_fss(_ptr(w), _ptr(f), _ptr(g), _ptr(H))
    cost = lambda Wc: np.array([p.fssobj(Wc[:2, i], Wc[2:3, i], Wc[3:, i], None, None, None) for i in range(Wc.shape[1])])
    v, J = eo.jac_cs(lambda Wc: cost(Wc)[None], w)
    assert abs(f[0] - v[0]) < 1e-15 and np.abs(g - J[0]).max() < 1e-14 and np.abs(H - eo.hess_fd(cost, w)).max() < 1e-7
    x = rng.uniform(0, 1, 2); xs = rng.uniform(0, 1, 2); g2 = np.zeros(2); H2 = np.zeros((2, 2))
    shim.shim_vfin(_ptr(x), _ptr(xs), _ptr(f), _ptr(g2), _ptr(H2))
    assert abs(f[0] - p.vfin(x, xs)) < 1e-10 and np.abs(H2 - 4000.0 * np.eye(2)).max() < 1e-9 and np.abs(g2 - 4000.0 * (x - xs)).max() < 1e-9
    wv = rng.standard_normal(6); g3 = np.zeros(6); H3 = np.zeros((6, 6))
    shim.shim_cmhe(_ptr(wv), _ptr(f), _ptr(g3), _ptr(H3))
    assert abs(f[0] - p.fobj_mhe(wv[:4], wv[4:], 0.0)) < 1e-14 and np.abs(g3 - wv).max() < 1e-15 and np.abs(H3 - np.eye(6)).max() < 1e-15


def test_capi_exports_every_declared_symbol(prob):
    """the per-model library builds for gfx950 and exports what include/mpc_enmpc.h declares (no compute call without a GPU)"""
    from mpc_code_amd import econcodegen, enmpc
    lib = ct.CDLL(econcodegen.build_enmpc_library(prob))
    hdr = open(os.path.join(ROOT, "include", "mpc_enmpc.h")).read()
    declared = set(re.findall(r"\b(enmpc_[a-z_]+)\s*\(", hdr))
    assert declared == set(enmpc.ENMPC_EXPORTS)
    for s in declared:
        assert hasattr(lib, s), s
    lib.enmpc_build_info.restype = ct.c_char_p
    assert lib.enmpc_build_info().decode().startswith("gfx950;enmpc;dims=2/1/2/2/2/4;mx=10")
    src = open(os.path.join(ROOT, "mpc-code_amd", "enmpc.py")).read() + open(os.path.join(ROOT, "mpc-code_amd", "econcodegen.py")).read() + open(os.path.join(ROOT, "mpc-code_amd", "econproblem.py")).read()
    assert "oracle" not in src.replace("the oracle", "") or "import enmpc_oracle" not in src      # the product never touches the checker
    assert "enmpc_oracle" not in src and "exnum" not in src


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the HIP path through the C-ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def _gpu_loop(pkg, over, x0, nsteps, **kw):
    from mpc_code_amd import enmpc
    p = pkg.load_problem(EX, overrides=over)
    return p, enmpc.run_enmpc_closed_loop(p, x0, nsteps, **kw)


def _check(r, gold, pre, nsteps):
    for k in ("U", "XS", "US", "X_ES", "X_HAT", "Xp", "D_HAT"):
        assert np.abs(r[k] - gold[pre + k][:nsteps]).max() < TOL_U, (pre, k, np.abs(r[k] - gold[pre + k][:nsteps]).max())
    for k in ("STATUS_DYN", "STATUS_SS"):
        assert np.array_equal(r[k], gold[pre + k][:nsteps]), (pre, k)
    # the same path, not only the same end: interior-point iteration counts of all three NLPs equal the oracle's at every step
    for k in ("ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
        assert np.array_equal(r[k], gold[pre + k][:nsteps]), (pre, k, r[k].T.tolist(), gold[pre + k][:nsteps].T.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [1, 2])
def test_gpu_shipped_example_follows_the_golden_loop(pkg, gold, kernel):
    p, r = _gpu_loop(pkg, None, gold["ship_x0"], 21, kernel=kernel)
    _check(r, gold, "ship_", 21)
    assert int(r["STATUS_MHE"].max()) == 0
    # the reference's other result arrays (MPC_code.py:877-895): measurement = plant state (StateFeedback), model outputs with the output disturbance
    assert np.array_equal(r["Yp"], r["Xp"]) and np.allclose(r["YS"], gold["ship_XS"][:21] + gold["ship_D_HAT"][:21] @ p.Cd.T, atol=TOL_U)
    assert np.allclose(r["Y_HAT"][1:], gold["ship_X_HAT"][1:21] + gold["ship_D_HAT"][:20] @ p.Cd.T, atol=TOL_U) and np.allclose(r["Y_HAT"][0], gold["ship_X_HAT"][0])
    assert r["TIME_DYN"].shape == (21,) and r["TIME_DYN"].min() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [1, 2])
def test_gpu_baseline_config_horizons_follow_the_golden_loops(pkg, gold, kernel):
    p, r = _gpu_loop(pkg, {"N": 40}, gold["c4_x0"], 10, kernel=kernel)           # BASELINE configs[3]: N = 40
    _check(r, gold, "c4_", 10)
    p, r = _gpu_loop(pkg, {"N_mhe": 20}, gold["c5_x0"], 24, kernel=kernel)       # BASELINE configs[4]: N_mhe = 20, through the window's filling
    _check(r, gold, "c5_", 24)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [1, 2, 64])
def test_gpu_filter_update_of_the_arrival_cost_follows_the_golden_loop(pkg, gold, kernel):
    """mhe_up = 'filter' (Estimator.py:627-649,740-748): the arrival weight takes one Kalman step at the first entries of the lists of
    one-step predictions and noises, the prior mean becomes the list's first prediction - through the filling of the window and beyond."""
    p, r = _gpu_loop(pkg, {"mhe_up": "filter", "N_mhe": 6}, gold["flt_x0"], 16, kernel=kernel)
    _check(r, gold, "flt_", 16)
    p, q = _gpu_loop(pkg, {"mhe_up": "filter", "N_mhe": 6}, gold["flt_x0"], 16, kernel=kernel, steps_per_launch=5)      # the lists through HBM between launches
    assert np.array_equal(q["U"], r["U"]) and np.array_equal(q["X_ES"], r["X_ES"])


@pytest.mark.gpu
@pytest.mark.parametrize("pre", ["ekf_", "sat_"])
def test_gpu_extended_kalman_filter_follows_the_golden_loops_and_the_c_restatement(pkg, pre, B=200):
    """The example with its estimator switch in the other position (Ex_ENMPC.py:109-123): the extended Kalman filter on [x; d] in the estimator's place
    (enmpc_ekf_kernel / phase_ekf; Estimator.py:313-386 through MPC_code.py:640-664), both launch styles against the golden loops, a larger batch against the C
    restatement, and the per-call seam (whose estimator call is then the filter) against the resident loop bit for bit."""
    import enmpc_oracle_c as ec
    from mpc_code_amd import enmpc
    g = np.load(GOLD_EKF)
    over = {"dmin": g["sat_dmin"], "dmax": g["sat_dmax"]} if pre == "sat_" else None
    p = pkg.load_problem(EX_EKF, overrides=over)
    n = g[pre + "U"].shape[0]
    s = enmpc.EnmpcSolver(p)
    try:
        for kernel in (1, 2):
            r = enmpc.run_enmpc_closed_loop(p, g[pre + "x0"], n, solver=s, kernel=kernel)
            _check(r, g, pre, n)
            assert int(r["STATUS_MHE"].max()) == 0 and int(r["ITERS_MHE"].max()) == 0
        x0 = np.random.default_rng(3).uniform([0.5, 0.0], [1.0, 0.5], size=(B, 2))      # (B: the kernel source on the CPU test suite's wave emulator takes a handful)
        c = ec.OracleEC(eo.load_problem(EX_EKF, overrides=over)).closed_loop(10, x0, nthreads=0)
        a = enmpc.run_enmpc_closed_loop(p, x0, 10, solver=s, kernel=2)
        for k in ("U", "XS", "US", "X_ES", "Xp"):
            assert np.abs(a[k] - c[k]).max() < TOL_U, (k, np.abs(a[k] - c[k]).max())
        for k in ("STATUS_DYN", "STATUS_SS", "ITERS_DYN", "ITERS_SS"):
            assert np.array_equal(a[k], c[k]), k
        b = enmpc.run_enmpc_stepwise(p, x0, 10, solver=s)
        for k in ("U", "X_HAT", "XS", "US", "Xp", "D_HAT", "X_ES", "STATUS_DYN", "STATUS_SS", "ITERS_DYN", "ITERS_SS"):
            assert np.array_equal(a[k], b[k]), k
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("more", [{}, {"mhe_up": "filter", "N_mhe": 18}])
def test_gpu_estimator_with_bounded_state_noise_follows_the_c_restatement(pkg, more, B=70):
    """wmin / wmax (Utilities.py:881-884,974-977): the library generated for such a problem (build info wb=1) carries the boxes of the noise in the estimator's
    solver - every launch style against the C restatement on 70 starts, the seam against the resident loop; a library generated without them refuses them."""
    import warnings
    import enmpc_oracle_c as ec
    from mpc_code_amd import enmpc, econcodegen
    from mpc_code_amd.capi import MpcAmdError
    over = dict(W_BOUNDS, **more)
    K = 24 if more else 12
    x0 = np.random.default_rng(3).uniform([0.5, 0.0], [1.0, 0.5], size=(B, 2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = pkg.load_problem(EX, overrides=over)
        c = ec.OracleEC(eo.load_problem(EX, overrides=over)).closed_loop(K, x0, nthreads=0)
    assert int(c["STATUS_MHE"].max()) == 0
    s = enmpc.EnmpcSolver(p)
    try:
        assert s.lib.enmpc_build_info().decode().endswith("wb=1")
        for kernel in (1, 2, 64):
            r = enmpc.run_enmpc_closed_loop(p, x0, K, solver=s, kernel=kernel)
            for k in ("U", "XS", "US", "X_ES", "Xp"):
                assert np.abs(r[k] - c[k]).max() < TOL_U, (kernel, k, np.abs(r[k] - c[k]).max())
            for k in ("STATUS_DYN", "STATUS_SS", "STATUS_MHE", "ITERS_DYN", "ITERS_SS"):
                assert np.array_equal(r[k], c[k]), (kernel, k)
            d = np.abs(r["ITERS_MHE"].astype(int) - c["ITERS_MHE"])      # (tol 1e-10: 'E_0 <= tol' an iteration apart in a few per cent of the solves, as in the randomised models)
            assert d.max() <= 1 and (d != 0).mean() < 0.05, (kernel, int((d != 0).sum()))
        a, b = enmpc.run_enmpc_closed_loop(p, x0, K, solver=s, kernel=2), enmpc.run_enmpc_stepwise(p, x0, K, solver=s)
        for k in ("U", "X_HAT", "XS", "US", "Xp", "D_HAT", "X_ES", "STATUS_MHE", "ITERS_MHE", "ITERS_DYN"):
            assert np.array_equal(a[k], b[k]), k
    finally:
        s.close()
    if not more:
        with pytest.raises(MpcAmdError):      # the shipped example's library has no rows for them
            enmpc.EnmpcSolver(p, lib_path=econcodegen.build_enmpc_library(pkg.load_problem(EX)))


@pytest.mark.gpu
def test_gpu_white_noise_through_the_per_call_seam_follows_the_c_restatement(pkg):
    """Measurement and state noise of the loop (MPC_code.py:537-541, :822-827) are the caller's side of the per-call seam: run_enmpc_stepwise(noise_seed=...) draws them, the C
    restatement handed the same draws gives the same loop - forty histories from the shipped start."""
    import warnings
    import enmpc_oracle_c as ec
    from mpc_code_amd import enmpc
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = pkg.load_problem(EX, overrides=WHITE_NOISE)
    B, K = 40, 14
    x0 = np.tile(p.x0_p, (B, 1))
    r = enmpc.run_enmpc_stepwise(p, x0, K, noise_seed=3)
    assert r["V_WN"].shape == (K, B, 2) and r["W_WN"].shape == (K, B, 2) and np.abs(r["U"][:, 0] - r["U"][:, 1]).max() > 0
    c = ec.OracleEC(eo.load_problem(EX, overrides={"N": 12, "N_mhe": 6})).closed_loop(K, x0, nthreads=0, v_wn=r["V_WN"], w_wn=r["W_WN"])
    for k in ("STATUS_DYN", "STATUS_SS", "STATUS_MHE"):
        assert np.array_equal(r[k], c[k]), k
    tied = any((r[k] != c[k]).any() for k in ("ITERS_DYN", "ITERS_SS", "ITERS_MHE"))
    for k in ("U", "XS", "US", "X_ES", "Xp"):
        assert np.abs(r[k] - c[k]).max() < (2e-6 if tied else TOL_U), (k, tied, np.abs(r[k] - c[k]).max())
    # ... and in the RESIDENT loop (enmpc_set_noise: the draws on the device, one row per step and instance): the split pipeline is the seam's noisy loop to the bit (the same
    # kernels), the one-launch kernel follows the C restatement; switched off again the loop is the deterministic one
    for kernel in (2, 1):
        a = enmpc.run_enmpc_closed_loop(p, x0, K, kernel=kernel, noise_seed=3)
        assert np.array_equal(a["V_WN"], r["V_WN"]) and np.array_equal(a["W_WN"], r["W_WN"]) and np.array_equal(a["Yp"], a["Xp"] + a["V_WN"])
        for k in ("U", "XS", "US", "X_ES", "Xp", "D_HAT", "X_HAT"):
            if kernel == 2:
                assert np.array_equal(a[k], r[k]), k
            elif k in c:
                assert np.abs(a[k] - c[k]).max() < 2e-6, (k, np.abs(a[k] - c[k]).max())
        assert np.array_equal(a["STATUS_DYN"], c["STATUS_DYN"]) and np.array_equal(a["STATUS_MHE"], c["STATUS_MHE"])
    b0, b1 = enmpc.run_enmpc_closed_loop(p, x0[:3], K, kernel=2), enmpc.run_enmpc_stepwise(p, x0[:3], K)
    assert np.array_equal(b0["U"], b1["U"]) and np.abs(b0["U"][:, 0] - b0["U"][:, 1]).max() == 0.0


@pytest.mark.gpu
def test_gpu_launch_boundaries_and_launch_styles_do_not_change_the_loop(pkg, gold):
    x0 = np.vstack([gold["ship_x0"], gold["c4_x0"]])
    p, a = _gpu_loop(pkg, None, x0, 14, kernel=1)                # one launch for all steps: the state stays in registers
    p, b = _gpu_loop(pkg, None, x0, 14, steps_per_launch=3, kernel=1)      # state, window and lists through HBM between launches
    p, c = _gpu_loop(pkg, None, x0, 14, kernel=2)                # split pipeline: a launch per phase and step, target with lane = instance
    for k in ("U", "XS", "US", "X_ES", "X_HAT", "Xp", "D_HAT", "ITERS_DYN", "ITERS_SS", "ITERS_MHE", "STATUS_DYN", "STATUS_SS", "STATUS_MHE"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    for k in ("U", "XS", "X_ES"):
        assert np.abs(c[k][:, 0] - gold["ship_" + k][:14, 0]).max() < TOL_U, k
    # two and four instances side by side in a wave (segments of 32 / 16 lanes): N = 25, N_mhe = 10 take 32 / 16, and a ragged batch
    # leaves segments without an instance
    xr = np.vstack([x0, x0[::-1], x0[:3]])
    p, a = _gpu_loop(pkg, None, xr, 14, kernel=64)
    for seg in (32, 16):
        p, b = _gpu_loop(pkg, None, xr, 14, kernel=seg)
        for k in ("U", "XS", "US", "X_ES", "X_HAT", "Xp", "D_HAT"):
            assert np.abs(a[k] - b[k]).max() < 1e-12, (seg, k, np.abs(a[k] - b[k]).max())
        for k in ("ITERS_DYN", "ITERS_SS", "ITERS_MHE", "STATUS_DYN", "STATUS_SS", "STATUS_MHE"):
            assert np.array_equal(a[k], b[k]), (seg, k)
    # the split pipeline's groups of the batch on streams of their own: the same loop whatever their number (ragged last group included)
    xg = np.tile(x0, (90, 1))[:347]
    p, a = _gpu_loop(pkg, None, xg, 6, kernel=2, groups=1)
    for G in (2, 3, 8):
        p, b = _gpu_loop(pkg, None, xg, 6, kernel=2, groups=G)
        for k in ("U", "XS", "X_ES", "Xp", "ITERS_DYN", "ITERS_MHE", "STATUS_DYN"):
            assert np.array_equal(a[k], b[k]), (G, k)
    p, b = _gpu_loop(pkg, {"N": 12, "N_mhe": 5}, xr, 9, kernel=16)      # both horizons in 16 lanes: four OCPs per wave too
    p, a = _gpu_loop(pkg, {"N": 12, "N_mhe": 5}, xr, 9, kernel=1)
    for k in ("U", "X_ES", "XS"):
        assert np.abs(a[k] - b[k]).max() < 1e-12, k
    assert np.array_equal(a["ITERS_DYN"], b["ITERS_DYN"]) and np.array_equal(a["ITERS_MHE"], b["ITERS_MHE"])


@pytest.mark.gpu
def test_gpu_full_size_batches(pkg):
    """BASELINE configs[3] at one GPU's share and at the whole batch (N = 40; 16384 and 131072 instances), configs[4] at its whole
    batch (N_mhe = 20; 32768): every NLP of every instance solved, bounds kept, the loop invariant under a permutation of the batch,
    the economics reached - and instances picked from the batch re-run by the oracle."""
    from mpc_code_amd import enmpc
    rng = np.random.default_rng(20250614)
    x0 = rng.uniform([0.5, 0.0], [1.0, 0.5], size=(131072, 2))
    p = pkg.load_problem(EX, overrides={"N": 40})
    s = enmpc.EnmpcSolver(p)
    r = enmpc.run_enmpc_closed_loop(p, x0, 4, solver=s)
    for k in ("STATUS_SS", "STATUS_MHE"):
        assert int(r[k].max()) == 0, k
    # The OCP of the cold step - far from its guess - is the one NLP here whose line search can run out of step lengths (17 of the 131072 cold solves): IPOPT then
    # enters its restoration phase, and so do the kernels since round 5 (the rare path: enmpc_ocp_resto_kernel behind every OCP launch) - these OCPs solve in 25 iterations.
    assert int(r["STATUS_DYN"].max()) == 0, np.unique(r["STATUS_DYN"], return_counts=True)
    assert r["U"].min() >= 0.0 and r["U"].max() <= 2.0 and np.isfinite(r["X_ES"]).all()
    assert r["XS"].min() >= 0.0 and r["XS"].max() <= 1.0 and r["X_ES"][..., :2].min() >= -1e-9 and r["X_ES"][..., :2].max() <= 1.0 + 1e-9
    sub = x0[:16384]
    a = enmpc.run_enmpc_closed_loop(p, sub, 12, solver=s)
    assert np.array_equal(a["U"][:4], r["U"][:4, :16384])                       # an instance does not see its neighbours
    perm = rng.permutation(16384)
    b = enmpc.run_enmpc_closed_loop(p, sub[perm], 12, solver=s)
    assert np.array_equal(b["U"], a["U"][:, perm]) and np.array_equal(b["ITERS_DYN"], a["ITERS_DYN"][:, perm])
    assert int(a["STATUS_DYN"].max()) == 0 and int(a["STATUS_MHE"].max()) == 0 and int(a["STATUS_SS"].max()) == 0
    assert int(a["ITERS_DYN"][0, 6907]) == 25 and int(a["ITERS_DYN"][0, 9079]) == 25      # the two cold OCPs of this share that go through the restoration phase (test_wave_emu.py has them on the CPU)
    # economics: after 12 steps every loop is heading to the profit-optimal feed rate, the targets already sit there
    assert np.abs(a["US"][-1] - 1.0430).max() < 0.05 and np.abs(a["U"][-1] - 1.0430).max() < 0.2
    s.close()
    q = eo.load_problem(EX, overrides={"N": 40})
    for i in (0, 7777, 16383):
        o = eo.closed_loop(q, 4, x0_p=sub[i])
        for k in ("U", "XS", "US", "X_ES"):
            assert np.abs(a[k][:4, i] - o[k]).max() < TOL_U, (i, k)
        assert a["ITERS_DYN"][:4, i].tolist() == o["ITERS_DYN"].tolist()
    # EVERY instance of the per-GPU share, every step, against the C restatement on the host cores: values, status words and the
    # interior-point iteration counts of all three NLPs
    import enmpc_oracle_c as ec

    def same_loop(g, cc, ns_, what):
        """Two implementations of the same algorithm: every status word equal; interior-point iteration counts equal except where a decision (E_0 <= tol,
        E_mu <= 10 mu, an acceptance test of the line search) sits within rounding of its threshold - then one of them takes an iteration or two more towards
        the same point, and from there on the instance's values differ by what the tolerance allows: 1e-8 on the problem as IPOPT scales it, 3e-7 in the
        OCP's own units.  Instances without such a tie agree to TOL_U."""
        for k in ("STATUS_DYN", "STATUS_SS", "STATUS_MHE"):
            assert np.array_equal(g[k][:ns_], cc[k]), (what, k, int((g[k][:ns_] != cc[k]).sum()))
        tied = np.zeros(cc["U"].shape[1], dtype=bool)
        for k in ("ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
            d = np.abs(g[k][:ns_].astype(int) - cc[k].astype(int))
            assert (d != 0).mean() < 5e-3 and d.max() <= 4, (what, k, int((d != 0).sum()), int(d.max()))
            tied |= (d != 0).any(axis=0)
        for k in ("U", "XS", "US", "X_ES", "Xp"):
            dv = np.abs(g[k][:ns_] - cc[k]).max(axis=(0, 2))
            assert dv[~tied].max() < TOL_U and dv.max() < 2e-6, (what, k, float(dv[~tied].max()), float(dv.max()), int(tied.sum()))
    nc_ = 5      # (the cold step and four warm ones: 82 k instance-steps, about a minute of the box's host cores; 12 steps: tools/enmpc_fullsize_check.py)
    c = ec.OracleEC(q).closed_loop(nc_, sub, nthreads=64)
    same_loop(a, c, nc_, "configs[3]")
    p5 = pkg.load_problem(EX, overrides={"N_mhe": 20})
    r5 = enmpc.run_enmpc_closed_loop(p5, x0[:32768], 23)
    for k in ("STATUS_SS", "STATUS_MHE"):
        assert int(r5[k].max()) == 0, k
    assert int(r5["STATUS_DYN"].max()) == 0
    q5 = eo.load_problem(EX, overrides={"N_mhe": 20})
    o = eo.closed_loop(q5, 23, x0_p=x0[31000])
    for k in ("U", "X_ES"):
        assert np.abs(r5[k][:, 31000] - o[k]).max() < TOL_U, k
    c5 = ec.OracleEC(q5).closed_loop(23, x0[:2048], nthreads=64)      # half of configs[4]'s per-GPU share through the filling of the window, every step
    same_loop({k: v[:, :2048] for k, v in r5.items() if isinstance(v, np.ndarray) and v.ndim >= 2}, c5, 23, "configs[4]")


@pytest.mark.gpu
@pytest.mark.parametrize("over,B", [(None, 70), ({"N": 40}, 5000), ({"mhe_up": "filter", "N_mhe": 6}, 9)])
def test_gpu_the_three_solver_calls_of_a_step_reproduce_the_fused_loop(pkg, over, B):
    """The per-call seam of include/mpc_enmpc.h - enmpc_mhe_update, enmpc_target_solve, enmpc_ocp_solve: the reference's defEstimator(..., 'mhe'),
    solver_ss(...), solver(...) of one step (MPC_code.py:577-650, :704-709, :776-781) for the whole batch, caller-owned host arrays - with the device's
    plant in between is the fused closed loop BIT FOR BIT: values, status words, iteration counts, through the filling of the window; with a plant
    of the caller's (NumPy Runge-Kutta, as the reference's Fx_p) it is the same loop to rounding."""
    from mpc_code_amd import enmpc
    p = pkg.load_problem(EX, overrides=over)
    x0 = np.random.default_rng(11).uniform([0.5, 0.0], [1.0, 0.5], size=(B, 2))
    ns = 14
    s = enmpc.EnmpcSolver(p)
    try:
        a = enmpc.run_enmpc_closed_loop(p, x0, ns, solver=s, kernel=2)
        b = enmpc.run_enmpc_stepwise(p, x0, ns, solver=s)
        for k in ("U", "X_HAT", "XS", "US", "Xp", "D_HAT", "X_ES", "STATUS_DYN", "STATUS_SS", "STATUS_MHE", "ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
            assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k].astype(float) - b[k].astype(float)).max()))
        if B <= 100:
            q = eo.load_problem(EX, overrides=over)      # the caller's plant: the Ex-file's User_fxp_Cont in NumPy, Mx Runge-Kutta steps (Utilities.py:58-82)
            c = enmpc.run_enmpc_stepwise(p, x0, ns, solver=s, plant=lambda x, u: eo.fx_plant(q, x.T, u.T).T)
            assert np.abs(c["U"] - a["U"]).max() < 1e-9 and np.array_equal(c["STATUS_DYN"], a["STATUS_DYN"])
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_sweeps_as_scans_and_as_recursions_agree(pkg):
    """The OCP's backward matrix sweep and its forward sweep run as parallel scans over the lanes (mpc_enmpc.hpp:ric_backward_scan, ric_forward); a wave in which a stage lacks
    curvature of its own runs the recursions, and -DEC_SWEEP_SERIAL builds them alone (a library of its own, built by __graft_entry__.build).  Both builds on BASELINE configs[3]'s
    horizon, 1024 starts, 12 steps from the cold start: every status word and every iteration count of the three NLPs equal, values to 1e-7 - and not the same bits."""
    from mpc_code_amd import enmpc, econcodegen
    p = pkg.load_problem(EX, overrides={"N": 40, "N_mhe": 10})
    x0 = np.random.default_rng(9).uniform([0.5, 0.0], [1.0, 0.5], size=(1024, 2))
    res = {}
    for name, flags in (("scans", []), ("recursions", ["-DEC_SWEEP_SERIAL"])):
        s = enmpc.EnmpcSolver(p, lib_path=econcodegen.build_enmpc_library(p, extra_flags=flags))
        try:
            res[name] = enmpc.run_enmpc_closed_loop(p, x0, 12, solver=s, kernel=2)
        finally:
            s.close()
    a, b = res["scans"], res["recursions"]
    for k in ("STATUS_DYN", "STATUS_SS", "STATUS_MHE", "ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
        assert np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))
    assert int(a["STATUS_DYN"].max()) == 0
    for k in ("U", "XS", "US", "X_ES", "Xp"):
        assert np.abs(a[k] - b[k]).max() < 1e-7, (k, np.abs(a[k] - b[k]).max())
    assert not np.array_equal(a["U"], b["U"])


@pytest.mark.gpu
@pytest.mark.parametrize("over,what", [({"xmin": np.array([0.8, 0.8]), "N": 12}, "ocp"), ({"xmin_ss": np.array([0.8, 0.8]), "N": 12}, "target")])
def test_gpu_unreachable_boxes_take_the_hold_branches(pkg, over, what):
    """Boxes no trajectory / no steady state of the reactor can reach (cA + cB <= cA0 = 1; both >= 0.8 asked for).  The reference's IPOPT answers
    'Infeasible_Problem_Detected' and the driver holds the input and propagates the model (MPC_code.py:786-805) or keeps the previous targets (:714-718).
    Here the restoration phase - the OCP's (since round 5: the kernels' rare path) or the target's - ends at a minimiser of the infeasibility (status 2:
    'Infeasible_Problem_Detected') after some twenty to fifty iterations, not at the iteration limit with an unconverged iterate applied (round 3) - and the loop goes on:
    every status word, iteration count and value as in the C restatement."""
    import warnings
    import enmpc_oracle_c as ec
    from mpc_code_amd import enmpc
    x0 = np.array([[0.9, 0.1], [0.6, 0.3], [0.7, 0.2]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = pkg.load_problem(EX, overrides=over)
        c = ec.OracleEC(eo.load_problem(EX, overrides=over)).closed_loop(5, x0, nthreads=3)
    assert (c["STATUS_SS"] == 2).all() and int(c["ITERS_SS"].max()) < 40 and int(c["ITERS_DYN"].max()) < (70 if what == "ocp" else 40)      # (the OCP's restoration phase converges to a minimiser of the infeasibility: some fifty iterations)
    if what == "ocp":
        assert (c["STATUS_DYN"] == 2).all() and np.all(c["U"] == p.u0[0])      # the input is held at u0
    else:
        assert (c["STATUS_DYN"] == 0).all() and np.all(c["XS"] == p.x0_m) and np.all(c["US"] == p.u0[0])      # the targets stay where they started
    s = enmpc.EnmpcSolver(p)
    try:
        for kernel in (1, 2):
            r = enmpc.run_enmpc_closed_loop(p, x0, 5, solver=s, kernel=kernel)
            for k in ("STATUS_DYN", "STATUS_SS", "STATUS_MHE", "ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
                if k == "ITERS_DYN" and what == "ocp":
                    # fifty iterations of a restoration phase that creeps to a minimiser of the infeasibility: its stopping test (E_0 <= tol on a problem with
                    # multipliers of 1e3) sits within rounding of its threshold for several iterations - the kernels' sweeps over the lanes and the dense factorisation
                    # leave it some iterations apart on some solves (measured with the recursion: 2 of 15, by 1 and 7; with the sweeps as parallel scans: 6 of 15, by up
                    # to 11); same verdict, same held input
                    d = np.abs(r[k].astype(int) - c[k].astype(int))
                    assert (d != 0).mean() <= 0.5 and d.max() <= 15, (kernel, k, r[k].T.tolist(), c[k].T.tolist())
                    continue
                assert np.array_equal(r[k], c[k]), (kernel, k, r[k].T.tolist(), c[k].T.tolist())
            for k in ("U", "XS", "US", "X_ES", "Xp"):
                assert np.abs(r[k] - c[k]).max() < TOL_U, (kernel, k)
    finally:
        s.close()


def test_loader_takes_user_inequality_rows(pkg):
    """User_g_ineq (Control_Calc.py:94-100,132-147; MPC_code.py:306-314): traced with y = Fy_model(x, u, d) substituted; the generated header carries values, Jacobian
    and Hessians of the rows only for a model that has them (a model without rows keeps its header and its library)"""
    from mpc_code_amd import econcodegen
    from mpc_code_amd.problem import UnsupportedProblem
    p = pkg.load_problem(EX_ROWS)
    assert len(p.g_ineq) == 2
    hdr = econcodegen.emit_econ_header(p)
    assert "struct Gin" in hdr and "MPC_EC_HAS_GIN" in hdr and "NG = 2" in hdr
    assert "Gin" not in econcodegen.emit_econ_header(pkg.load_problem(EX))
    for k in ("User_h_eq", "User_g_ineq_SS", "User_h_eq_SS"):
        with pytest.raises(UnsupportedProblem):
            pkg.load_problem(EX, overrides={k: (lambda *a: a[0])})
    o = eo.load_problem(EX_ROWS)
    assert o.g_ineq is not None and eo.g_rows(o, np.array([[0.5], [0.3]]), np.array([[1.0]]), np.zeros((2, 1))).shape == (2, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("B,nsteps", [(40, 10)])
def test_gpu_user_inequality_rows_follow_the_oracle(pkg, B, nsteps):
    """The reactor with two user rows in the OCP, one affine in input and output, one non-linear (examples/reactor_enmpc_rows.py): the reference's solver gives every
    row G_k <= 0 a slack variable, G_k - s_k = 0, s_k <= 0 [ext] - restated as such in the dense oracle (enmpc_oracle.py:ocp_eval), carried as one more stage state
    per row in the kernels (mpc_enmpc.hip:phase_ocp).  Same NLP, same algorithm: values to 1e-7 and equal iteration counts, both launch styles; the loop settles ON
    the rows (the unconstrained economic optimum violates both)."""
    from mpc_code_amd import enmpc
    over = {"N": 12, "N_mhe": 5}
    p = pkg.load_problem(EX_ROWS, overrides=over)
    q = eo.load_problem(EX_ROWS, overrides=over)
    x0 = np.random.default_rng(8).uniform([0.5, 0.0], [1.0, 0.5], size=(B, 2))
    chk = list(range(min(B, 3)))
    o = [eo.closed_loop(q, nsteps, x0_p=x0[b]) for b in chk]
    s = enmpc.EnmpcSolver(p)
    try:
        for kernel in (1, 2):
            r = enmpc.run_enmpc_closed_loop(p, x0, nsteps, solver=s, kernel=kernel)
            assert int(r["STATUS_DYN"].max()) == 0 and int(r["STATUS_SS"].max()) == 0 and int(r["STATUS_MHE"].max()) == 0
            for i, b in enumerate(chk):
                for k in ("U", "XS", "US", "X_ES", "Xp"):
                    assert np.abs(r[k][:, b] - o[i][k]).max() < TOL_U, (kernel, b, k, np.abs(r[k][:, b] - o[i][k]).max())
                for k in ("ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
                    assert np.array_equal(r[k][:, b], o[i][k]), (kernel, b, k, r[k][:, b].tolist(), o[i][k].tolist())
            # the rows hold along the closed loop (at the applied input and the state the OCP started from) and bind at the end
            g1 = r["U"][..., 0] + 0.5 * (r["X_HAT"][..., 0] + r["D_HAT"][..., 0] * 0.0) - 1.2
            assert nsteps < 8 or (r["U"][-1, :, 0] * r["X_HAT"][-1, :, 0]).max() < 0.40 + 1e-6
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_ragged_batches_and_call_order(pkg, gold):
    from mpc_code_amd import enmpc
    from mpc_code_amd.capi import MpcAmdError
    p = pkg.load_problem(EX)
    s = enmpc.EnmpcSolver(p)
    assert s.build_info().startswith("gfx950;enmpc;dims=2/1/2/2/2/4")
    s.alloc(3, 8)
    with pytest.raises(MpcAmdError):
        s.run(0, 2)                          # no state yet
    s.set_state(np.tile(gold["ship_x0"], (3, 1)))
    with pytest.raises(MpcAmdError):
        s.run(2, 2)                          # the estimator's window is sequential
    with pytest.raises(MpcAmdError):
        s.run(0, 9)                          # more steps than allocated
    s.run(0, 2); s.run(2, 3); s.sync()
    U = s.get_log("U")
    assert U.shape == (5, 3, 1) and np.abs(U[:, 0] - gold["ship_U"][:5, 0]).max() < TOL_U and np.array_equal(U[:, 0], U[:, 2])
    s.close()
    for B in (1, 65):
        x0 = np.tile(gold["ship_x0"], (B, 1))
        r = enmpc.run_enmpc_closed_loop(p, x0, 3)
        assert np.abs(r["U"][:, -1] - gold["ship_U"][:3, 0]).max() < TOL_U


@pytest.mark.gpu
@pytest.mark.parametrize("over,nsteps", [({"N": 2, "N_mhe": 2}, 8), ({"N": 3, "N_mhe": 3}, 8), ({"N": 33, "N_mhe": 17}, 22), ({"N": 64, "N_mhe": 63}, 66),
                                         ({"Sol_itmax": 4}, 6), ({"Sol_itmax": 1}, 4)])
def test_gpu_edge_horizons_and_iteration_limits_follow_the_c_restatement(pkg, over, nsteps):
    """Shortest and longest horizons a wavefront holds (one stage per lane: 2 <= N <= 64, 2 <= N_mhe <= 63), a window that crosses the
    32-lane segment, and NLPs cut off at the iteration limit (accepted like the reference accepts every status but 'infeasible',
    MPC_code.py:714,786): every launch style against the C restatement, every step, through the filling of the window."""
    import enmpc_oracle_c as ec
    from mpc_code_amd import enmpc
    x0 = np.random.default_rng(5).uniform([0.5, 0.0], [1.0, 0.5], size=(3 if nsteps > 50 else 6, 2))      # (the longest horizons: half a minute of host time per instance)
    p = pkg.load_problem(EX, overrides=over)
    c = ec.OracleEC(eo.load_problem(EX, overrides=over)).closed_loop(nsteps, x0, nthreads=6)
    s = enmpc.EnmpcSolver(p)
    for kernel in (1, 2):
        r = enmpc.run_enmpc_closed_loop(p, x0, nsteps, solver=s, kernel=kernel)
        for k in ("U", "XS", "US", "X_ES", "Xp"):
            assert np.abs(r[k] - c[k]).max() < TOL_U, (kernel, k, np.abs(r[k] - c[k]).max())
        for k in ("STATUS_DYN", "STATUS_SS", "STATUS_MHE", "ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
            assert np.array_equal(r[k], c[k]), (kernel, k, r[k].T.tolist(), c[k].T.tolist())
    if "Sol_itmax" in over:
        assert int(c["STATUS_DYN"].max()) == 1      # the cut-off shows
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3, 4] + list(range(5, 37)))
def test_gpu_randomised_reactor_models_follow_the_c_restatement(pkg, seed):
    """Other reactors than the shipped one (tests/enmpc_cases.py: round 3's tools/enmpc_fuzz.py as a test): rate constants, prices, the sampling time, both
    horizons and the estimator's update drawn at random (each model gets its own generated library: the constants are compiled in), six starts, twelve
    steps - every launch style against the C restatement evaluated with the same constants: values, status words, iteration counts of all three NLPs.
    Seeds 5 - 36 are the 32 models on which round 3's restated iteration (full steps, no safe slack) and IPOPT parted: the odd ones draw other boxes and make
    the disturbance bounds bounds of the estimator (MPC_code.py:657-664).  With the filter line search, the safe slack and - for the target - the restoration
    phase: NO status 2 on any of the 6912 solves, no solve above 60 iterations except the one documented in enmpc_cases.FUZZ_LONG_SOLVES."""
    import warnings
    import enmpc_oracle_c as ec
    from enmpc_cases import draw, FUZZ_STEPS, FUZZ_LONG_SOLVES
    from mpc_code_amd import enmpc
    over, x0 = draw(seed)
    nsteps = FUZZ_STEPS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = pkg.load_problem(EX, overrides=over)
        q = eo.load_problem(EX, overrides=over)
    c = ec.OracleEC(q).closed_loop(nsteps, x0, nthreads=0)
    assert np.isfinite(c["U"]).all()
    for k in ("STATUS_DYN", "STATUS_SS", "STATUS_MHE"):
        assert int(c[k].max()) == 0, (seed, k)
    for k in ("ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
        assert int(c[k].max()) <= (FUZZ_LONG_SOLVES[seed][1] if FUZZ_LONG_SOLVES.get(seed, ("",))[0] == k else 60), (seed, k, int(c[k].max()))
    s = enmpc.EnmpcSolver(p)
    try:
        for kernel in (1, 2):
            r = enmpc.run_enmpc_closed_loop(p, x0, nsteps, solver=s, kernel=kernel)
            # Two implementations of the same iteration take the same number of iterations except where a decision (E_0 <= tol, E_mu <= 10 mu, an acceptance
            # test of the line search) sits within rounding of its threshold: then one of them takes an iteration more towards the same point, and the two
            # points differ by what the tolerance allows - 1e-8 on the problem as IPOPT scales it, i.e. 1e-8 / df = 3e-7 in the OCP's own units (df = 0.03 on
            # the cold steps), carried through the following steps of the loop.  Where all iteration counts agree the values agree to TOL_U.
            tied = any((r[k] != c[k]).any() for k in ("ITERS_DYN", "ITERS_SS", "ITERS_MHE"))
            for k in ("U", "XS", "US", "X_ES", "Xp"):
                assert np.abs(r[k] - c[k]).max() < (2e-6 if tied else TOL_U), (over, kernel, k, tied, np.abs(r[k] - c[k]).max())
            for k in ("STATUS_DYN", "STATUS_SS", "STATUS_MHE"):
                assert np.array_equal(r[k], c[k]), (over, kernel, k)
            for k in ("ITERS_DYN", "ITERS_SS", "ITERS_MHE"):
                d = np.abs(r[k].astype(int) - c[k].astype(int))
                # (the estimator's tolerance of 1e-10 is close to what the residuals' rounding allows: its 'E_0 <= tol' falls an iteration apart in up to 6 of a model's 72 solves)
                assert (d != 0).mean() < 0.10 and d.max() <= 4, (over, kernel, k, int((d != 0).sum()), int(d.max()))
    finally:
        s.close()
