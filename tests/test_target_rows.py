"""Affine user rows of the TARGET problem on the linear path (the reference's `User_g_ineq_SS` / `User_h_eq_SS`, Target_Calc.py:87-110,139-155; MPC_code.py:295-300).

The loader reads the rows off the Ex-file's functions (problem.py:_affine_user_rows, ys = C xs + Cd dhat + fy_const substituted), the host folds the equality rows into
the null-space reduction and appends the inequality rows to W (csrc/mpc_amd.hip:build_target), the device solvers carry them (target_lane, target_row16).  The dense
statement here is built independently: oracle/mpc_oracle.py:target_qp on wss = [xs, us, ys] with the rows appended in the reference's own form - on Ys as a variable,
read off the Ex-file function by evaluating it on unit vectors - then solved by the oracle's interior point method and its active-set polish."""
import os
import re
import subprocess

import numpy as np
import pytest

import mpc_oracle as mo
from conftest import ROOT

SS_EX = "cstr_lmpc_ss_rows.py"
INC = os.path.join(ROOT, "include")


def _raw_rows(fn, p):
    """(J [rows, nx+nu+ny], Jd [rows, nd], c [rows]) of fn(x, u, y, d, t, px, py) on the reference's variables: evaluated on numbers, not traced."""
    n, m, q, nd = p.nx, p.nu, p.ny, p.nd
    nz = n + m + q + nd

    def ev(z):
        return np.atleast_1d(np.asarray(fn(z[:n], z[n:n + m], z[n + m:n + m + q], z[n + m + q:], 0.0, np.zeros(n), np.zeros(q)), dtype=float)).ravel()
    c = ev(np.zeros(nz))
    J = np.stack([ev(np.eye(nz)[j]) - c for j in range(nz)], axis=1)
    return J[:, :n + m + q], J[:, n + m + q:], c


def dense_target_qp(p, ns, usp, ysp, dhat, us_prev):
    """target_qp with the Ex-file's _SS rows appended: H_ss(wss, d) = 0 to the equalities, G_ss(wss, d) <= 0 to the bounded rows (Target_Calc.py:95-109,149-155)."""
    H, g, E, e, G, lo, hi = mo.target_qp(p, usp, ysp, np.zeros(p.nx), dhat, us_prev)
    if ns.get("User_h_eq_SS") is not None:
        J, Jd, c = _raw_rows(ns["User_h_eq_SS"], p)
        E = np.vstack([E, J]); e = np.concatenate([e, -(Jd @ dhat + c)])
    if ns.get("User_g_ineq_SS") is not None:
        J, Jd, c = _raw_rows(ns["User_g_ineq_SS"], p)
        G = np.vstack([G, J]); lo = np.concatenate([lo, np.full(len(c), -np.inf)]); hi = np.concatenate([hi, -(Jd @ dhat + c)])
    return H, g, E, e, G, lo, hi


def dense_target(p, ns, usp, ysp, dhat, us_prev):
    qp = dense_target_qp(p, ns, usp, ysp, dhat, us_prev)
    r = mo.qp_ipm_dense(*qp, tol=1e-11)
    w, exact = r["w"], False
    if r["status"] == mo.STATUS_SOLVED:
        pol = mo.qp_polish(*qp, r["w"], r["z_lo"], r["z_hi"])
        if pol is not None:
            w, exact = pol["w"], True
    n, m = p.nx, p.nu
    return dict(xs=w[:n], us=w[n:n + m], ys=w[n + m:], status=r["status"], exact=exact, qp=qp)


def row_values(p, ns, xs, us, ys, dhat):
    """(equality rows, inequality rows) at a point, on the reference's variables"""
    out = []
    for f in ("User_h_eq_SS", "User_g_ineq_SS"):
        out.append(np.zeros(0) if ns.get(f) is None else np.atleast_1d(np.asarray(ns[f](xs, us, ys, dhat, 0.0, None, None), dtype=float)).ravel())
    return out


def _ns(pkg, ex, overrides=None):
    from mpc_code_amd import exfile
    return exfile.load_exfile(pkg.example_path(ex), overrides)


def wide_rows_problem(N=20):
    """nx = 6, nu = 2, ny = 8, nd = 0 with one inequality and one equality row: NCT = 6 + 2 + 8 + 1 = 17 constraint rows of the target - more than the 16 lanes of
    target_row16, so the wave-autonomous loop takes its lane = instance fallback; and a target warm-start record (2 + 3 x 17 = 53 doubles) larger than the
    horizon-parallel loop's slot without rows (2 nu + 3 (ns + nu + 8) = 52).  The set point moves over the steps, so the inequality row binds at some of them."""
    import scipy.linalg as scla
    from mpc_code_amd.problem import LinearMPCProblem, _affine_user_rows
    rng = np.random.default_rng(2026)
    A = rng.standard_normal((6, 6)); A *= 0.9 / np.abs(np.linalg.eigvals(A)).max()
    Bm = rng.standard_normal((6, 2)) * 0.5
    C = np.vstack([np.eye(6), rng.standard_normal((2, 6)) * 0.3])
    Q = np.eye(6); R = 0.1 * np.eye(2)
    P = scla.solve_discrete_are(A, Bm, Q, R)
    inf = np.inf
    rows = {"User_h_eq_SS": lambda x, u, y, d, t, px, py: x[5] - 0.5 * u[0] + 0.1 * y[7],
            "User_g_ineq_SS": lambda x, u, y, d, t, px, py: -y[0] - 0.5 * y[6] - 0.1}
    Hx, Hu, Hd, h0 = _affine_user_rows(rows["User_h_eq_SS"], "User_h_eq_SS", 6, 2, 8, 0, C, np.zeros((8, 0)), np.zeros(8), max_rows=None)
    Gx, Gu, Gd, g0 = _affine_user_rows(rows["User_g_ineq_SS"], "User_g_ineq_SS", 6, 2, 8, 0, C, np.zeros((8, 0)), np.zeros(8))
    ysp0 = rng.standard_normal(8) * 0.5

    def defSP(t):
        return [ysp0 * (0.2 + 0.3 * (int(t) % 5)), np.zeros(2), np.zeros(6)]
    p = LinearMPCProblem(nx=6, nu=2, ny=8, nd=0, nxp=6, N=N, h=1.0, Nsim=20, A=A, B=Bm, C=C, Bd=np.zeros((6, 0)), Cd=np.zeros((8, 0)),
                         fx_const=np.zeros(6), fy_const=np.zeros(8), Ap=A, Bp=Bm, Cp=C, Q=Q, R=R, DUForm=False, P=P,
                         Qss=np.eye(8), Rss=np.zeros((2, 2)), DUssForm=False, umin=-np.ones(2), umax=np.ones(2),
                         xmin=np.full(6, -inf), xmax=np.full(6, inf), ymin=np.full(8, -inf), ymax=np.full(8, inf), y_bounded=False,
                         umin_ss=-2.0 * np.ones(2), umax_ss=2.0 * np.ones(2), xmin_ss=np.full(6, -inf), xmax_ss=np.full(6, inf),
                         ymin_ss=np.full(8, -inf), ymax_ss=np.full(8, inf), estimator="none",
                         x0_p=np.zeros(6), x0_m=np.zeros(6), u0=np.zeros(2), dhat0=np.zeros(0), defSP=defSP,
                         Gx_ss=Gx, Gu_ss=Gu, Gd_ss=Gd, g0_ss=g0, Hx_ss=Hx, Hu_ss=Hu, Hd_ss=Hd, h0_ss=h0)
    return p, rows


@pytest.fixture(scope="module")
def ss(pkg):
    return pkg.load_problem(pkg.example_path(SS_EX))


@pytest.fixture(scope="module")
def ss_ns(pkg):
    return _ns(pkg, SS_EX)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_loader_reads_the_target_rows(ss):
    """y_2 - 0.02 u_0 + 0.01 d_0 = 0 and y_0 + 0.02 u_0 - 0.2 <= 0, with y = C x (C = I, Cd = 0, fy_const = 0 in the CSTR) substituted"""
    assert ss.n_ss_eq_rows == 1 and ss.n_ss_ineq_rows == 1
    assert np.allclose(ss.Hx_ss, [[0.0, 0.0, 1.0]]) and np.allclose(ss.Hu_ss, [[-0.02, 0.0]]) and np.allclose(ss.Hd_ss, [[0.01, 0.0, 0.0]]) and np.allclose(ss.h0_ss, [0.0])
    assert np.allclose(ss.Gx_ss, [[1.0, 0.0, 0.0]]) and np.allclose(ss.Gu_ss, [[0.02, 0.0]]) and np.allclose(ss.Gd_ss, [[0.0, 0.0, 0.0]]) and np.allclose(ss.g0_ss, [-0.2])
    assert ss.n_user_rows == 0      # (the OCP does not see them)


def test_loader_substitutes_the_output_model(pkg):
    """a row on y with Cd and fy_const non-zero: y = C x + Cd d + fy_const"""
    base = pkg.example_path("cstr_lmpc.py")
    Cd = np.array([[0.5, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    p = pkg.load_problem(base, overrides={"Cd": Cd, "ylin": np.array([0.3, 0.0, 0.0]),
                                          "User_g_ineq_SS": lambda x, u, y, d, t, px, py: 2.0 * y[0] - u[1] + 0.25 * d[2] - 1.0})
    assert np.allclose(p.Gx_ss, 2.0 * p.C[0:1]) and np.allclose(p.Gu_ss, [[0.0, -1.0]])
    assert np.allclose(p.Gd_ss, [[1.0, 0.0, 0.25]]) and np.allclose(p.g0_ss, [2.0 * p.fy_const[0] - 1.0])


@pytest.mark.parametrize("over, match", [
    ({"User_g_ineq_SS": lambda x, u, y, d, t, px, py: u[0] * x[0] - 1.0}, "User_g_ineq_SS: only rows that are affine"),
    ({"User_h_eq_SS": lambda x, u, y, d, t, px, py: u[0] + t - 1.0}, "User_h_eq_SS: only rows that are affine"),
    ({"User_g_ineq_SS": lambda x, u, y, d, t, px, py: [u[0] - 1.0, u[1] - 1.0, x[0], x[1], x[2]]}, "User_g_ineq_SS: between one and 4 rows"),
    ({"User_h_eq_SS": lambda x, u, y, d, t, px, py: [u[0] - 1.0, x[0]]}, "nh < nu"),
    ({"User_h_eq_SS": lambda x, u, y, d, t, px, py: 0.0659 * u[1] - 0.3}, "linearly dependent"),      # a multiple of [A-I, B]'s third row (u_1 alone)
    ({"def_px": lambda t: [np.zeros(3)]}, "def_px / def_py"),
    ({"def_py": lambda t: [np.zeros(3)]}, "def_px / def_py"),
])
def test_loader_refuses_loudly(pkg, over, match):
    from mpc_code_amd.problem import UnsupportedProblem
    with pytest.raises(UnsupportedProblem, match=match):
        pkg.load_problem(pkg.example_path(SS_EX), overrides=over)


def test_loader_carries_the_rows_with_features_that_do_not_touch_the_target(pkg):
    for ex, over in (("cstr_lmpc_rows.py", {}), ("cstr_lmpc_soft.py", {}), ("cstr_lmpc.py", {"TermCons": True}), ("cstr_lmpc.py", {"Dumin": -np.ones(2), "Dumax": np.ones(2)})):
        ns = _ns(pkg, SS_EX)
        p = pkg.load_problem(pkg.example_path(ex), overrides=dict(over, User_g_ineq_SS=ns["User_g_ineq_SS"], User_h_eq_SS=ns["User_h_eq_SS"]))
        assert p.n_ss_ineq_rows == 1 and p.n_ss_eq_rows == 1, ex


def test_nonlinear_and_economic_loaders_keep_refusing(pkg):
    from mpc_code_amd.problem import UnsupportedProblem
    row = lambda x, u, y, d, t, px, py: u[0] - 1.0
    for ex in ("cstr_nmpc.py", "reactor_enmpc.py"):
        for f in ("User_g_ineq_SS", "User_h_eq_SS"):
            with pytest.raises(UnsupportedProblem):
                pkg.load_problem(pkg.example_path(ex), overrides={f: row})


def test_dense_statement_holds_the_rows(pkg, ss, ss_ns):
    """at the optimum of the dense statement the equality row holds, the inequality row is active, and the target differs from the one without rows"""
    plain = pkg.load_problem(pkg.example_path("cstr_lmpc.py"))
    dhat = np.array([0.1752, -1.0389, 0.0])      # (the shipped scenario from its fourth step on)
    for ysp in (np.array([0.2, 0.0, 0.0]), np.array([0.0, 0.0, 0.1])):      # before and after the set-point change
        t = dense_target(ss, ss_ns, np.zeros(2), ysp, dhat, np.zeros(2))
        t0 = mo.target_solve_exact(plain, np.zeros(2), ysp, np.zeros(3), dhat, np.zeros(2))
        assert t["status"] == 0 and t["exact"] and t0["status"] == 0
        h, g = row_values(ss, ss_ns, t["xs"], t["us"], t["ys"], dhat)
        assert np.abs(h).max() < 1e-10 and np.abs(g).max() < 1e-10, (h, g)      # (g active: zero)
        assert np.abs(t["xs"] - t0["xs"]).max() > 1e-2


def test_ctypes_descriptor_matches_the_header(tmp_path):
    """a C host that fills the new fields: field offsets and the size of mpc_lin_desc are those of capi's ctypes structure"""
    from mpc_code_amd import capi
    import ctypes as ct
    fields = ("n_user_rows", "g0", "n_ss_ineq_rows", "Gx_ss", "Gu_ss", "Gd_ss", "g0_ss", "n_ss_eq_rows", "Hx_ss", "Hu_ss", "Hd_ss", "h0_ss")
    src = tmp_path / "desc.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"mpc_amd.h\"\n"
                   "int main(void) {\n"
                   "    static const double G[3] = {1.0, 0.0, 0.0}, H[2] = {-0.02, 0.0}, z = 0.0;\n"
                   "    mpc_lin_desc d = {0};\n"
                   "    d.n_ss_ineq_rows = 1; d.Gx_ss = G; d.Gu_ss = H; d.Gd_ss = G; d.g0_ss = &z;\n"
                   "    d.n_ss_eq_rows = 1; d.Hx_ss = G; d.Hu_ss = H; d.Hd_ss = G; d.h0_ss = &z;\n"
                   "    printf(\"size %zu\\n\", sizeof(mpc_lin_desc));\n"
                   + "".join(f"    printf(\"{f} %zu\\n\", offsetof(mpc_lin_desc, {f}));\n" for f in fields)
                   + "    return d.n_ss_ineq_rows + d.n_ss_eq_rows == 2 ? 0 : 1;\n}\n")
    exe = str(tmp_path / "desc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, str(src), "-o", exe])
    out = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == ct.sizeof(capi._Desc)
    for f in fields:
        assert int(out[f]) == getattr(capi._Desc, f).offset, f
    hdr = open(os.path.join(INC, "mpc_amd.h")).read()
    assert re.search(r"int32_t n_ss_eq_rows;\s*const double \*Hx_ss, \*Hu_ss, \*Hd_ss, \*h0_ss;\s*\} mpc_lin_desc;", hdr)      # appended at the end


def test_dimension_sets_at_the_edges_compile():
    """sets whose target warm-start record outgrows the horizon-parallel loop's slot without rows (ny = 8 with one inequality row, ny = 5 with four), and the set of
    wide_rows_problem: every kernel of the library instantiates (the static_asserts on the LDS slots included)"""
    csrc = os.path.join(ROOT, "mpc-code_amd", "csrc")
    sets = "X(2,2,8,2,2,0,0,1,0) X(2,2,5,2,2,0,0,4,0) X(6,2,8,0,6,0,0,1,1) X(4,2,8,2,4,1,0,4,1)"
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", f"-DMPC_DIM_LIST(X)={sets}", "mpc_amd.hip"],
                       cwd=csrc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def test_dimension_sets_without_rows_keep_their_library_names(pkg):
    from mpc_code_amd import capi
    assert capi.jit_library_path((3, 2, 3, 3, 3, 1, 0, 0, 0)) == capi.jit_library_path((3, 2, 3, 3, 3, 1, 0))
    assert capi.jit_library_path((3, 2, 3, 3, 3, 0, 0, 1, 1)).endswith("libmpc_amd_3_2_3_3_3_0_0_1_1.so")


# ------------------------------------------------------------------------------------------------------------------ GPU
def _close(a, b, tol):
    """|a - b| <= tol, relative to the entry's size beyond one (the CSTR's second state sits near its bound 10)"""
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


def _draw(rng, B):
    dhat = np.array([0.1752, -1.0389, 0.0]) + rng.uniform(-1.0, 1.0, size=(B, 3)) * np.array([0.3, 1.0, 0.002])
    ysp = np.where(rng.uniform(size=(B, 1)) < 0.5, [0.2, 0.0, 0.0], [0.0, 0.0, 0.1]) + 0.05 * rng.normal(size=(B, 3))
    usp = rng.normal(size=(B, 2))
    return dhat, ysp, usp


@pytest.mark.gpu
def test_gpu_target_solve_matches_the_dense_statement(ss, ss_ns):
    from mpc_code_amd import capi
    rng = np.random.default_rng(20261015)
    B = 64
    dhat, ysp, usp = _draw(rng, B)
    up = rng.normal(size=(B, 2))
    s = capi.Solver(ss)
    try:
        r = s.target_solve(usp, ysp, np.zeros((B, 3)), dhat, up)
    finally:
        s.close()
    n_exact = n_active = n_inf = 0
    for b in range(B):
        t = dense_target(ss, ss_ns, usp[b], ysp[b], dhat[b], up[b])
        assert r["status"][b] == t["status"], (b, r["status"][b], t["status"])
        if t["status"] != 0:
            n_inf += 1
            continue
        h, g = row_values(ss, ss_ns, r["xs"][b], r["us"][b], r["ys"][b], dhat[b])
        assert np.abs(h).max() < 1e-9 and g.max() < 1e-9, (b, h, g)
        if t["exact"]:
            n_exact += 1
            assert _close(r["xs"][b], t["xs"], 1e-7) and _close(r["us"][b], t["us"], 1e-7), (b, r["xs"][b] - t["xs"], r["us"][b] - t["us"])
            n_active += int(abs(row_values(ss, ss_ns, t["xs"], t["us"], t["ys"], dhat[b])[1][0]) < 1e-9)
    assert n_exact >= 30 and n_active >= 4 and n_exact - n_active >= 4 and n_inf >= 4, (n_exact, n_active, n_inf)      # (the draw: 35 / 6 / 29)


def _check_loop(p, ns, r, x0, u0, tag):
    """every logged target against the dense statement at the logged DHAT (and the previous US): status, and the new target or the kept one (before the
    first step: the loop's initial target xs = xhat, us = u, MPC_code.py:682-684)"""
    ST, XS, US = r["STATUS_SS"], r["XS"], r["US"]
    DH = r["D_HAT"] if p.nd else np.zeros(ST.shape + (0,))
    nsteps, B = ST.shape
    counts = dict(solved=0, infeasible=0, active=0)
    for b in range(0, B, 8):
        us_prev = np.asarray(u0[b], dtype=float)
        xs_prev = np.asarray(x0[b], dtype=float)
        for k in range(nsteps):
            t = dense_target(p, ns, p.schedules(nsteps)["usp"][k], p.schedules(nsteps)["ysp"][k], DH[k, b], us_prev)
            assert ST[k, b] == t["status"], (tag, b, k, ST[k, b], t["status"])
            if t["status"] == 2:
                counts["infeasible"] += 1
                assert np.array_equal(XS[k, b], xs_prev) and np.array_equal(US[k, b], us_prev), (tag, b, k)      # the previous target is kept
            else:
                counts["solved"] += 1
                tol = 1e-6 if t["exact"] else 1e-5      # (a warm-started solve of the loop may stop at its relaxed stationarity test, mpc_device.hpp:kTolStatAcc)
                assert _close(XS[k, b], t["xs"], tol) and _close(US[k, b], t["us"], tol), (tag, b, k, XS[k, b] - t["xs"], US[k, b] - t["us"])
                counts["active"] += int(abs(row_values(p, ns, t["xs"], t["us"], t["ys"], DH[k, b])[1]).min() < 1e-9)
            xs_prev, us_prev = XS[k, b], US[k, b]
    return counts


def _loop_x0(B, seed):
    rng = np.random.default_rng(seed)
    x0 = np.array([3.0, 3.0, 3.0]) + rng.uniform(-1.0, 1.0, size=(B, 3)) * np.array([0.5, 2.0, 1.0])
    return x0


@pytest.mark.gpu
@pytest.mark.parametrize("lk", [1, 2, 3])
def test_gpu_resident_loop_follows_the_dense_target(ss, ss_ns, lk):
    """256 instances x 30 steps across the set-point change (t = 15) and the plant disturbance change (t = 20) on the lane, horizon-parallel and wave-autonomous loops"""
    from mpc_code_amd import capi, driver
    x0 = _loop_x0(256, 7)
    s = capi.Solver(ss)
    try:
        s.set_option("loop_kernel", lk)
        r = driver.run_closed_loop(ss, x0, x0, 30, solver=s)
    finally:
        s.close()
    c = _check_loop(ss, ss_ns, r, x0, np.broadcast_to(ss.u0, (256, 2)), lk)
    assert c["solved"] > 0 and c["infeasible"] > 0 and c["active"] > 0, c


@pytest.mark.gpu
def test_gpu_soft_loop_follows_the_dense_target(pkg, ss_ns):
    """the same rows on the problem with soft output constraints (loop_kernel_soft)"""
    from mpc_code_amd import capi, driver
    p = pkg.load_problem(pkg.example_path("cstr_lmpc_soft.py"), overrides={k: ss_ns[k] for k in ("User_g_ineq_SS", "User_h_eq_SS")})
    ns = _ns(pkg, "cstr_lmpc_soft.py", {k: ss_ns[k] for k in ("User_g_ineq_SS", "User_h_eq_SS")})
    x0 = _loop_x0(256, 8)
    s = capi.Solver(p)
    try:
        r = driver.run_closed_loop(p, x0, x0, 30, solver=s)
    finally:
        s.close()
    c = _check_loop(p, ns, r, x0, np.broadcast_to(p.u0, (256, 2)), "soft")
    assert c["solved"] > 0 and c["active"] > 0, c


@pytest.mark.gpu
@pytest.mark.parametrize("lk", [1, 3])
def test_gpu_hold_rule_where_the_rows_leave_no_target(pkg, ss_ns, lk):
    """x_0 >= 5 d_0 - 1 together with the example's equality row: no steady state where the disturbance estimate d_0 is beyond about 0.32.  Initial estimates drawn
    on both sides: status 2 for part of the batch over the first steps (until the estimator has the plant's 0.175), and the previous target is kept there"""
    from mpc_code_amd import capi
    over = {"User_h_eq_SS": ss_ns["User_h_eq_SS"], "User_g_ineq_SS": lambda x, u, y, d, t, px, py: -x[0] + 5.0 * d[0] - 1.0}
    p = pkg.load_problem(pkg.example_path("cstr_lmpc.py"), overrides=over)
    ns = _ns(pkg, "cstr_lmpc.py", over)
    B, nsteps = 256, 12
    rng = np.random.default_rng(9)
    x0 = _loop_x0(B, 10)
    dh0 = np.column_stack([rng.uniform(0.2, 0.45, B), np.zeros(B), np.zeros(B)])
    s = capi.Solver(p)
    try:
        s.set_option("loop_kernel", lk)
        s.loop_alloc(B, nsteps, capi.LOG_ALL)
        s.loop_set_state(x0, x0, dhat=dh0)
        s.loop_set_schedule(p.schedules(nsteps))
        s.loop_run(0, nsteps)
        s.loop_sync()
        r = {k: s.loop_get_log(k) for k in ("STATUS_SS", "XS", "US", "D_HAT")}
    finally:
        s.close()
    c = _check_loop(p, ns, r, x0, np.broadcast_to(p.u0, (B, 2)), ("hold", lk))
    inf_inst = (r["STATUS_SS"] == 2).any(axis=0)
    assert c["infeasible"] > 0 and c["solved"] > 0 and 0.1 < inf_inst.mean() < 0.9, (c, inf_inst.mean())


@pytest.mark.gpu
def test_gpu_ocp_rows_and_target_rows_together_on_the_wave_kernel(pkg, ss_ns):
    """cstr_lmpc_rows.py (User_g_ineq in the OCP) with the _SS rows: wave-autonomous loop, targets against the dense statement"""
    from mpc_code_amd import capi, driver
    over = {k: ss_ns[k] for k in ("User_g_ineq_SS", "User_h_eq_SS")}
    p = pkg.load_problem(pkg.example_path("cstr_lmpc_rows.py"), overrides=over)
    ns = _ns(pkg, "cstr_lmpc_rows.py", over)
    assert p.n_user_rows == 2
    x0 = _loop_x0(256, 11)
    s = capi.Solver(p)
    try:
        s.set_option("loop_kernel", 3)
        r = driver.run_closed_loop(p, x0, x0, 30, solver=s)
    finally:
        s.close()
    c = _check_loop(p, ns, r, x0, np.broadcast_to(p.u0, (256, 2)), "ocp+ss")
    assert c["solved"] > 0 and c["active"] > 0, c
    U = r["U"]
    assert (U[..., 0] + 0.5 * U[..., 1] - 5.0)[r["STATUS_DYN"] != 2].max() < 1e-6      # (the OCP's first row)


@pytest.mark.gpu
@pytest.mark.parametrize("lk", [1, 2, 3])
def test_gpu_wide_target_rows_on_every_loop(lk):
    """wide_rows_problem: the wave-autonomous loop on its lane fallback (17 target rows > 16 lanes) and the horizon-parallel loop with the larger warm-start record,
    every step's target against the dense statement"""
    from mpc_code_amd import capi, driver
    p, ns = wide_rows_problem()
    x0 = np.random.default_rng(12).uniform(-0.5, 0.5, size=(128, 6))
    s = capi.Solver(p)
    try:
        s.set_option("loop_kernel", lk)
        assert s.get_option("loop_kernel") == lk
        r = driver.run_closed_loop(p, x0, x0, 12, solver=s)
    finally:
        s.close()
    c = _check_loop(p, ns, r, x0, np.zeros((128, 2)), ("wide", lk))
    assert c["solved"] > 0 and c["active"] > 0 and c["solved"] > c["active"], c

