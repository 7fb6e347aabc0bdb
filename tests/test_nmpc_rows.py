"""User inequality rows on the non-linear tracking path (the reference's ``User_g_ineq(x, u, y, d, t, px, py) <= 0`` at every stage of the horizon,
Control_Calc.py:94-100,132-147; MPC_code.py:306-314): loader, generated header, library - and on the GPU the per-call OCP, the
closed loops of the three kernels and the hold rule, against the test-side restatement of tests/nmpc_rows_ref.py (oracle/nmpc_oracle.py's functions
with the rows appended to its dense QPs; Jacobians of the rows by central differences).
"""
import ctypes as ct
import hashlib
import os
import warnings

import numpy as np
import pytest

from conftest import ROOT

import nmpc_rows_ref as rr

EX = "cstr_nmpc_rows.py"
# sha256 of emit_model_header for the models without rows, as the parent commit emits them: their libraries stay what they were
PLAIN_HEADER_SHA = {
    "cstr_nmpc.py": "06a3100348c175cc2dd43f12f4355a2c1dcc038927524396f8a51ab60809a872",
    "quadtank_nmpc_dis.py": "71fbbd413eeb47c2603f56fc8fb58ea104088fcb5f92b410f1b6adfe1cc8e281",
    "reactor_nmpc.py": "23f061ec28c09b862c0b1ade61e108a40df1a183335fcc5899515a876ac0002d",
}


def two_rows(x, u, y, d, t, px, py):
    """the example's row and a second one on the reactor temperature: stage state 3 + 2 = 5, beyond the wave-style kernels"""
    return [u[1] * x[0] - 0.87 * d[1], x[1] - 340.0]


def _load(pkg, ex=EX, overrides=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return pkg.load_problem(pkg.example_path(ex), overrides)


def _ref(overrides=None):
    return rr.load(os.path.join(ROOT, "mpc-code_amd", "examples", EX), overrides)


@pytest.fixture(scope="module")
def nr(pkg):
    return _load(pkg)


@pytest.fixture(scope="module")
def orr():
    return _ref()


# ------------------------------------------------------------------------------------------------- loader, header, library (CPU)
def test_loader_carries_the_rows(nr):
    from mpc_code_amd.nlproblem import NonlinearMPCProblem
    assert isinstance(nr, NonlinearMPCProblem)
    assert nr.ng == 1 and (nr.nx, nr.nu, nr.ny, nr.nd) == (3, 2, 2, 2)


def test_traced_rows_and_jacobians_equal_the_user_function(nr, orr):
    from mpc_code_amd import symtrace as st
    rng = np.random.default_rng(11)
    for _ in range(8):
        x = nr.x0_m * (1.0 + 0.05 * rng.uniform(-1, 1, 3)); u = nr.u0 * (1.0 + 0.05 * rng.uniform(-1, 1, 2)); d = nr.dhat0 + 0.02 * rng.uniform(-1, 1, 2)
        t = float(rng.uniform(0, 10))
        v = nr._vals(x=x, u=u, d=d, t=t)
        g = np.array([float(a) for a in st.evaluate(nr.g_ineq, v)])
        assert np.allclose(g, rr.rows(orr, x, u, d, t), rtol=1e-14, atol=1e-14)
        Gx = np.array([[float(st.evaluate([e], v)[0]) for e in row] for row in nr.g_x])
        Gu = np.array([[float(st.evaluate([e], v)[0]) for e in row] for row in nr.g_u])
        Fx, Fu, _ = rr.rows_jac(orr, x, u, d, t)
        assert np.allclose(Gx, Fx, rtol=1e-7, atol=1e-7) and np.allclose(Gu, Fu, rtol=1e-7, atol=1e-7)


def test_rows_see_the_output_map(pkg):
    """y is Fy_model(x, u, d, t) (Control_Calc.py:130)."""
    from mpc_code_amd import symtrace as st
    p = _load(pkg, "cstr_nmpc.py", {"User_g_ineq": lambda x, u, y, d, t, px, py: y[1] * u[1] - 0.05})
    assert p.ng == 1
    x = p.x0_m * 1.01; u = p.u0; d = p.dhat0
    g = float(st.evaluate(p.g_ineq, p._vals(x=x, u=u, d=d, t=0.0))[0])
    assert np.isclose(g, p.model_output(x, u, d, 0.0)[1] * u[1] - 0.05, rtol=1e-14)


@pytest.mark.parametrize("over,match", [
    ({"User_g_ineq": lambda x, u, y, d, t, px, py: x[0:0]}, "between one and four"),
    ({"User_g_ineq": lambda x, u, y, d, t, px, py: x[0] * u[0] * np.ones(5)}, "between one and four|cannot be traced|wrong"),
    ({"User_g_ineq": lambda x, u, y, d, t, px, py: float(x[0]) - 1.0}, "cannot be traced"),
    ({"S": 0.1 * np.eye(2), "R": None, "User_g_ineq": lambda x, u, y, d, t, px, py: u[0] * x[0] * np.ones(4)}, "exceeds 8|cannot be traced"),
    ({"User_h_eq": lambda x, u, y, d, t, px, py: u[0] - 1.0}, "User_h_eq"),
    ({"User_g_ineq_SS": lambda x, u, y, d, t, px, py: u[0] - 1.0}, "User_g_ineq_SS"),
    ({"User_h_eq_SS": lambda x, u, y, d, t, px, py: u[0] - 1.0}, "User_h_eq_SS"),
    ({"slacks": True}, "slacks"),
    ({"TermCons": True}, "TermCons"),
    ({"def_px": lambda t: [np.zeros(3)]}, "def_px"),
    ({"def_py": lambda t: [np.zeros(2)]}, "def_py"),
])
def test_loader_refuses_loudly(pkg, over, match):
    from mpc_code_amd.problem import UnsupportedProblem
    with pytest.raises(UnsupportedProblem, match=match):
        _load(pkg, EX, over)


def test_row_counts_at_the_limits(pkg):
    from mpc_code_amd.problem import UnsupportedProblem
    four = lambda x, u, y, d, t, px, py: [u[1] * x[0] - 1, x[1] - 400, x[2] - 1, u[0] * u[1] - 100]
    assert _load(pkg, EX, {"User_g_ineq": four}).ng == 4
    five = lambda x, u, y, d, t, px, py: [u[1] * x[0] - 1, x[1] - 400, x[2] - 1, u[0] * u[1] - 100, x[0] - 2]
    with pytest.raises(UnsupportedProblem, match="between one and four"):
        _load(pkg, EX, {"User_g_ineq": five})
    with pytest.raises(UnsupportedProblem, match="exceeds 8"):      # input-move form: 3 + 2 + 4 = 9
        _load(pkg, EX, {"User_g_ineq": four, "Dumax": np.array([1.0, 0.05]), "Dumin": np.array([-1.0, -0.05])})
    assert _load(pkg, EX, {"User_g_ineq": two_rows, "Dumax": np.array([1.0, 0.05]), "Dumin": np.array([-1.0, -0.05])}).ng == 2


def test_wave_fit_counts_the_rows(pkg, nr):
    from mpc_code_amd import nlcodegen
    text = nlcodegen.emit_model_header(nr)
    assert "#define MPC_NL_WAVE_FITS 1" in text and "static constexpr int NG = 1;" in text
    for fn in ("g(", "g_jac("):
        assert "void " + fn in text
    assert "#define MPC_NL_WAVE_FITS 0" in nlcodegen.emit_model_header(_load(pkg, EX, {"User_g_ineq": two_rows}))


@pytest.mark.parametrize("ex", sorted(PLAIN_HEADER_SHA))
def test_headers_without_rows_are_unchanged(pkg, ex):
    from mpc_code_amd import nlcodegen
    text = nlcodegen.emit_model_header(_load(pkg, ex))
    assert "NG" not in text and "g_jac" not in text
    assert hashlib.sha256(text.encode()).hexdigest() == PLAIN_HEADER_SHA[ex]


@pytest.fixture(scope="module")
def rows_lib(nr):
    from mpc_code_amd import nlcodegen
    return nlcodegen.build_nmpc_library(nr)


def test_row_library_builds_and_exports_the_header(rows_lib):
    import re
    from mpc_code_amd import nmpc
    hdr = open(os.path.join(ROOT, "include", "mpc_nmpc.h")).read()
    declared = set(re.findall(r"\b(nmpc_[a-z_]+)\s*\(", hdr))
    lib = ct.CDLL(rows_lib)
    for s in declared | set(nmpc.NMPC_EXPORTS):
        assert hasattr(lib, s), s
    lib.nmpc_build_info.restype = ct.c_char_p
    info = lib.nmpc_build_info().decode()
    assert info.startswith("gfx950;nmpc;dims=3/2/2/2/3;mx=10") and info.endswith(";ng=1")


def test_restatement_kkt_point_holds_an_active_row(orr):
    """The restatement's converged SQP point is a KKT point of the NLP with the rows; a row is active there, and the point is not the
    optimum without rows."""
    p = orr
    xh, u, d = p.x0_m.copy(), p.u0.copy(), p.dhat0.copy()
    w0 = np.concatenate([np.tile(np.concatenate([xh, u]), p.N), xh])
    r = rr.ocp_solve(p, xh, xh, u, d, w0, max_sqp=50, tol=1e-10, u_prev=u)
    assert r["status"] == rr.STATUS_SOLVED
    c = rr.kkt_rows(p, r["w"], xh, xh, u, d, u_prev=u)
    assert c["defect"] < 1e-9 and c["bound_violation"] < 1e-9
    assert c["stationarity"] <= 1e-8, c
    assert c["row_max"] <= 1e-10, c
    assert c["n_rows_active"] >= 1
    q = rr.ocp_solve_plain(p, xh, xh, u, d, w0, max_sqp=50, tol=1e-10, u_prev=u)
    assert np.abs(q["u0"] - r["u0"]).max() > 1e-3
    assert rr.row_values(p, q["w"], d).max() > 1e-4      # the optimum without rows violates them


# ------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def rsolver(nr):
    from mpc_code_amd import nmpc
    s = nmpc.NmpcSolver(nr)
    yield s
    s.close()


def _percall(s, p, xh, d, xs, us, up, max_sqp=50):
    """nmpc_ocp_solve from the first guess (xh, u_prev) in every stage: the estimator call before it leaves xh as the model state of the step."""
    B = xh.shape[0]
    s.alloc(B, 1); s.set_state(xh, xh)
    ne = p.nx + p.nd
    s.ekf_update(p.model_output(xh, up, d, 0.0), up, xh, d, np.tile(np.eye(ne).ravel(), (B, 1)))
    return s.ocp_solve(xh, d, xs, us, up, max_sqp=max_sqp, sqp_tol=1e-9)


def _ref_percall(p, xh, d, xs, us, up):
    w0 = np.concatenate([np.tile(np.concatenate([xh, up]), p.N), xh])
    return rr.ocp_solve(p, xh, xs, us, d, w0, max_sqp=50, tol=1e-9, u_prev=up)


@pytest.mark.gpu
def test_gpu_per_call_ocp_equals_the_restatement(nr, orr, rsolver):
    B = 24
    rng = np.random.default_rng(5)
    xh = nr.x0_m * (1.0 + 0.02 * rng.uniform(-1, 1, size=(B, 3)))
    up = nr.u0 * (1.0 + 0.02 * rng.uniform(-1, 1, size=(B, 2)))
    d = nr.dhat0 + 0.005 * rng.uniform(-1, 1, size=(B, 2))
    xs = np.tile(nr.x0_m, (B, 1)); us = np.tile(nr.u0, (B, 1))
    u, x1, st, it, sq = _percall(rsolver, nr, xh, d, xs, us, up)
    active = 0
    for b in range(B):
        o = _ref_percall(orr, xh[b], d[b], xs[b], us[b], up[b])
        assert st[b] == o["status"], (b, st[b], o["status"])
        if o["status"] == rr.STATUS_INFEASIBLE:
            continue
        assert np.max(np.abs(u[b] - o["u0"]) / (1 + np.abs(o["u0"]))) < 1e-6, b
        assert np.max(np.abs(x1[b] - o["x1"]) / (1 + np.abs(o["x1"]))) < 1e-6, b
        g0 = rr.rows(orr, xh[b], u[b], d[b])
        assert g0.max() <= 1e-8, (b, g0)
        assert rr.row_values(orr, o["w"], d[b]).max() <= 1e-8
        active += int(np.abs(g0).min() < 1e-7)
    assert active >= 1 and (st == 0).sum() >= B // 2


LOOPS = {"rti": (1, 40), "sqp": (50, 8)}


@pytest.fixture(scope="module")
def loop_starts(nr):
    rng = np.random.default_rng(2)
    return np.vstack([nr.x0_p, nr.x0_p * (1.0 + 0.01 * rng.uniform(-1, 1, 3))])


@pytest.fixture(scope="module")
def ref_loops(orr, loop_starts):
    return {mode: [rr.closed_loop(orr, ns, x0_p=x, x0_m=x, max_sqp=ms) for x in loop_starts] for mode, (ms, ns) in LOOPS.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [1, 3, 4])
@pytest.mark.parametrize("mode", ["rti", "sqp"])
def test_gpu_closed_loop_equals_the_restatement(nr, rsolver, loop_starts, ref_loops, mode, kernel):
    from mpc_code_amd import nmpc
    ms, ns = LOOPS[mode]
    rsolver.set_kernel(kernel)
    assert rsolver.get_kernel() == kernel
    r = nmpc.run_nmpc_closed_loop(nr, loop_starts, loop_starts, nsteps=ns, solver=rsolver, max_sqp=ms, sqp_tol=1e-9)
    rsolver.set_kernel(0)
    for b, o in enumerate(ref_loops[mode]):
        assert np.array_equal(r["STATUS_DYN"][:, b], o["STATUS_DYN"]) and np.array_equal(r["STATUS_SS"][:, b], o["STATUS_SS"]), b
        for k in ("U", "X_HAT", "XS", "US", "Xp", "D_HAT"):
            assert np.max(np.abs(r[k][:, b] - o[k]) / (1.0 + np.abs(o[k]))) < 2e-7, (b, k)
        assert (np.abs(o["ROW0"]) < 1e-7).sum() >= ns // 4      # the row binds along the loop
        assert np.nanmax(o["ROW0"]) <= 1e-8


@pytest.mark.gpu
def test_gpu_two_rows_take_the_lane_kernel(pkg):
    from mpc_code_amd import nmpc
    from mpc_code_amd.capi import MpcAmdError
    p = _load(pkg, EX, {"User_g_ineq": two_rows})
    o = rr.closed_loop(_ref({"User_g_ineq": two_rows}), 20, max_sqp=1)
    s = nmpc.NmpcSolver(p)
    try:
        s.alloc(4, 20)
        assert s.get_kernel() == 1
        for k in (3, 4):
            with pytest.raises(MpcAmdError, match="wave-autonomous"):
                s.set_kernel(k)
        r = nmpc.run_nmpc_closed_loop(p, p.x0_p[None], p.x0_m[None], nsteps=20, solver=s, max_sqp=1)
    finally:
        s.close()
    assert np.array_equal(r["STATUS_DYN"][:, 0], o["STATUS_DYN"])
    for k in ("U", "X_HAT", "XS", "US", "Xp", "D_HAT"):
        assert np.max(np.abs(r[k][:, 0] - o[k]) / (1.0 + np.abs(o[k]))) < 2e-7, k


@pytest.mark.gpu
def test_gpu_infeasible_stage0_row_holds_the_input(pkg):
    """A row on the estimate alone that the estimate violates: the stage-0 row cannot hold whatever u_0 is - status 2, the previous input held and
    the model propagated (MPC_code.py:804-805); next to it instances that satisfy it."""
    over = {"User_g_ineq": lambda x, u, y, d, t, px, py: [x[0] - 0.86]}
    p, o = _load(pkg, EX, over), _ref(over)
    from mpc_code_amd import nmpc
    s = nmpc.NmpcSolver(p)
    try:
        xh = np.array([p.x0_m, p.x0_m * [0.97, 1.0, 1.0], p.x0_m * [1.01, 1.0, 1.0], p.x0_m * [0.96, 1.0, 1.0]])
        B = xh.shape[0]
        d, up = np.tile(p.dhat0, (B, 1)), np.tile(p.u0, (B, 1))
        xs, us = xh.copy(), up.copy()
        u, x1, st, it, sq = _percall(s, p, xh, d, xs, us, up)
    finally:
        s.close()
    assert st[0] == 2 and st[2] == 2 and (st[1] != 2 or st[3] != 2)
    for b in range(B):
        r = _ref_percall(o, xh[b], d[b], xs[b], us[b], up[b])
        assert (st[b] == 2) == (r["status"] == 2), (b, st[b], r["status"])      # (the restatement may stop at its SQP limit where the device converged)
        if st[b] == 2:
            assert np.array_equal(u[b], up[b])
            assert np.max(np.abs(x1[b] - rr.no.model_fx(o, xh[b], up[b], d[b], 0.0)) / (1 + np.abs(x1[b]))) < 1e-9
        elif st[b] == 0 and r["status"] == 0:
            assert np.max(np.abs(u[b] - r["u0"]) / (1 + np.abs(r["u0"]))) < 1e-6, b


@pytest.mark.gpu
def test_gpu_kernels_agree_on_a_ragged_batch(nr, rsolver):
    from mpc_code_amd import nmpc
    B = 1000
    rng = np.random.default_rng(9)
    x0 = nr.x0_p * (1.0 + 0.02 * rng.uniform(-1, 1, size=(B, 3)))
    xm = nr.x0_p * (1.0 + 0.02 * rng.uniform(-1, 1, size=(B, 3)))
    res = {}
    for kern in (1, 3, 4):
        rsolver.set_kernel(kern)
        res[kern] = nmpc.run_nmpc_closed_loop(nr, x0, xm, nsteps=10, solver=rsolver, max_sqp=1)
    rsolver.set_kernel(0)
    st = res[1]["STATUS_DYN"]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(res[1]["Xp"]).all(axis=(0, 2)) & (st != 2).all(axis=0)
    assert ok.sum() > B // 2
    for kern in (3, 4):
        assert np.array_equal(res[kern]["STATUS_DYN"][:, ok], st[:, ok]), kern
        for k in ("U", "X_HAT", "XS", "US", "Xp", "D_HAT"):
            a, b = res[kern][k][:, ok], res[1][k][:, ok]
            assert np.isfinite(a).all(), (kern, k)
            assert np.max(np.abs(a - b) / (1 + np.abs(b))) < 1e-6, (kern, k)


@pytest.mark.gpu
def test_gpu_run_exfile_completes_on_the_example(tmp_path):
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "run_exfile.py"), os.path.join(ROOT, "mpc-code_amd", "examples", EX), "--nsteps", "10"],
                         capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.gpu
def test_gpu_full_size(nr, orr, rsolver):
    from mpc_code_amd import nmpc
    B, ns = 16384, 20
    rng = np.random.default_rng(7)
    x0 = np.tile(nr.x0_p, (B, 1)); x0[1:] *= 1.0 + 0.02 * rng.uniform(-1, 1, size=(B - 1, 3))
    r = nmpc.run_nmpc_closed_loop(nr, x0, x0, nsteps=ns, solver=rsolver, max_sqp=1)
    assert rsolver.get_kernel() == 4
    assert np.all(np.isfinite(r["U"]))
    for b in [0] + list(rng.choice(B, 2, replace=False)):
        o = rr.closed_loop(orr, ns, x0_p=x0[b], x0_m=x0[b], max_sqp=1)
        assert not np.any((r["STATUS_DYN"][:, b] == 2) & (o["STATUS_DYN"] != 2)), int(b)
        assert np.max(np.abs(r["U"][:, b] - o["U"]) / (1 + np.abs(o["U"]))) < 1e-6, int(b)
    # SQP to the KKT point at 2048 instances through the per-call OCP: the stage-0 row holds on every solved instance
    cb = 2048
    xh = nr.x0_m * (1.0 + 0.02 * rng.uniform(-1, 1, size=(cb, 3)))
    up = nr.u0 * (1.0 + 0.02 * rng.uniform(-1, 1, size=(cb, 2)))
    d = np.tile(nr.dhat0, (cb, 1))
    u, x1, st, it, sq = _percall(rsolver, nr, xh, d, np.tile(nr.x0_m, (cb, 1)), np.tile(nr.u0, (cb, 1)), up)
    ok = st == 0
    assert ok.sum() > cb // 2
    from mpc_code_amd import symtrace as st_
    g = np.asarray(st_.evaluate(nr.g_ineq, nr._vals(x=xh, u=u, d=d, t=0.0))[0], dtype=float)
    assert g[ok].max() <= 1e-8 and (np.abs(g[ok]) < 1e-7).sum() > 0
