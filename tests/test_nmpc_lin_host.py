"""The non-linear tracking path with a continuous model and offree = 'lin', StateFeedback and G_wn / Q_wn, without a GPU: both
loaders on the three models of tests/nmpc_lin_family.py and on examples/reactor_nmpc_lin.py, the NumPy evaluators against the oracle's, the traced
Jacobians, every new refusal with its message, the generated header, the goldens (tests/golden/nmpc_lin_family.npz) and the noise reference
(tests/nmpc_state_noise_ref.py).
"""
import warnings

import numpy as np
import pytest

import nmpc_family as fam
import nmpc_lin_family as lf
import nmpc_state_noise_ref as snr

TOL_CAP = 2e-7      # the cap of the GPU tests' tolerance (tests/test_nmpc_lin_family.py): every switch has to move its member by 100 times this


@pytest.fixture(scope="module")
def gold():
    g = np.load(lf.GOLDEN)
    return {k: g[k] for k in g.files}


def points(p, n=4, seed=0):
    rng = np.random.default_rng(seed)
    return (p.x0_m * (1.0 + 0.2 * rng.uniform(-1, 1, size=(n, p.nx))), p.u0 * (1.0 + 0.2 * rng.uniform(-1, 1, size=(n, p.nu))),
            0.05 * rng.uniform(-1, 1, size=(n, p.nd)), rng.uniform(0, 5, size=n))


def ev(p, exprs, x, u, d, t=0.0):
    from mpc_code_amd import symtrace as st
    return np.array([float(v) for v in st.evaluate(list(exprs), p._vals(x=x, u=u, d=d, t=t))])


# ------------------------------------------------------------------------------------------------- loaders
CLASS = {"cl21": (6, "ekf", [0, 1], False), "cl21sf": (6, "ekf", [0, 1], True), "cl42": (9, "lue", [1, 3], False)}


@pytest.mark.parametrize("member", lf.MEMBERS)
def test_both_loaders_accept_the_member(pkg, member):
    p, o = lf.load_product(member), lf.load_oracle(member)
    N, est, ycols, sfb = CLASS[member]
    assert (p.nx, p.nu, p.ny, p.nd) == lf.DIMS[member] and p.nxp == p.nx and p.N == N
    assert (p.discrete, p.plant_discrete, p.offree, p.estimator, p.ycols, p.StateFeedback, p.ng) == (False, False, "lin", est, ycols, sfb, 0)
    assert np.abs(p.Bd).max() > 0 and np.abs(p.Cd).max() > 0
    assert (p.dmin is not None) == (member == "cl42")
    if member == "cl42":
        assert all(np.isfinite(getattr(p, k)).all() for k in ("xmin", "xmax", "umin", "umax", "ymin", "ymax", "dmin", "dmax"))
    for k in ("Q", "R", "Qss", "Rss", "Pf", "umin", "umax", "xmin", "xmax", "ymin", "ymax", "x0_p", "x0_m", "u0", "dhat0", "P0"):
        assert np.array_equal(getattr(o, k), getattr(p, k)), k
    for k in ("K", "Bd", "Cd", "dmin", "dmax", "Q_kf", "R_kf"):
        a, b = getattr(o, k), getattr(p, k)
        assert (a is None and b is None) or np.array_equal(a, b), k
    assert (o.discrete, o.estimator, o.offree, o.N) == (False, est, "lin", N)


def test_the_shipped_example_loads_with_all_three_features(pkg):
    with pytest.warns(UserWarning, match="simulated only on request"):
        p = pkg.load_problem(pkg.example_path("reactor_nmpc_lin.py"))
    assert (p.discrete, p.offree, p.estimator, p.StateFeedback, p.ycols) == (False, "lin", "ekf", True, [0, 1])
    assert np.array_equal(p.Bd, np.zeros((2, 2))) and np.array_equal(p.Cd, np.eye(2))
    assert np.array_equal(p.G_wn, 1e-2 * np.eye(2)) and np.array_equal(p.Q_wn, 1e-3 * np.eye(2)) and np.array_equal(p.R_wn, 1e-7 * np.eye(2))
    from mpc_code_amd import nmpc
    V, W = nmpc.path_noise(p, 5, 3, seed=4)      # per step first v, then w (noise.loop_noise)
    rng = np.random.default_rng(4)
    for k in range(5):
        assert np.allclose(V[k], rng.standard_normal((3, 2)) * np.sqrt(1e-7), rtol=1e-12, atol=0)
        assert np.allclose(W[k], rng.standard_normal((3, 2)) * 1e-2 * np.sqrt(1e-3), rtol=1e-12, atol=0)
    # without G_wn the draws of a seed stay what measurement_noise gives
    q = pkg.load_problem(pkg.example_path("reactor_nmpc_lin.py"), overrides={"G_wn": None, "Q_wn": None})
    V2, W2 = nmpc.path_noise(q, 5, 3, seed=4)
    assert W2 is None and np.array_equal(V2, nmpc.measurement_noise(q, 5, 3, 4))


@pytest.mark.parametrize("member", ("cl21", "cl42"))
def test_numpy_evaluators_equal_the_oracle_s(pkg, member):
    """model_step (RK4 of f, then + Bd d) and model_output (+ Cd d) against nmpc_oracle.model_fx / model_fy at random points, to 1e-13; the twin cl21sf,
    which the oracle cannot evaluate (it has no User_fym to call), against cl21's."""
    import nmpc_oracle as no
    p, o = lf.load_product(member), lf.load_oracle(member)
    x, u, d, t = points(p)
    for i in range(len(x)):
        assert np.abs(p.model_step(x[i], u[i], d[i], t[i]) - no.model_fx(o, x[i], u[i], d[i], t[i])).max() < 1e-13
        assert np.abs(p.model_output(x[i], u[i], d[i], t[i]) - no.model_fy(o, x[i], u[i], d[i], t[i])).max() < 1e-13
        assert np.abs(p.plant_step(x[i], u[i], t[i]) - no.plant_fx(o, x[i], u[i], t[i])).max() < 1e-13
        assert np.abs(p.plant_output(x[i], u[i], t[i]) - no.plant_fy(o, x[i], u[i], t[i])).max() < 1e-13
    if member == "cl21":
        s = lf.load_product("cl21sf")
        assert np.array_equal(s.model_step(x, u, d, 0.0), p.model_step(x, u, d, 0.0)) and np.array_equal(s.model_output(x, u, d, 0.0), p.model_output(x, u, d, 0.0))
        assert np.array_equal(s.plant_output(x, u, 0.0), x)      # Fy_p = x_p
    assert np.abs(p.model_step(x, u, d, 0.0) - p.model_step(x, u, 0 * d, 0.0) - d @ p.Bd.T).max() < 1e-15      # + Bd d after the integration, not through it


@pytest.mark.parametrize("member", lf.MEMBERS)
def test_traced_jacobians_against_central_differences(pkg, member):
    p = lf.load_product(member)
    x, u, d, _ = points(p, seed=1)
    assert all(e.is_const(0.0) for row in p.f_d for e in row)      # f does not see d: the step's sensitivity to d is Bd itself
    for i in range(len(x)):
        z0 = np.concatenate([x[i], u[i], d[i]])
        split = lambda z: (z[:p.nx], z[p.nx:p.nx + p.nu], z[p.nx + p.nu:])
        for exprs, jacs in ((p.f, (p.f_x, p.f_u, p.f_d)), (p.hy, (p.h_x, None, p.h_d))):
            fd = np.zeros((len(exprs), z0.size))
            for j in range(z0.size):
                e = np.zeros(z0.size); e[j] = 1e-6 * max(1.0, abs(z0[j]))
                fd[:, j] = (ev(p, exprs, *split(z0 + e)) - ev(p, exprs, *split(z0 - e))) / (2 * e[j])
            for J, cols in zip(jacs, (slice(0, p.nx), slice(p.nx, p.nx + p.nu), slice(p.nx + p.nu, None))):
                if J is not None:
                    got = np.array([ev(p, row, x[i], u[i], d[i]) for row in J])
                    assert np.allclose(got, fd[:, cols], rtol=1e-6, atol=1e-7)
    assert np.array_equal(np.array([ev(p, row, x[0], u[0], d[0]) for row in p.h_d]), p.Cd)


def test_the_state_feedback_twin_is_the_same_problem_and_the_same_code(pkg):
    from mpc_code_amd import nlcodegen
    a, b = lf.load_product("cl21"), lf.load_product("cl21sf")
    for k in ("Q", "R", "Qss", "Rss", "Pf", "umin", "umax", "xmin", "xmax", "ymin", "ymax", "umin_ss", "umax_ss", "xmin_ss", "xmax_ss", "ymin_ss", "ymax_ss",
              "x0_p", "x0_m", "u0", "dhat0", "P0", "Bd", "Cd", "Q_kf", "R_kf"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert (a.N, a.h, a.Mx, a.ycols, a.estimator, a.offree) == (b.N, b.h, b.Mx, b.ycols, b.estimator, b.offree)
    assert not a.StateFeedback and b.StateFeedback and "User_fym" not in b.funcs
    ha, hb = nlcodegen.emit_model_header(a), nlcodegen.emit_model_header(b)
    body = lambda t: t.split("\n", 1)[1]      # (the first line names the file)
    assert body(ha) == body(hb)
    assert "cl21sf" in hb.split("\n", 1)[0]    # ... which is why the library hash differs: it covers the whole header, the name included
    assert nlcodegen.nmpc_library_path(ha) != nlcodegen.nmpc_library_path(hb)


# ------------------------------------------------------------------------------------------------- refusals
def _dep_on_d(x, u, d, t, px):
    return [-x[0] + 0.3 * x[1] + u[0] + 0.1 * d[0], 0.5 * x[0] - 0.8 * x[1]]


@pytest.mark.parametrize("member,over,match", [
    ("cl21", {"User_fxm_Cont": _dep_on_d}, "User_fxm_Cont depends on d"),
    ("cl21", {"Bd": None}, "'Bd' missing"),
    ("cl21", {"Cd": None}, "'Cd' missing"),
    ("cl42", {"StateFeedback": True}, "StateFeedback = True needs ny = nx"),
    ("cl21sf", {"def_pyp": lambda t: [np.zeros(2)]}, "StateFeedback = True with def_pyp"),
    ("cl21sf", {"offree": "no"}, "StateFeedback = True with offree = 'no'"),
    ("cl21", {"G_wn": np.eye(2)}, "G_wn and Q_wn .* have to come together"),
    ("cl21", {"Q_wn": np.eye(2)}, "G_wn and Q_wn .* have to come together"),
    ("cl21", {"G_wn": np.ones((2, 3)), "Q_wn": np.eye(2)}, None),      # (Q_wn has to be [nw, nw] with nw = G_wn's second dimension: a shape error)
])
def test_loader_refuses_loudly(pkg, member, over, match):
    from mpc_code_amd.problem import UnsupportedProblem
    with pytest.raises(UnsupportedProblem if match else ValueError, match=match or "Q_wn has shape"):
        lf.load_product(member, over)


def test_noise_matrices_are_kept_and_warned_about(pkg):
    import mpc_code_amd
    with pytest.warns(UserWarning, match="R_wn / G_wn"):
        p = mpc_code_amd.load_problem(lf.model_path("cl21"), overrides={"G_wn": 0.1 * np.eye(2), "Q_wn": 1e-4 * np.eye(2)})
    assert np.array_equal(p.G_wn, 0.1 * np.eye(2)) and np.array_equal(p.Q_wn, 1e-4 * np.eye(2)) and p.R_wn is None
    # G_wn [nxp, nw] with nw != nxp: carried, one draw per noise component
    from mpc_code_amd import nmpc
    G = np.array([[1.0, 0.0, 0.5], [0.0, 2.0, 0.5]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        q = mpc_code_amd.load_problem(lf.model_path("cl21"), overrides={"G_wn": G, "Q_wn": np.diag([1e-4, 4e-4, 9e-4])})
    assert q.G_wn.shape == (2, 3) and q.Q_wn.shape == (3, 3)
    V, W = nmpc.path_noise(q, 4, 5, seed=2)
    rng = np.random.default_rng(2)
    assert V is None and W.shape == (4, 5, 2)
    for k in range(4):
        assert np.allclose(W[k], (rng.standard_normal((5, 3)) * np.array([1e-2, 2e-2, 3e-2])) @ G.T, rtol=1e-12, atol=1e-18)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert mpc_code_amd.load_problem(lf.model_path("cl21")).G_wn is None


# ------------------------------------------------------------------------------------------------- generated header
def test_header_carries_lin_bd_and_the_table(pkg):
    from mpc_code_amd import nlcodegen
    p = lf.load_product("cl42")
    hdr = nlcodegen.emit_model_header(p)
    assert "static constexpr bool LIN_BD = true;" in hdr
    assert "static constexpr double BD[4][2] = {{0.1, 0.0}, {0.0, 0.05}, {0.0, 0.1}, {0.02, 0.0}};" in hdr      # exact zeros as literal zeros
    assert "DISCRETE = false, PLANT_DISCRETE = false, DUV = false" in hdr and "#define MPC_NL_WAVE_FITS 1" in hdr
    # the library hash changes with Bd and with LIN_BD
    other = nlcodegen.emit_model_header(lf.load_product("cl42", {"Bd": 2.0 * p.Bd}))
    assert nlcodegen.nmpc_library_path(other) != nlcodegen.nmpc_library_path(hdr)
    without = "\n".join(l for l in hdr.split("\n") if "LIN_BD" not in l and " BD[" not in l)
    assert without != hdr and nlcodegen.nmpc_library_path(without) != nlcodegen.nmpc_library_path(hdr)


@pytest.mark.parametrize("ex", ["cstr_nmpc.py", "reactor_nmpc.py", "quadtank_nmpc_dis.py"])
def test_models_without_the_feature_generate_the_header_they_did(pkg, ex):
    """continuous 'nl' and discrete 'lin' (whose + Bd d is inside the traced map): not a character of LIN_BD - the constant is declared only where it is set
    and read through LinBdOf (mpc_nmpc.hpp), because tests/test_nmpc_rows.py pins the sha256 of these very headers."""
    from mpc_code_amd import nlcodegen
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = pkg.load_problem(pkg.example_path(ex))
    hdr = nlcodegen.emit_model_header(p)
    assert "LIN_BD" not in hdr and "BD[" not in hdr
    assert (p.offree, p.discrete) == (("lin", True) if ex.startswith("quadtank") else ("nl", False))
    d42 = nlcodegen.emit_model_header(fam.load_product("d42"))
    assert "LIN_BD" not in d42


# ------------------------------------------------------------------------------------------------- goldens
def test_golden_starts_and_statuses(pkg, gold):
    for name in lf.case_names():
        member, steps, _, _ = lf.case_spec(name)
        x0, xm = lf.starts(name, lf.load_product(member).x0_p)
        assert np.array_equal(x0, gold[name + "_x0"]) and np.array_equal(xm, gold[name + "_xm"]), name
        assert gold[name + "_U"].shape[0] == steps and steps <= 12
        if name == lf.HOLD_CASE:
            held = np.isin(np.arange(lf.B), lf.HELD)
            assert x0.shape[0] == lf.B and lf.HELD == (0, 1, 4, 5, 8)      # two of each full wave and the lone slot
            assert (gold[name + "_STATUS_DYN"][:, held] == 2).all() and not gold[name + "_STATUS_DYN"][:, ~held].any() and not gold[name + "_STATUS_SS"].any()
        else:
            assert x0.shape[0] == lf.B and np.abs(x0 - xm).min(axis=1).max() > 0      # plant and model start apart
            assert not gold[name + "_STATUS_DYN"].any() and not gold[name + "_STATUS_SS"].any(), name
    assert float(gold["E_ref"]) == max(float(gold[n + "_eref"]) for n in lf.case_names())


def test_every_switch_bites(gold):
    """Bd = 0, Cd = 0, K halved, and G = Bd left out of the EKF's covariance update only: the oracle's rti run moves by at least 100 x the tolerance cap."""
    for member, sw in lf.SWITCHES.items():
        for tag in sw:
            assert float(gold[f"bite_{member}_{tag}"]) >= 100 * TOL_CAP, (member, tag)
    assert float(gold["cl21_gain_bite"]) >= 100 * TOL_CAP


@pytest.mark.parametrize("member", lf.GOLDEN_MEMBERS)
def test_oracle_reproduces_three_rows_of_the_member(member, gold):
    name = member + "_rti"
    _, _, max_sqp, over = lf.case_spec(name)
    b = 4
    r = lf.oracle_instance(member, over, 3, max_sqp, gold[name + "_x0"][b], gold[name + "_xm"][b])
    for k in lf.LOGS:
        assert np.allclose(r[k], gold[f"{name}_{k}"][:3, b], rtol=1e-10, atol=1e-10), k
    for k in lf.ILOGS:
        assert np.array_equal(r[k], gold[f"{name}_{k}"][:3, b]), k


# ------------------------------------------------------------------------------------------------- the noise reference
def test_state_noise_reference(gold):
    """With w = 0 the reference is the plain closed_loop to the bit; with w != 0, Xp[k+1] minus the noise-free plant step from (Xp[k], U[k]) is pxp_k + w_k to 1e-14."""
    import nmpc_oracle as no
    o = lf.load_oracle("cl21", {"def_pxp": lambda t: [np.array([0.0, 0.004])] if t >= 1.0 else [np.zeros(2)]})
    x0, xm = gold["cl21_rti_x0"][:2], gold["cl21_rti_xm"][:2]
    K = 5
    rng = np.random.default_rng(3)
    v, w = 1e-3 * rng.standard_normal((K, 2, 2)), 1e-2 * rng.standard_normal((K, 2, 2))
    plain = [no.closed_loop(o, K, x0_p=x0[b], x0_m=xm[b], max_sqp=1, sqp_tol=lf.SQP_TOL, v_wn=v[:, b]) for b in range(2)]
    zero = snr.closed_loop(o, K, x0, xm, v=v, w=np.zeros_like(w))
    for k in snr.LOGS + snr.ILOGS:
        assert np.array_equal(zero[k], np.stack([r[k] for r in plain], axis=1)), k
    r = snr.closed_loop(o, K, x0, xm, v=v, w=w)
    pxp = o.schedules(K)["pxp"]
    assert np.abs(pxp).max() > 0
    for k in range(K - 1):
        for b in range(2):
            step = no.plant_fx(o, r["Xp"][k, b], r["U"][k, b], k * o.h)
            assert np.abs(r["Xp"][k + 1, b] - step - (pxp[k] + w[k, b])).max() < 1e-14
    assert np.abs(r["Xp"][1:] - zero["Xp"][1:]).min() > 0      # the noise is in the loop
