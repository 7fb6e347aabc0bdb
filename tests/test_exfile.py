"""Ex-file surface: the loader runs Ex-style files without CasADi and yields the reference's problem."""
import numpy as np
import pytest

from reference_golden import EX_FIELDS as FIELDS
from reference_golden import EX_FILES, KIND_REFUSALS, assert_fields


def test_cstr_dimensions_and_flags(cstr):
    # reference MPC_code.py:31-52 on Ex_LMPC_CSTR: nw = 253; kal = True -> time-varying Kalman filter
    assert (cstr.nx, cstr.nu, cstr.ny, cstr.nd, cstr.N, cstr.nw) == (3, 2, 3, 3, 50, 253)
    assert cstr.estimator == "kal" and not cstr.DUForm and cstr.y_bounded and cstr.max_iter == 100
    # DARE terminal weight: the same SciPy call as Utilities.py:409; SURVEY.md 8a7 quotes its spectrum
    ev = np.linalg.eigvalsh(cstr.P)
    assert np.allclose(ev, [1.49963e-05, 1.064095, 5.323557], rtol=1e-5)
    assert np.allclose(cstr.A.T @ cstr.P @ cstr.A - cstr.P - cstr.A.T @ cstr.P @ cstr.B @ np.linalg.solve(
        cstr.R + cstr.B.T @ cstr.P @ cstr.B, cstr.B.T @ cstr.P @ cstr.A) + cstr.Q, 0, atol=1e-9)


def test_wb_is_delta_u_form(wb):
    # Ex_LMPC_WB gives S and no R -> DUForm (MPC_code.py:237-239), DARE with R <- S (:253-255); lue -> fixed gain
    assert (wb.nx, wb.nu, wb.ny, wb.nd, wb.nw) == (4, 2, 2, 2, 304)
    assert wb.DUForm and wb.estimator == "kalss" and not wb.y_bounded
    assert np.array_equal(wb.K, np.vstack([np.zeros((4, 2)), np.eye(2)]))
    assert np.all(np.isinf(wb.xmin)) and np.allclose(wb.umax, 0.5)


def test_schedules_follow_callbacks(cstr):
    s = cstr.schedules(30)
    assert np.array_equal(s["ysp"][15], [0.2, 0, 0]) and np.array_equal(s["ysp"][16], [0, 0, 0.1])   # Ex_LMPC_CSTR.py:119-141
    assert np.array_equal(s["pxp"][20], [0.1, 0, 0]) and np.array_equal(s["pxp"][21], [0, 0, 0])     # :40-57
    assert np.array_equal(s["pyp"][7], [0.1, 0.1, 0])                                               # :59-79


@pytest.mark.parametrize("ours,theirs", [("cstr_lmpc.py", "Ex_LMPC_CSTR.py"), ("wood_berry_lmpc.py", "Ex_LMPC_WB.py"),
                                         ("cstr_nlplant_lmpc.py", "Ex_LMPC_nlplant.py"),
                                         ("cstr_xp_nlplant_lmpc.py", "Ex_LMPCxp_nlplant.py")])
def test_unmodified_reference_examples_load_to_the_same_problem(pkg, ref_gold, ours, theirs):
    """The loader's reading of the reference's unmodified Ex-file (tests/golden/reference_examples.npz) and of ours: one problem."""
    a = pkg.load_problem(pkg.example_path(ours))
    pre = "ex_" + theirs[:-3] + "_"
    assert_fields(a, ref_gold, pre, FIELDS)
    for t in (0, 10, 11, 15, 16, 20, 21, 99):
        for i, x in enumerate(a.defSP(t)):
            assert np.array_equal(np.ravel(x), ref_gold[f"{pre}sp{t}_{i}"])
    assert a.estimator == str(ref_gold[pre + "estimator"]) and [a.DUForm, a.N, a.plant_is_linear] == ref_gold[pre + "flags"].tolist() and a.N == 50
    if not a.plant_is_linear:      # the two plant functions integrate to the same states (to rounding: the stored states were computed on another host)
        x, u = ref_gold[pre + "plant_x"], ref_gold[pre + "plant_u"]
        np.testing.assert_allclose(a.plant_step(x, u, 0.4, np.zeros(a.nxp)), ref_gold[pre + "plant"], rtol=1e-13, atol=0)


def test_every_example_of_the_reference_loads_unmodified(pkg, ref_gold):
    """All seven Ex_*.py files of the reference went through load_problem as they are (round 3: the economic one too; recorded in
    tests/golden/reference_examples.npz), and their counterparts here load to the same problem classes; features no path carries are
    still refused loudly."""
    import warnings
    kinds = dict(zip(ref_gold["kinds_files"].tolist(), ref_gold["kinds_types"].tolist()))
    assert kinds == {"Ex_ENMPC.py": "EconomicMPCProblem", "Ex_LMPC_CSTR.py": "LinearMPCProblem", "Ex_LMPC_WB.py": "LinearMPCProblem", "Ex_LMPC_nlplant.py": "LinearMPCProblem",
                     "Ex_LMPCxp_nlplant.py": "LinearMPCProblem", "Ex_NMPC.py": "NonlinearMPCProblem", "Ex_NMPC_dis.py": "NonlinearMPCProblem"}, kinds
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ours = {theirs: type(pkg.load_problem(pkg.example_path(f))).__name__ for theirs, f in EX_FILES.items()}
    assert ours == kinds, ours
    assert ref_gold["kinds_refused"].tolist() == [True] * len(KIND_REFUSALS)
    for over in KIND_REFUSALS:
        with pytest.raises(pkg.UnsupportedProblem):
            pkg.load_problem(pkg.example_path("reactor_enmpc.py"), overrides=over)


def test_overrides_apply_after_the_file(pkg):
    p = pkg.load_problem(pkg.example_path("cstr_lmpc.py"), overrides={"N": 30})
    assert p.N == 30 and p.nw == 3 * 31 + 2 * 30


def test_nonlinear_plant_example(pkg):
    """Linear controller around (xlin, ulin) + non-linear plant integrated by RK4 on the host (Utilities.py:58-82,135-155)."""
    p = pkg.load_problem(pkg.example_path("cstr_nlplant_lmpc.py"))
    assert (p.nx, p.nu, p.ny, p.nd, p.nxp, p.N, p.h, p.plant_Mx) == (3, 2, 2, 2, 3, 50, 0.2, 10)
    assert p.DUForm and p.estimator == "kal" and not p.plant_is_linear and not p.y_bounded
    assert np.allclose(p.fx_const, p.extras.get("xlin", np.array([0.5, 350, 0.659])) - p.A @ [0.5, 350, 0.659] - p.B @ [300, 0.1])
    # the operating point is (nearly) a steady state of the plant; a hotter jacket heats the reactor and burns reactant
    x1 = p.plant_step(p.x0_p[None], p.u0[None], 0.0, np.zeros(3))[0]
    assert np.abs(x1 - p.x0_p).max() < 0.2 and x1[2] == p.x0_p[2]
    x2 = p.plant_step(p.x0_p[None], (p.u0 + [3.0, 0.0])[None], 0.0, np.zeros(3))[0]
    assert x2[1] > x1[1] and x2[0] < x1[0]
    # RK4 with Mx sub-steps: halving the step changes the result at the O(dt^4) level only
    import copy
    q = copy.copy(p); q.plant_Mx = 20
    assert 0 < np.abs(q.plant_step(p.x0_p[None], p.u0[None], 0.0, np.zeros(3)) - x1).max() < 1e-6
    from mpc_code_amd.exfile import _old_div, _vertcat
    assert _old_div(7, 2) == 3 and _old_div(7.0, 2) == 3.5 and _old_div(-8750, 350) == -25
    assert _vertcat(1.0, np.array([1.0, 2.0]), 3.0).shape == (3, 2) and _vertcat(np.zeros((2, 4)), np.ones(4)).shape == (3, 4)
