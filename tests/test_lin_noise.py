"""White noise R_wn, G_wn / Q_wn in the resident closed loop of the linear path (mpc_loop_set_noise; MPC_code.py:537-541, 822-827) on every loop kernel:
against the C restatement with the noise folded into its schedule (tests/lin_noise_ref.py; the reference itself is checked without a GPU in
tests/test_lin_noise_host.py), bit-for-bit invariances of the launch structure, the fused loop against the call-by-call one where there is no C
restatement, and the error paths."""
import ctypes as ct
import dataclasses

import numpy as np
import pytest

import lin_noise_ref as ref
from test_gpu_parity import LOOP_KERNELS, _with_model_params, assert_same_closed_loop

pytestmark = pytest.mark.gpu

TOL = 1e-7
FLOAT_LOGS = ("U", "X_HAT", "XS", "US", "YS", "Xp", "D_HAT")
INT_LOGS = ("STATUS_DYN", "STATUS_SS", "ITERS_DYN", "ITERS_SS")


def fused(s, p, x0, v, w, runs=((0, ref.NSTEPS),), alloc=True, set_noise=True):
    """one resident loop through the C-ABI: state, schedule, noise (None: none), the given (k0, nsteps) runs; every log"""
    n = sum(r[1] for r in runs)
    if alloc:
        s.loop_alloc(len(x0), n, 2)
    s.loop_set_state(x0, x0)
    s.loop_set_schedule(p.schedules(n))
    s.loop_set_model_schedule(None, None)
    if set_noise:
        s.loop_set_noise(v, w)
    for k0, m in runs:
        s.loop_run(k0, m)
    s.loop_sync()
    return {k: s.loop_get_log(k) for k in FLOAT_LOGS + INT_LOGS}


def same_bits(a, b, what):
    for k in FLOAT_LOGS + INT_LOGS:
        assert np.array_equal(a[k], b[k]), (what, k, np.abs(a[k].astype(float) - b[k]).max())


# ---- A. against the C restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cstr", "wb"])
@pytest.mark.parametrize("lk", LOOP_KERNELS)
def test_noisy_loop_matches_folded_c_restatement(lk, which, oracle_c, solver_factory):
    """B = 70 (padded stride 128, a last wave of the wave kernel with two of four instances), 12 steps, both noises of noise_seed = 7 through the driver;
    Kalman filter (CSTR) and fixed gain (Wood-Berry).  On the wave kernel also each noise alone: the strides of v and w cannot be swapped unseen."""
    from mpc_code_amd.driver import run_closed_loop
    p, x0 = ref.problem(which), ref.start_states(which)
    s = solver_factory(p, lk)
    g = run_closed_loop(p, x0, x0, ref.NSTEPS, solver=s, fused=True, noise_seed=ref.SEED)
    v, w = ref.draws(which)
    assert np.array_equal(g["V_WN"], v) and np.array_equal(g["W_WN"], w)
    c = ref.c_reference(oracle_c, which)
    for k in ("U", "X_HAT", "Xp"):
        print(which, lk, k, np.abs(g[k] - c[k]).max())
    assert_same_closed_loop(g, c, p, TOL)
    assert np.array_equal(g["Yp"], g["Xp"] @ p.Cp.T + p.schedules(ref.NSTEPS)["pyp"][:, None, :] + v)
    free = fused(s, p, x0, None, None, alloc=False, set_noise=False)      # the driver cleared the noise of the caller's solver
    assert_same_closed_loop(free, ref.c_reference(oracle_c, which, "none"), p, TOL)
    if lk == 3:
        for mode in ("v", "w"):
            one = fused(s, p, x0, *ref.draws(which, mode))
            assert_same_closed_loop(one, ref.c_reference(oracle_c, which, mode), p, TOL)


# ---- B. bit-for-bit invariances -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lk", LOOP_KERNELS)
def test_launch_structure_and_switching_off_do_not_change_a_bit(lk, solver_factory):
    p, x0 = ref.problem("cstr"), ref.start_states("cstr")
    v, w = ref.draws("cstr")
    s = solver_factory(p, lk)
    one = fused(s, p, x0, v, w)
    assert np.abs(one["U"] - fused(s, p, x0, None, None)["U"]).max() > 0.5      # (the noise is felt: tests/test_lin_noise_host.py)
    s.set_option("steps_per_launch", 5)
    same_bits(fused(s, p, x0, v, w), one, "steps_per_launch = 5")      # launches of 5, 5 and 2 steps: the per-launch offset of both arrays
    s.set_option("steps_per_launch", 50)
    same_bits(fused(s, p, x0, v, w, runs=((0, 7), (7, 5))), one, "two runs")      # a second mpc_loop_run at k0 = 7
    fresh = fused(solver_factory(p, lk), p, x0, None, None, set_noise=False)      # a handle that never saw noise
    s.loop_set_noise(v, w)
    same_bits(fused(s, p, x0, None, None, alloc=False), fresh, "loop_set_noise(None, None)")
    same_bits(fused(s, p, x0, np.zeros_like(v), np.zeros_like(w)), fresh, "zero arrays")
    same_bits(fused(s, p, x0, np.zeros_like(v), None), fresh, "zero v alone")
    if lk == 3:
        for ni in (1, 2, 4):      # 70 instances: whole waves of one and two, a last wave with two of four slots empty
            s.set_option("wave_instances", ni)
            same_bits(fused(s, p, x0, v, w), one, f"wave_instances = {ni}")
        s.set_option("wave_instances", 0)


# ---- C. fused against call-by-call on the lane loops without a C restatement ----------------------------------------------------------------------
def fused_and_stepwise(p, x0p, x0m, n, s, sigma_note=""):
    from mpc_code_amd.driver import run_closed_loop
    f = run_closed_loop(p, x0p, x0m, n, solver=s, fused=True, noise_seed=ref.SEED)
    c = run_closed_loop(p, x0p, x0m, n, solver=s, fused=False, noise_seed=ref.SEED)
    assert np.array_equal(f["V_WN"], c["V_WN"]) and np.array_equal(f["W_WN"], c["W_WN"])
    q = run_closed_loop(p, x0p, x0m, n, solver=s, fused=True)
    assert "V_WN" not in q and np.abs(q["U"] - f["U"]).max() > 10 * np.abs(f["U"] - c["U"]).max()      # the noise is felt, far above what is compared
    return f, c


def test_soft_loop_fused_equals_the_three_calls(pkg):
    """loop_kernel_soft; inputs and tolerance of tests/test_soft.py::test_gpu_soft_fused_loop_equals_the_three_calls_per_step"""
    from mpc_code_amd import capi
    soft = ref.with_noise(pkg, "cstr_lmpc_soft.py")
    rng = np.random.default_rng(5)
    B, ns = 70, 7
    x0 = np.vstack([soft.x0_p[None], soft.x0_p[None] + rng.uniform(-1.0, 1.0, size=(B - 1, soft.nxp))])
    s = capi.Solver(soft)
    try:
        s.set_option("steps_per_launch", 3)
        f, c = fused_and_stepwise(soft, x0, x0[:, :soft.nx], ns, s)
    finally:
        s.close()
    for k in ("STATUS_DYN", "STATUS_SS"):
        assert np.array_equal(f[k], c[k]), k
    for k in ("U", "X_HAT", "XS", "US", "Xp", "Yp", "D_HAT", "Sl"):
        print("soft", k, np.abs(f[k] - c[k]).max())
        assert np.abs(f[k] - c[k]).max() < 5e-6, (k, np.abs(f[k] - c[k]).max())


def test_model_parameter_loop_fused_equals_the_three_calls(pkg, cstr):
    """loop_kernel_pxy (def_px / def_py over the horizon; p_y_k and v_k both enter the measurement, p_x_k and w_k both the plant state); problem, starts and
    tolerance of tests/test_gpu_parity.py::test_model_parameters_over_the_horizon"""
    from mpc_code_amd import capi
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = _with_model_params(pkg, **ref.noise_overrides(cstr))
    assert p.has_model_params and p.R_wn is not None
    rng = np.random.default_rng(11)
    x0 = rng.uniform([-0.3, -4, -3], [0.3, 4, 3], size=(70, 3))
    s = capi.Solver(p)
    try:
        s.set_option("steps_per_launch", 3)
        f, c = fused_and_stepwise(p, x0, x0, 8, s)
    finally:
        s.close()
    for k in ("STATUS_DYN", "STATUS_SS"):
        assert np.array_equal(f[k], c[k]), k
    for k in ("U", "X_HAT", "XS", "US", "Xp", "Yp", "Y_HAT", "YS", "D_HAT"):
        print("pxy", k, np.abs(f[k] - c[k]).max())
        assert np.abs(f[k] - c[k]).max() < 1e-8, (k, np.abs(f[k] - c[k]).max())


def test_user_plant_loop_fused_equals_the_three_calls(pkg, xp_nlplant):
    """The compiled user plant (nx = 4, nxp = 3, ny = 2: the two noise arrays differ in shape); starts, steps and tolerance of
    tests/test_gpu_parity.py::test_fused_closed_loop_with_the_user_plant, on the instance-per-lane kernel only (the model is open-loop unstable: see there),
    noise of the size of that test's start spread."""
    from mpc_code_amd import capi
    import warnings
    q = xp_nlplant
    spread = np.array([2e-4, 0.02, 2e-4])
    over = {"R_wn": np.diag((np.abs(q.Cp) @ spread) ** 2).tolist(), "G_wn": np.eye(3).tolist(), "Q_wn": np.diag(spread ** 2).tolist()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = pkg.load_problem(pkg.example_path("cstr_xp_nlplant_lmpc.py"), overrides=over)
    assert (p.nx, p.nxp, p.ny) == (4, 3, 2)
    rng = np.random.default_rng(3)
    B, K = 48, 12
    x0p = p.x0_p + rng.normal(size=(B, p.nxp)) * spread
    x0m = np.hstack([x0p, np.zeros((B, p.nx - p.nxp))])
    s = capi.Solver(p)
    try:
        assert s.fused_plant and s.get_option("loop_kernel") == 1
        f, c = fused_and_stepwise(p, x0p, x0m, K, s)
    finally:
        s.close()
    assert np.array_equal(f["STATUS_DYN"], c["STATUS_DYN"]) and np.array_equal(f["STATUS_SS"], c["STATUS_SS"])
    for k in ("U", "Xp", "X_HAT", "XS", "D_HAT", "Yp"):
        print("user plant", k, np.abs(f[k] - c[k]).max())
        assert np.abs(f[k] - c[k]).max() < 1e-4, (k, np.abs(f[k] - c[k]).max())
    assert np.array_equal(f["Yp"], f["Xp"] @ p.Cp.T + p.schedules(K)["pyp"][:, None, :] + f["V_WN"])


# ---- D. errors ------------------------------------------------------------------------------------------------------------------------------------
def test_error_paths(pkg, solver_factory):
    from mpc_code_amd.capi import MpcAmdError, Solver
    p, x0 = ref.problem("cstr"), ref.start_states("cstr")
    v, w = ref.draws("cstr")
    dp = ct.POINTER(ct.c_double)
    s = Solver(p)
    try:
        assert s.lib.mpc_loop_set_noise(s.h, 12, v.ctypes.data_as(dp), None) == -1 and b"mpc_loop_alloc" in s.lib.mpc_last_error()      # before mpc_loop_alloc
        with pytest.raises((MpcAmdError, ValueError)):
            s.loop_set_noise(v, w)
        s.loop_alloc(len(x0), ref.NSTEPS, 2)
        for bad_v, bad_w in ((v[:, :69], None), (v[..., :2], None), (None, w[:, :, :2]), (v[0], None), (v, w[:5])):
            with pytest.raises(ValueError, match="noise"):
                s.loop_set_noise(bad_v, bad_w)
        assert s.lib.mpc_loop_set_noise(s.h, 0, v.ctypes.data_as(dp), None) == -1 and s.lib.mpc_loop_set_noise(s.h, 13, v.ctypes.data_as(dp), None) == -1
        s.loop_set_state(x0, x0); s.loop_set_schedule(p.schedules(ref.NSTEPS))
        s.loop_set_noise(v[:8], w[:8])
        with pytest.raises(MpcAmdError, match="noise"):      # the schedule has 12 steps, the noise 8
            s.loop_run(0, 12)
        with pytest.raises(MpcAmdError, match="noise"):
            s.loop_run(6, 3)
        s.loop_run(0, 8); s.loop_sync()
        noisy = s.loop_get_log("U")[:8]
        # a refused call leaves the noise in force as it was: the same eight steps again, to the bit
        assert s.lib.mpc_loop_set_noise(s.h, 13, v.ctypes.data_as(dp), None) == -1
        s.loop_set_state(x0, x0); s.loop_run(0, 8); s.loop_sync()
        assert np.array_equal(s.loop_get_log("U")[:8], noisy)
        # a second mpc_loop_alloc clears the noise: the loop of a handle that never saw any
        free = fused(s, p, x0, None, None, set_noise=False)
        fresh = fused(solver_factory(p), p, x0, None, None, set_noise=False)
        same_bits(free, fresh, "after a second mpc_loop_alloc")
        assert np.abs(noisy - free["U"][:8]).max() > 0.5
    finally:
        s.close()
    s = Solver(dataclasses.replace(p, estimator="none"))      # MPC_EST_NONE: nothing reads the measurement; the state noise is still taken
    try:
        s.loop_alloc(len(x0), ref.NSTEPS, 2)
        with pytest.raises(MpcAmdError, match=r"\(-8\)"):
            s.loop_set_noise(v, None)
        s.loop_set_noise(None, w)
        with pytest.raises(MpcAmdError, match=r"\(-8\)"):      # ... and refused, it leaves w in force
            s.loop_set_noise(v, w)
        kept = fused(s, p, x0, None, None, alloc=False, set_noise=False)
        s.loop_set_noise(None, None)
        from mpc_code_amd.driver import run_closed_loop
        for mode in (True, False):      # the driver refuses the same case in both of its modes
            with pytest.raises(ValueError, match="without estimator"):
                run_closed_loop(s.p, x0, x0, ref.NSTEPS, solver=s, fused=mode, noise_seed=ref.SEED)
        open_loop = fused(s, p, x0, None, None, alloc=False, set_noise=False)
        moved = fused(s, p, x0, None, w, alloc=False)
        same_bits(kept, moved, "w kept after a refused call")
        assert np.array_equal(moved["Xp"][0], open_loop["Xp"][0]) and np.abs(moved["Xp"][1:] - open_loop["Xp"][1:]).max() > 1e-3
    finally:
        s.close()
