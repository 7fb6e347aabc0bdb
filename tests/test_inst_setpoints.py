"""Per-instance set-point schedules in the resident closed loop of the linear path (mpc_loop_set_setpoints) on every loop kernel:
against the C restatement run instance by instance with each instance's own schedule (tests/inst_setpoints_ref.py; the yardstick itself is checked without
a GPU in tests/test_inst_setpoints_host.py), bit for bit against shared-schedule runs, the fused loop against the call-by-call one where there is no C
restatement, and the error paths.  B = 70 (padded stride 128, a last wave of the wave kernel with two of four slots empty), 12 steps; instance b tracks
s_{b mod 3}, and s_2 has a stretch whose set point lies far outside the bounds (that instance's target rides its bounds next to neighbours that move freely)."""
import ctypes as ct

import numpy as np
import pytest

import inst_setpoints_ref as ref
import lin_noise_ref as lnr
from test_gpu_parity import LOOP_KERNELS, _with_model_params, assert_same_closed_loop
from test_lin_noise import FLOAT_LOGS, INT_LOGS, TOL, same_bits

pytestmark = pytest.mark.gpu

N = ref.NSTEPS


def fused(s, x0, sched, ysp=None, usp=None, runs=((0, N),), alloc=True, set_sp=True, v=None, w=None):
    """one resident loop through the C-ABI: state, shared schedule, per-instance set points (after the schedule, which clears them), the (k0, nsteps) runs"""
    n = sum(r[1] for r in runs)
    if alloc:
        s.loop_alloc(len(x0), n, 2)
    s.loop_set_state(x0, x0)
    s.loop_set_schedule(sched)
    s.loop_set_model_schedule(None, None)
    s.loop_set_noise(v, w)
    if set_sp:
        s.loop_set_setpoints(ysp, usp)
    for k0, m in runs:
        s.loop_run(k0, m)
    s.loop_sync()
    return {k: s.loop_get_log(k) for k in FLOAT_LOGS + INT_LOGS}


# ---- A. against the C restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cstr", "wb", "cstr_rss"])
@pytest.mark.parametrize("lk", LOOP_KERNELS)
def test_per_instance_loop_matches_c_restatement(lk, which, oracle_c, solver_factory):
    """through the driver, both arrays; Kalman filter (CSTR), fixed gain and input-move form (Wood-Berry), and the CSTR whose target reads usp (Rss != 0)"""
    from mpc_code_amd.driver import run_closed_loop
    p, x0 = ref.problem(which), ref.start_states(which)
    ysp, usp = ref.arrays(which)
    s = solver_factory(p, lk)
    g = run_closed_loop(p, x0, x0, N, solver=s, fused=True, setpoints={"ysp": ysp, "usp": usp})
    assert np.array_equal(g["YSP"], ysp, equal_nan=True) and np.array_equal(g["USP"], usp)
    c = ref.c_reference(oracle_c, which)
    for k in ("U", "X_HAT", "XS", "US", "Xp"):
        print(f"LEVEL inst-setpoints {which} loop_kernel {lk} {k}: {np.abs(g[k] - c[k]).max():.2e}")
    assert_same_closed_loop(g, c, p, TOL)
    assert not (g["STATUS_SS"] == 2).any()      # (a set point enters the target's cost alone: none makes it infeasible)
    # the driver cleared the set points of the caller's solver: the next plain run is the shared schedule's
    plain = fused(s, x0, p.schedules(N), alloc=False, set_sp=False)
    assert_same_closed_loop(plain, oracle_c.OracleC(p).closed_loop(N, x0, x0), p, TOL)


def test_wave_kernel_each_array_alone_and_with_both_noises(oracle_c, solver_factory):
    """ysp alone and usp alone (the two strides cannot be swapped unseen; Rss != 0, so usp is read), and both together with v and w of noise_seed = 7"""
    from mpc_code_amd.driver import run_closed_loop
    which = "cstr_rss"
    p, x0 = ref.problem(which), ref.start_states(which)
    ysp, usp = ref.arrays(which)
    s = solver_factory(p, 3)
    for mode, sp in (("y", {"ysp": ysp}), ("u", {"usp": usp})):
        g = run_closed_loop(p, x0, x0, N, solver=s, fused=True, setpoints=sp)
        c = ref.c_reference(oracle_c, which, mode)
        print(f"LEVEL inst-setpoints {which} wave {mode} alone U: {np.abs(g['U'] - c['U']).max():.2e}")
        assert_same_closed_loop(g, c, p, TOL)
        shared = p.schedules(N)
        assert np.array_equal(g["YSP"], ysp if mode == "y" else np.repeat(shared["ysp"][:, None], ref.B, axis=1), equal_nan=True)
        assert np.array_equal(g["USP"], usp if mode == "u" else np.repeat(shared["usp"][:, None], ref.B, axis=1))
    pn = ref.problem(which, True)
    sn = solver_factory(pn, 3)
    g = run_closed_loop(pn, x0, x0, N, solver=sn, fused=True, noise_seed=lnr.SEED, setpoints={"ysp": ysp, "usp": usp})
    c = ref.c_reference(oracle_c, which, "yuvw")
    print(f"LEVEL inst-setpoints {which} wave with v and w U: {np.abs(g['U'] - c['U']).max():.2e}")
    assert_same_closed_loop(g, c, pn, TOL)


# ---- B. bit for bit, against code that exists without the feature -------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cstr_rss", "wb"])
@pytest.mark.parametrize("lk", LOOP_KERNELS)
def test_bit_for_bit_against_shared_schedule_runs(lk, which, solver_factory):
    p, x0 = ref.problem(which), ref.start_states(which)
    ysp, usp = ref.arrays(which)
    s = solver_factory(p, lk)
    L = [fused(s, x0, ref.shared_sched(which, j), set_sp=False) for j in range(3)]      # the plain shared-schedule runs of the whole batch on s_0, s_1, s_2
    # what B2 rests on: an instance's result does not depend on its neighbours - the plain run against the same run with the batch reversed
    perm = np.arange(ref.B)[::-1]
    rev = fused(s, x0[perm], ref.shared_sched(which, 0), set_sp=False)
    for k in FLOAT_LOGS + INT_LOGS:
        assert np.array_equal(rev[k], L[0][k][:, perm]), ("neighbour independence", k)
    # B1: arrays that repeat the shared schedule for every instance
    for j in (0, 2):
        y1, u1 = ref.schedule(which, j)
        rep = fused(s, x0, p.schedules(N), np.repeat(y1[:, None], ref.B, axis=1), np.repeat(u1[:, None], ref.B, axis=1))
        same_bits(rep, L[j], f"arrays repeating s_{j}")
    # B2: instance b of the per-instance run is instance b of the shared run on s_{b mod 3}
    one = fused(s, x0, p.schedules(N), ysp, usp)
    for k in FLOAT_LOGS + INT_LOGS:
        for j in range(3):
            assert np.array_equal(one[k][:, j::3], L[j][k][:, j::3]), ("B2", k, j)
    assert np.abs(L[0]["U"] - L[1]["U"]).max() > 1e-3      # (the schedules are felt)
    # B3: launch structure
    s.set_option("steps_per_launch", 5)
    same_bits(fused(s, x0, p.schedules(N), ysp, usp), one, "steps_per_launch = 5")      # launches of 5, 5 and 2 steps: the per-launch offset of both arrays
    s.set_option("steps_per_launch", 50)
    same_bits(fused(s, x0, p.schedules(N), ysp, usp, runs=((0, 7), (7, 5))), one, "two runs")
    if lk == 3:
        for ni in (1, 2, 4):      # 70 instances: whole waves of one and two, a last wave with two of four slots empty
            s.set_option("wave_instances", ni)
            same_bits(fused(s, x0, p.schedules(N), ysp, usp), one, f"wave_instances = {ni}")
        s.set_option("wave_instances", 0)
    # B4: set and cleared again, the next plain run is one on a handle that never saw per-instance set points
    fresh = fused(solver_factory(p, lk), x0, p.schedules(N), set_sp=False)
    s.loop_set_setpoints(ysp, usp)
    same_bits(fused(s, x0, p.schedules(N), None, None, alloc=False), fresh, "after (NULL, NULL)")
    s.loop_set_setpoints(ysp, usp)
    same_bits(fused(s, x0, p.schedules(N), alloc=False, set_sp=False), fresh, "after a new mpc_loop_set_schedule")      # (fused sets the schedule after this call)
    s.loop_set_setpoints(ysp, None)
    kept = fused(s, x0, p.schedules(N), alloc=False, set_sp=False)
    same_bits(kept, fresh, "ysp alone, then a new schedule")


# ---- C. fused against call-by-call on the lane loops without a C restatement ----------------------------------------------------------------------
def _fused_and_stepwise(p, which, x0p, x0m, n, s):
    from mpc_code_amd.driver import run_closed_loop
    ysp, usp = ref.arrays_for(p, which, len(x0p), n)
    f = run_closed_loop(p, x0p, x0m, n, solver=s, fused=True, setpoints={"ysp": ysp, "usp": usp})
    c = run_closed_loop(p, x0p, x0m, n, solver=s, fused=False, setpoints={"ysp": ysp, "usp": usp})
    q = run_closed_loop(p, x0p, x0m, n, solver=s, fused=True)
    assert np.abs(q["U"] - f["U"]).max() > 100 * np.abs(f["U"] - c["U"]).max()      # the set points are felt, far above what is compared
    # B1: arrays repeating the shared schedule give the plain run, to the bit
    sh = p.schedules(n)
    r = run_closed_loop(p, x0p, x0m, n, solver=s, fused=True, setpoints={"ysp": np.repeat(sh["ysp"][:n, None], len(x0p), axis=1), "usp": np.repeat(sh["usp"][:n, None], len(x0p), axis=1)})
    for k in FLOAT_LOGS + INT_LOGS:
        assert np.array_equal(r[k], q[k]), ("B1", k)
    return f, c


def test_soft_loop_fused_equals_the_three_calls(pkg):
    """loop_kernel_soft; inputs and tolerance of tests/test_lin_noise.py::test_soft_loop_fused_equals_the_three_calls"""
    from mpc_code_amd import capi
    soft = pkg.load_problem(pkg.example_path("cstr_lmpc_soft.py"), overrides={"Rss": np.diag([2.0, 1.0]).tolist()})
    rng = np.random.default_rng(5)
    B, ns = 70, 7
    x0 = np.vstack([soft.x0_p[None], soft.x0_p[None] + rng.uniform(-1.0, 1.0, size=(B - 1, soft.nxp))])
    s = capi.Solver(soft)
    try:
        s.set_option("steps_per_launch", 3)
        f, c = _fused_and_stepwise(soft, "cstr", x0, x0[:, :soft.nx], ns, s)
    finally:
        s.close()
    for k in ("STATUS_DYN", "STATUS_SS"):
        assert np.array_equal(f[k], c[k]), k
    for k in ("U", "X_HAT", "XS", "US", "Xp", "Yp", "D_HAT", "Sl"):
        print(f"LEVEL inst-setpoints soft fused vs call-by-call {k}: {np.abs(f[k] - c[k]).max():.2e}")
        assert np.abs(f[k] - c[k]).max() < 5e-6, (k, np.abs(f[k] - c[k]).max())


def test_model_parameter_loop_fused_equals_the_three_calls(pkg):
    """loop_kernel_pxy (def_px / def_py over the horizon); problem, starts and tolerance of tests/test_lin_noise.py::test_model_parameter_loop_fused_equals_the_three_calls"""
    from mpc_code_amd import capi
    p = _with_model_params(pkg, Rss=np.diag([2.0, 1.0]).tolist())
    assert p.has_model_params
    rng = np.random.default_rng(11)
    x0 = rng.uniform([-0.3, -4, -3], [0.3, 4, 3], size=(70, 3))
    s = capi.Solver(p)
    try:
        s.set_option("steps_per_launch", 3)
        f, c = _fused_and_stepwise(p, "cstr", x0, x0, 8, s)
    finally:
        s.close()
    for k in ("STATUS_DYN", "STATUS_SS"):
        assert np.array_equal(f[k], c[k]), k
    for k in ("U", "X_HAT", "XS", "US", "Xp", "Yp", "Y_HAT", "YS", "D_HAT"):
        print(f"LEVEL inst-setpoints pxy fused vs call-by-call {k}: {np.abs(f[k] - c[k]).max():.2e}")
        assert np.abs(f[k] - c[k]).max() < 1e-8, (k, np.abs(f[k] - c[k]).max())


# ---- D. errors ------------------------------------------------------------------------------------------------------------------------------------
def test_error_paths(solver_factory):
    from mpc_code_amd.capi import MpcAmdError, Solver
    which = "cstr_rss"
    p, x0 = ref.problem(which), ref.start_states(which)
    ysp, usp = ref.arrays(which)
    dp = ct.POINTER(ct.c_double)
    yp, up = ysp.ctypes.data_as(dp), usp.ctypes.data_as(dp)
    s = Solver(p)
    try:
        assert s.lib.mpc_loop_set_setpoints(s.h, N, yp, up) == -1 and b"mpc_loop_alloc" in s.lib.mpc_last_error()      # before mpc_loop_alloc
        s.loop_alloc(len(x0), N, 2)
        for bad_y, bad_u in ((ysp[:, :69], None), (ysp[..., :2], None), (None, usp[:, :, :1]), (ysp[0], None), (ysp, usp[:5])):
            with pytest.raises(ValueError, match="set points"):
                s.loop_set_setpoints(bad_y, bad_u)
        s.loop_set_state(x0, x0); s.loop_set_schedule(p.schedules(N))
        s.loop_set_setpoints(ysp[:8], usp[:8])
        with pytest.raises(MpcAmdError, match="set points"):      # the schedule has 12 steps, the arrays 8
            s.loop_run(0, 12)
        with pytest.raises(MpcAmdError, match="set points"):
            s.loop_run(6, 3)
        s.loop_run(0, 8); s.loop_sync()
        first = {k: s.loop_get_log(k)[:8] for k in FLOAT_LOGS + INT_LOGS}
        # nsteps of 0 and of max_steps + 1: -1, and what was in force stays - the same eight steps again, to the bit
        assert s.lib.mpc_loop_set_setpoints(s.h, 0, yp, up) == -1 and s.lib.mpc_loop_set_setpoints(s.h, N + 1, yp, None) == -1
        s.loop_set_state(x0, x0); s.loop_run(0, 8); s.loop_sync()
        for k in FLOAT_LOGS + INT_LOGS:
            assert np.array_equal(s.loop_get_log(k)[:8], first[k]), k
        # ... and they are the per-instance run's first eight steps
        whole = fused(solver_factory(p), x0, p.schedules(N), ysp, usp)
        for k in FLOAT_LOGS + INT_LOGS:
            assert np.array_equal(whole[k][:8], first[k]), k
        # a second mpc_loop_alloc clears them
        free = fused(s, x0, p.schedules(N), set_sp=False)
        same_bits(free, fused(solver_factory(p), x0, p.schedules(N), set_sp=False), "after a second mpc_loop_alloc")
    finally:
        s.close()
