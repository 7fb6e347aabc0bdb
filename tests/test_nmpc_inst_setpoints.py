"""Per-instance set-point schedules in the resident loops of the non-linear tracking path (nmpc_set_setpoints, nmpc_target_solve_inst)
on the kernels 1, 3 and 4: against the oracle run instance by instance with each instance's own schedule (tests/nmpc_inst_setpoints_ref.py, recorded in
tests/golden/nmpc_inst_setpoints.npz; tests/test_inst_setpoints_host.py recomputes instances of it without a GPU), bit for bit against shared-schedule runs,
launch structure, group offsets, the per-call seam, error paths.  B = 9 (two full waves of four and a lone slot, or four pairs and a lone slot), 10 steps,
real-time iteration; instance b tracks s_{b mod 3}.

TOL = 1e-6 relative: what tests/test_nmpc_state_noise.py uses for these models and kernels against the oracle."""
import numpy as np
import pytest

import nmpc_family as fam
import nmpc_inst_setpoints_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-6
STEPS = ref.STEPS
LOGS = ref.LOGS
ALL = ref.LOGS + ("STATUS_DYN", "STATUS_SS", "ITERS_DYN", "SQP_DYN", "SQP_SS")
KERNELS = [1, 3, 4]

_runs = {}


def run(case, kernel, sp="yu", shared=None, runs=((0, STEPS),), groups=None, nb=None, noisy=False):
    """one resident loop: shared schedule (the model's own, or s_`shared`), then per-instance set points (sp: "yu", "y", "u", "" none, or a pair of arrays)"""
    key = (case, kernel, sp, shared, runs, groups, nb, noisy) if isinstance(sp, str) else None      # (runs on arrays of the caller's are not kept)
    if key is None or key not in _runs:
        from mpc_code_amd import nmpc
        p, o, x0, xm = ref.problem(case, noisy)
        ysp, usp, v, w = ref.inputs(case, noisy) if nb is None else (ref.arrays(case, nb=nb) + (None, None))
        if nb is not None:
            x0, xm = np.resize(x0, (nb, x0.shape[1])), np.resize(xm, (nb, xm.shape[1]))      # the nine starts, over and over
        s = nmpc.NmpcSolver(p)
        try:
            s.set_kernel(kernel)
            if groups is not None:
                s.set_groups(groups)
            s.alloc(len(x0), STEPS)
            s.set_state(x0, xm)
            s.set_schedule(p.schedules(STEPS) if shared is None else ref.shared_sched(case, shared))
            s.set_noise(v, w)
            if not isinstance(sp, str):
                s.set_setpoints(*sp)
            elif sp:
                s.set_setpoints(ysp if "y" in sp else None, usp if "u" in sp else None)
            for k0, n in runs:
                s.run(k0, n, 1, 1e-9)
            s.sync()
            out = {k: s.get_log(k) for k in ALL}
        finally:
            s.close()
        if key is None:
            return out
        _runs[key] = out
    return _runs[key]


def same_bits(a, b, what):
    for k in ALL:
        assert np.array_equal(a[k], b[k]), (what, k)


# ---- A. against the oracle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case,noisy", [(c, n) for c, n in ref.GOLDEN_CASES])
def test_per_instance_loop_follows_the_oracle(case, noisy, kernel):
    """through the driver: cstr_nmpc (N = 30, the paired form), cl21 at N = 32 (paired) and 33 (four instances); cl21 at N = 32 also together with v and w"""
    from mpc_code_amd import nmpc
    p, o, x0, xm = ref.problem(case, noisy)
    ysp, usp, v, w = ref.inputs(case, noisy)
    s = nmpc.NmpcSolver(p)
    try:
        s.set_kernel(kernel)
        r = nmpc.run_nmpc_closed_loop(p, x0, xm, nsteps=STEPS, solver=s, max_sqp=1, noise_seed=ref.SEED if noisy else None, setpoints={"ysp": ysp, "usp": usp})
    finally:
        s.close()
    assert np.array_equal(r["YSP"], ysp, equal_nan=True) and np.array_equal(r["USP"], usp)
    if noisy:
        assert np.array_equal(r["V_WN"], v) and np.array_equal(r["W_WN"], w)
    g = ref.reference(case, noisy)
    for k in LOGS:
        print(f"LEVEL inst-setpoints nmpc {case}{' with v and w' if noisy else ''} kernel {kernel} {k}: {fam.rel_diff(r[k], g[k]):.2e}")
    assert np.array_equal(r["STATUS_DYN"], g["STATUS_DYN"]) and np.array_equal(r["STATUS_SS"], g["STATUS_SS"])
    for k in LOGS:
        assert fam.rel_diff(r[k], g[k]) < TOL, k
    if not noisy:
        same_bits(r, run(case, kernel), "the driver against the calls of the C-ABI")


# ---- B. bit for bit ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", ["cstr", "cl21_N33"])
def test_bit_for_bit_against_shared_schedule_runs(case, kernel):
    L = [run(case, kernel, sp="", shared=j) for j in range(3)]      # plain shared-schedule runs of the whole batch on s_0, s_1, s_2
    p, o, x0, xm = ref.problem(case)
    # B1: arrays that repeat the shared schedule for every instance
    for j in (1, 2):
        y1, u1 = ref.schedule(case, j)
        rep = run(case, kernel, sp=(np.repeat(y1[:, None], ref.B, axis=1), np.repeat(u1[:, None], ref.B, axis=1)))
        same_bits(rep, L[j], f"arrays repeating s_{j}")
    # B2: instance b of the per-instance run is instance b of the shared run on s_{b mod 3}
    one = run(case, kernel)
    for k in ALL:
        for j in range(3):
            assert np.array_equal(one[k][:, j::3], L[j][k][:, j::3]), ("B2", k, j)
    assert fam.rel_diff(L[0]["U"], L[1]["U"]) > 1e-3      # (the schedules are felt)
    same_bits(run(case, kernel, runs=((0, 4), (4, 6))), one, "two runs")      # the split pipeline's closing launch of the first call reads no set point
    # ysp alone leaves usp on the shared schedule, and the other way round
    same_bits(run(case, kernel, sp="y", shared=0), run(case, kernel, sp=(ref.arrays(case)[0], np.repeat(ref.schedule(case, 0)[1][:, None], ref.B, axis=1))), "ysp alone")
    same_bits(run(case, kernel, sp="u", shared=0), run(case, kernel, sp=(np.repeat(ref.schedule(case, 0)[0][:, None], ref.B, axis=1), ref.arrays(case)[1])), "usp alone")


def test_group_offsets_of_the_split_pipeline():
    """B = 130 on the split pipeline in two groups (128 and 2 instances): a set point indexed relative to the group would give instance 128 the row of instance 0"""
    case = "cl21_N32"
    L = [run(case, 4, sp="", shared=j, nb=130, groups=1) for j in range(3)]
    one = run(case, 4, nb=130, groups=2)
    for k in ALL:
        for j in range(3):
            assert np.array_equal(one[k][:, j::3], L[j][k][:, j::3]), ("B2 at 130 in two groups", k, j)
    same_bits(run(case, 4, nb=130, groups=1), one, "one group")


@pytest.mark.parametrize("case", ["cstr", "cl21_N32"])
def test_kernel_1_equals_the_call_by_call_loop_to_the_bit(case):
    """nmpc_ekf_update, nmpc_target_solve_inst, nmpc_ocp_solve with nmpc_plant_step in between"""
    from mpc_code_amd import nmpc
    p, o, x0, xm = ref.problem(case)
    ysp, usp = ref.arrays(case)
    st = nmpc.run_nmpc_stepwise(p, x0, xm, nsteps=STEPS, max_sqp=1, setpoints={"ysp": ysp, "usp": usp})
    r = run(case, 1)
    for k in ALL:
        assert np.array_equal(r[k], st[k]), k
    assert np.array_equal(st["YSP"], ysp, equal_nan=True)
    half = nmpc.run_nmpc_stepwise(p, x0, xm, nsteps=STEPS, max_sqp=1, setpoints={"usp": usp})      # ysp from the shared schedule, broadcast to the rows
    same = run(case, 1, sp="u")
    for k in ALL:
        assert np.array_equal(same[k], half[k]), k


@pytest.mark.parametrize("case", ["cstr", "cl21_N32", "cl21_N33"])
def test_kernel_4_agrees_with_kernel_3(case):
    """at the level the two have without the feature (4e-12)"""
    a, b = run(case, 3), run(case, 4)
    assert np.array_equal(a["STATUS_DYN"], b["STATUS_DYN"]) and np.array_equal(a["STATUS_SS"], b["STATUS_SS"])
    for k in LOGS:
        print(f"LEVEL inst-setpoints nmpc {case} kernel 4 against kernel 3 {k}: {fam.rel_diff(a[k], b[k]):.2e}")
        assert fam.rel_diff(a[k], b[k]) < 4e-12, k


# ---- C. errors --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_error_paths(kernel):
    import ctypes as ct
    from mpc_code_amd import nmpc
    from mpc_code_amd.capi import MpcAmdError
    case = "cl21_N32"
    p, o, x0, xm = ref.problem(case)
    ysp, usp = ref.arrays(case)
    dp = ct.POINTER(ct.c_double)
    yp, up = ysp.ctypes.data_as(dp), usp.ctypes.data_as(dp)
    s = nmpc.NmpcSolver(p)
    try:
        assert s.lib.nmpc_set_setpoints(s.h, STEPS, yp, up) == -1 and b"nmpc_alloc" in s.lib.nmpc_last_error()      # before nmpc_alloc
        s.set_kernel(kernel)
        s.alloc(ref.B, STEPS)
        for bad_y, bad_u in ((ysp[:, :8], None), (ysp[..., :1], None), (None, usp[:, :, :0]), (ysp[0], None), (ysp, usp[:5])):
            with pytest.raises(ValueError, match="set points"):
                s.set_setpoints(bad_y, bad_u)
        with pytest.raises(ValueError, match="per_instance"):
            s.target_solve(np.zeros((ref.B, max(p.nd, 1))), ysp[0, :5], usp[0], x0, np.zeros((ref.B, p.nu)), per_instance=True)
        s.set_state(x0, xm); s.set_schedule(p.schedules(STEPS))
        s.set_setpoints(ysp[:6], usp[:6])
        with pytest.raises(MpcAmdError, match="set points"):      # the schedule has 10 steps, the arrays 6
            s.run(0, STEPS, 1, 1e-9)
        with pytest.raises(MpcAmdError, match="set points"):
            s.run(4, 3, 1, 1e-9)
        # nsteps of 0 and of max_steps + 1: -1, and what was in force stays
        assert s.lib.nmpc_set_setpoints(s.h, 0, yp, up) == -1 and s.lib.nmpc_set_setpoints(s.h, STEPS + 1, yp, None) == -1
        s.run(0, 6, 1, 1e-9); s.sync()
        whole = run(case, kernel)
        for k in ALL:
            assert np.array_equal(s.get_log(k)[:6], whole[k][:6]), k
        # set_state does not touch them; a new schedule clears them; so does (None, None), and a second nmpc_alloc
        plain = run(case, kernel, sp="")
        s.set_state(x0, xm); s.run(0, 6, 1, 1e-9); s.sync()
        assert np.array_equal(s.get_log("U")[:6], whole["U"][:6])
        for clear in ("schedule", "none", "alloc"):
            s.set_setpoints(ysp, usp)
            if clear == "schedule":
                s.set_schedule(p.schedules(STEPS))
            elif clear == "none":
                s.set_setpoints(None, None)
            else:
                s.alloc(ref.B, STEPS); s.set_schedule(p.schedules(STEPS))
            s.set_state(x0, xm); s.run(0, STEPS, 1, 1e-9); s.sync()
            for k in ALL:
                assert np.array_equal(s.get_log(k), plain[k]), (clear, k)
    finally:
        s.close()
