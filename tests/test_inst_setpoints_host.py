"""Per-instance set-point schedules, the parts that need no GPU: the yardsticks the GPU tests compare with (tests/inst_setpoints_ref.py,
tests/nmpc_inst_setpoints_ref.py) against each other and against their recorded runs, that the inputs discriminate, the Python plumbing on stub solvers,
and the headers against the bindings' lists."""
import os
import re

import numpy as np
import pytest

import inst_setpoints_ref as ref
import nmpc_family as fam
import nmpc_inst_setpoints_ref as nref
from conftest import ROOT

TOL = 1e-7      # the tolerance of the GPU tests against the C restatement (tests/test_lin_noise.py, tests/test_inst_setpoints.py)
N = ref.NSTEPS


# ---- 1. the two linear yardsticks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cstr", "wb", "cstr_rss"])
def test_c_restatement_instance_by_instance_against_the_numpy_restatement(which, oracle_c):
    """the C restatement, one instance at a time with its own schedule, against the NumPy restatement, which takes [B, .] rows for the whole batch at once:
    equal status words, every log within the tolerance tests/test_lin_noise_host.py has for this pair"""
    p, x0 = ref.problem(which), ref.start_states(which)
    ysp, usp = ref.arrays(which)
    c = ref.c_reference(oracle_c, which)
    r = ref.np_loop(p, N, x0, x0, ysp, usp)
    assert np.array_equal(c["STATUS_DYN"], r["STATUS_DYN"]) and np.array_equal(c["STATUS_SS"], r["STATUS_SS"])
    for k in ("U", "XS", "US", "YS", "X_HAT", "Xp", "D_HAT"):
        d = np.abs(c[k] - r[k]).max()
        print(which, k, d)
        assert d < TOL, (k, d)
    # a set point enters the target's cost alone: every target is solved, and in s_2's stretch far outside the bounds it rides a bound of the target problem
    assert (c["STATUS_SS"] == 0).all()
    far = np.concatenate([c["XS"][5:8, 2::3], c["US"][5:8, 2::3]], axis=2)
    lo, hi = np.concatenate([np.ravel(p.xmin_ss), np.ravel(p.umin_ss)]), np.concatenate([np.ravel(p.xmax_ss), np.ravel(p.umax_ss)])
    assert (np.minimum(np.abs(far - lo), np.abs(far - hi)).min(axis=2) < 1e-6).all()


@pytest.mark.parametrize("which", ["cstr", "wb", "cstr_rss"])
def test_the_inputs_discriminate(which, oracle_c):
    """in the yardstick: rows swapped between two instances, one instance's changes a step late, usp replaced by zeros (where the target reads it) - each moves
    U by at least 100 tolerances of the GPU test"""
    p, x0 = ref.problem(which), ref.start_states(which)
    ysp, usp = ref.arrays(which)
    sel = [0, 1, 2, 3]
    base = ref.c_loops(oracle_c, p, N, x0[sel], x0[sel], ysp[:, sel], usp[:, sel])
    full = ref.c_reference(oracle_c, which)
    assert all(np.array_equal(base[k], full[k][:, sel]) for k in base)      # (an instance's loop does not depend on the batch it is computed in)
    sw = [1, 0, 2, 3]
    swapped = ref.c_loops(oracle_c, p, N, x0[sel], x0[sel], ysp[:, sw], usp[:, sw])
    moved = np.abs(swapped["U"] - base["U"]).max(axis=(0, 2))
    print(which, "rows of instances 0 and 1 swapped move U by", moved)
    assert moved[:2].min() >= 100 * TOL and moved[2:].max() == 0.0
    late_y, late_u = np.array(ysp[:, sel]), np.array(usp[:, sel])
    late_y[:, 1], late_u[:, 1] = ref.schedule(which, 1, shift=1)
    late = ref.c_loops(oracle_c, p, N, x0[sel], x0[sel], late_y, late_u)
    moved = np.abs(late["U"] - base["U"]).max(axis=(0, 2))
    print(which, "instance 1 one step late moves U by", moved)
    assert moved[1] >= 100 * TOL and moved[[0, 2, 3]].max() == 0.0
    assert np.array_equal(late["U"][:2], base["U"][:2]) and np.abs(late["U"][2, 1] - base["U"][2, 1]).max() >= 100 * TOL      # ... from the step of the change on
    zero = ref.c_loops(oracle_c, p, N, x0[sel], x0[sel], ysp[:, sel], np.zeros_like(usp[:, sel]))
    moved = np.abs(zero["U"] - base["U"]).max(axis=(0, 2))
    print(which, "usp = 0 moves U by", moved)
    if which == "cstr_rss":
        assert moved.min() >= 100 * TOL
    else:      # Rss = 0: the target does not read usp
        assert moved.max() == 0.0


# ---- the non-linear yardstick --------------------------------------------------------------------------------------------------------------------
def test_recorded_oracle_runs_are_the_oracles(pkg):
    """tests/golden/nmpc_inst_setpoints.npz: its inputs are the ones the tests build, and instances of cl21 recomputed here give the recorded rows to the bit;
    every target solved; the schedules are felt"""
    with np.load(nref.GOLDEN) as g:
        for case, noisy in nref.GOLDEN_CASES:
            ysp, usp, v, w = nref.inputs(case, noisy)
            assert np.array_equal(g[nref.golden_key(case, noisy, "ysp")], ysp, equal_nan=True) and np.array_equal(g[nref.golden_key(case, noisy, "usp")], usp)
            r = nref.reference(case, noisy)
            assert (r["STATUS_SS"] == 0).all()
            assert fam.rel_diff(r["U"][:, 0], r["U"][:, 3]) > 100 * 1e-6 and fam.rel_diff(r["U"][:, 0], r["U"][:, 1]) > 100 * 1e-6
    sel = [1, 5]
    again = nref.oracle_run("cl21_N33", False, instances=sel)
    rec = nref.reference("cl21_N33", False)
    for k in nref.LOGS + nref.ILOGS:
        assert np.array_equal(again[k], rec[k][:, sel]), k
    # the closure: the oracle problem's schedules are that instance's rows
    p, o, x0, xm = nref.problem("cl21_N33")
    ysp, usp = nref.arrays("cl21_N33")
    s = nref.with_setpoints(o, ysp[:, 4], usp[:, 4]).schedules(nref.STEPS)
    assert np.array_equal(s["ysp"], ysp[:, 4]) and np.array_equal(s["usp"], usp[:, 4]) and np.array_equal(s["pxp"], o.schedules(nref.STEPS)["pxp"])


# ---- 3. Python plumbing without a device ----------------------------------------------------------------------------------------------------------
def test_setpoint_dicts_are_checked(pkg):
    from mpc_code_amd.capi import check_setpoints, tracked_setpoints
    y, u = np.zeros((5, 7, 3)), np.ones((5, 7, 2))
    assert check_setpoints(None, 5, 7, 3, 2) == (None, None)
    a, b = check_setpoints({"ysp": y, "usp": u}, 5, 7, 3, 2)
    assert a.shape == y.shape and b.shape == u.shape and check_setpoints({"usp": u}, 5, 7, 3, 2)[0] is None
    for bad in ({"ysp": y[:4]}, {"ysp": y[:, :6]}, {"ysp": y[..., :2]}, {"usp": y}, {"ysp": y[0]}, {"ysp": y, "xsp": y}, {}, {"ysp": None}, [y, u]):
        with pytest.raises(ValueError, match="setpoints"):
            check_setpoints(bad, 5, 7, 3, 2)
    with pytest.raises(ValueError, match=r"\[5, 7, 3\] expected, got \(4, 7, 3\)"):
        check_setpoints({"ysp": y[:4]}, 5, 7, 3, 2)
    sched = {"ysp": np.arange(18.0).reshape(6, 3), "usp": np.arange(12.0).reshape(6, 2)}
    t = tracked_setpoints(sched, None, u, 5, 7)
    assert t["USP"] is u and t["YSP"].shape == (5, 7, 3) and np.array_equal(t["YSP"][:, 4], sched["ysp"][:5])


class _StubLinearSolver:
    """what driver.run_closed_loop asks of capi.Solver in its fused mode, recording the calls"""

    def __init__(self, p):
        self.p, self.calls, self.fused_plant = p, [], True

    def loop_alloc(self, B, n, level):
        self.B, self.n = B, n
        self.calls.append("alloc")

    def loop_set_state(self, *a):
        self.calls.append("state")

    def loop_set_schedule(self, sched):
        self.calls.append("schedule")

    def loop_set_model_schedule(self, px, py):
        pass

    def loop_set_noise(self, v, w):
        self.calls.append(("noise", v is not None, w is not None))

    def loop_set_setpoints(self, ysp, usp):
        self.calls.append(("setpoints", None if ysp is None else np.array(ysp), None if usp is None else np.array(usp)))

    def loop_run(self, k0, n):
        self.calls.append("run")
        if getattr(self, "fail", False):
            raise RuntimeError("launch failed")

    def loop_sync(self):
        pass

    def loop_get_log(self, name):
        p = self.p
        d = dict(U=p.nu, X_HAT=p.nx, XS=p.nx, US=p.nu, YS=p.ny, Xp=p.nxp, D_HAT=p.nd)
        return np.zeros((self.n, self.B, d[name])) if name in d else np.zeros((self.n, self.B), np.int32)

    def last_kernel_ms(self):
        return 1.0, 1


def test_linear_driver_hands_the_arrays_on_and_clears_them(cstr):
    from mpc_code_amd.driver import run_closed_loop
    B, n = 5, 6
    x0 = np.zeros((B, 3))
    ysp = np.random.default_rng(0).normal(size=(n, B, 3)); usp = np.random.default_rng(1).normal(size=(n, B, 2))
    s = _StubLinearSolver(cstr)
    out = run_closed_loop(cstr, x0, x0, n, solver=s, setpoints={"ysp": ysp})
    sp = [c for c in s.calls if isinstance(c, tuple) and c[0] == "setpoints"]
    assert len(sp) == 2 and np.array_equal(sp[0][1], ysp) and sp[0][2] is None and sp[1][1] is None and sp[1][2] is None      # set, then cleared in the finally
    assert s.calls.index("schedule") < s.calls.index(sp[0]) < s.calls.index("run")      # after the schedule, which clears them
    assert np.array_equal(out["YSP"], ysp) and np.array_equal(out["USP"], np.repeat(cstr.schedules(n)["usp"][:, None], B, axis=1))
    s = _StubLinearSolver(cstr); s.fail = True      # ... also after an exception
    with pytest.raises(RuntimeError):
        run_closed_loop(cstr, x0, x0, n, solver=s, setpoints={"ysp": ysp, "usp": usp})
    assert s.calls[-1][0] == "setpoints" and s.calls[-1][1] is None and s.calls[-1][2] is None
    s = _StubLinearSolver(cstr)      # without setpoints= nothing is set or cleared, and the result still says what was tracked
    out = run_closed_loop(cstr, x0, x0, n, solver=s)
    assert not [c for c in s.calls if isinstance(c, tuple) and c[0] == "setpoints"] and out["YSP"].shape == (n, B, 3)
    for bad in ({"ysp": ysp[:, :4]}, {"usp": ysp}, {"ysp": ysp[:5]}):
        s = _StubLinearSolver(cstr)
        with pytest.raises(ValueError, match="setpoints"):
            run_closed_loop(cstr, x0, x0, n, solver=s, setpoints=bad)
        assert "run" not in s.calls


def test_linear_call_by_call_mode_gets_the_rows_step_by_step(cstr):
    """driver._stepwise hands sched["ysp"][k] to mpc_target_solve: [B, ny] rows of step k where the shared schedule has one row"""
    from mpc_code_amd import driver
    B, n = 4, 3
    ysp = np.random.default_rng(0).normal(size=(n, B, 3)); usp = np.random.default_rng(1).normal(size=(n, B, 2))
    seen = []

    class Stub:
        def set_option(self, *a):
            pass

        def kf_update(self, y, xi, P):
            return xi, P

        def target_solve(self, usp_k, ysp_k, xsp_k, dhat, us_prev):
            seen.append((np.array(usp_k), np.array(ysp_k)))
            return dict(xs=np.zeros((B, 3)), us=np.zeros((B, 2)), ys=np.zeros((B, 3)), status=np.zeros(B, np.int32), iters=np.zeros(B, np.int32))

        def ocp_solve(self, xhat, xs, us, dhat, u, px=None, py=None):
            return dict(u0=np.zeros((B, 2)), x1=np.zeros((B, 3)), status=np.zeros(B, np.int32), iters=np.zeros(B, np.int32))

    out = driver.run_closed_loop(cstr, np.zeros((B, 3)), np.zeros((B, 3)), n, solver=Stub(), fused=False, setpoints={"ysp": ysp, "usp": usp})
    assert len(seen) == n and all(np.array_equal(seen[k][0], usp[k]) and np.array_equal(seen[k][1], ysp[k]) for k in range(n))
    assert np.array_equal(out["YSP"], ysp) and np.array_equal(out["USP"], usp)


def test_nonlinear_drivers_hand_the_arrays_on(pkg):
    from mpc_code_amd import nmpc
    p = pkg.load_problem(pkg.example_path("cstr_nmpc.py"))
    B, n = 3, 4
    x0 = np.tile(p.x0_p, (B, 1))
    ysp = np.random.default_rng(0).normal(size=(n, B, p.ny)); usp = np.random.default_rng(1).normal(size=(n, B, p.nu))
    calls = []

    class Stub:
        LOGS, ILOGS = nmpc.NmpcSolver.LOGS, nmpc.NmpcSolver.ILOGS

        def alloc(self, B_, n_):
            self.B, self.n = B_, n_

        def set_state(self, *a):
            pass

        def set_schedule(self, s):
            calls.append("schedule")

        def set_noise(self, *a):
            pass

        def set_setpoints(self, y, u):
            calls.append(("setpoints", y, u))

        def run(self, *a):
            calls.append("run")

        def sync(self):
            pass

        def get_log(self, k):
            return np.zeros((self.n, self.B, getattr(p, self.LOGS[k]))) + (p.x0_p if k in ("Xp", "X_HAT", "XS") else 0.0) if k in self.LOGS else np.zeros((self.n, self.B), np.int32)

        def last_kernel_ms(self):
            return 1.0

        # the per-call seam
        def ekf_update(self, y, u, xhat, dhat, P):
            return xhat, dhat, P

        def target_solve(self, dhat, ysp_k, usp_k, xs, us, per_instance=False):
            calls.append(("target", np.array(ysp_k), np.array(usp_k), per_instance))
            return xs, us, np.zeros(B, np.int32), np.zeros(B, np.int32)

        def ocp_solve(self, xhat, dhat, xs, us, u, max_sqp, tol):
            return u, xhat, np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)

        def plant_step(self, u, x, pxp):
            return x

    out = nmpc.run_nmpc_closed_loop(p, x0, x0, nsteps=n, solver=Stub(), setpoints={"usp": usp})
    assert calls[0] == "schedule" and calls[1][0] == "setpoints" and calls[1][1] is None and np.array_equal(calls[1][2], usp) and calls[2] == "run"
    assert calls[3][0] == "setpoints" and calls[3][1] is None and calls[3][2] is None      # cleared in the finally
    assert np.array_equal(out["USP"], usp) and np.array_equal(out["YSP"], np.repeat(p.schedules(n)["ysp"][:, None], B, axis=1))
    with pytest.raises(ValueError, match="setpoints"):
        nmpc.run_nmpc_closed_loop(p, x0, x0, nsteps=n, solver=Stub(), setpoints={"ysp": ysp[:, :2]})
    del calls[:]
    out = nmpc.run_nmpc_stepwise(p, x0, x0, nsteps=n, solver=Stub(), setpoints={"ysp": ysp})
    tg = [c for c in calls if c[0] == "target"]
    assert len(tg) == n and all(c[3] for c in tg) and all(np.array_equal(tg[k][1], ysp[k]) for k in range(n))
    assert all(np.array_equal(tg[k][2], np.tile(p.schedules(n)["usp"][k], (B, 1))) for k in range(n))      # the shared row, broadcast to the instances
    assert np.array_equal(out["YSP"], ysp)
    del calls[:]
    nmpc.run_nmpc_stepwise(p, x0, x0, nsteps=n, solver=Stub())
    assert not any(c[3] for c in calls if c[0] == "target")      # without setpoints=: the shared call, as before


def test_economic_path_refuses_setpoints(pkg):
    p = pkg.load_problem(pkg.example_path("reactor_enmpc.py"))
    with pytest.raises(ValueError, match="economic path has no set points"):
        pkg.run_example(p, x0_p=p.x0_p[None], nsteps=2, setpoints={"ysp": np.zeros((2, 1, p.ny))})


def test_run_exfile_checks_the_file_against_batch_and_steps(pkg, tmp_path, capsys):
    import run_exfile
    ex = pkg.example_path("cstr_lmpc.py")
    good, bad = str(tmp_path / "good.npz"), str(tmp_path / "bad.npz")
    np.savez(good, ysp=np.zeros((6, 4, 3)), usp=np.zeros((6, 4, 2)))
    np.savez(bad, ysp=np.zeros((6, 5, 3)))
    assert run_exfile.main([ex, "--batch", "4", "--nsteps", "6", "--setpoints", good, "--load-only"]) == 0
    assert "set points per instance" in capsys.readouterr().out
    for args in (["--batch", "4", "--nsteps", "6", "--setpoints", bad], ["--batch", "4", "--nsteps", "7", "--setpoints", good], ["--batch", "3", "--nsteps", "6", "--setpoints", good]):
        with pytest.raises(SystemExit, match="expected, got"):
            run_exfile.main([ex] + args + ["--load-only"])
    with pytest.raises(SystemExit, match="economic path"):
        run_exfile.main([pkg.example_path("reactor_enmpc.py"), "--setpoints", good, "--load-only"])


def test_plot_draws_the_instances_own_set_point(tmp_path, monkeypatch):
    from mpc_code_amd import plots
    n, B = 6, 3
    rng = np.random.default_rng(0)
    out = {"U": rng.normal(size=(n, B, 1)), "Yp": rng.normal(size=(n, B, 2)), "YS": rng.normal(size=(n, B, 2)), "YSP": rng.normal(size=(n, B, 2))}
    drawn = []
    monkeypatch.setattr(plots, "_figure", lambda plt, t, series, label, k, path, *a: drawn.append((label, k, [np.array(s) for s in series])) or f"{label}{k}")
    plots.make_plots(out, 1.0, str(tmp_path), instance=2, ysp=out["YSP"][:, 2])
    outputs = [d for d in drawn if d[0] == "Output "]
    assert len(outputs) == 2
    for label, k, series in outputs:
        assert len(series) == 3 and np.array_equal(series[0], out["Yp"][:, 2, k]) and np.array_equal(series[2], out["YSP"][:, 2, k])
    del drawn[:]
    plots.make_plots(out, 1.0, str(tmp_path), instance=2)
    assert all(len(series) == 2 for label, k, series in drawn if label == "Output ")


# ---- 4. headers and bindings ------------------------------------------------------------------------------------------------------------------------
def test_headers_declare_what_the_bindings_list():
    from mpc_code_amd import capi, nmpc
    lin = open(os.path.join(ROOT, "include", "mpc_amd.h")).read()
    nl = open(os.path.join(ROOT, "include", "mpc_nmpc.h")).read()
    assert set(re.findall(r"\b(nmpc_[a-z_]+)\s*\(", nl)) == set(nmpc.NMPC_EXPORTS)
    for name, hdr, names in (("mpc_loop_set_setpoints", lin, capi.EXPORTS), ("nmpc_set_setpoints", nl, nmpc.NMPC_EXPORTS), ("nmpc_target_solve_inst", nl, nmpc.NMPC_EXPORTS)):
        assert re.search(r"\bint " + name + r"\s*\(", hdr) and name in names, name
    assert "B instances that share the problem and the schedules and differ\n * in their state.  Step order" not in lin      # the sentence that said so
    assert hasattr(capi.Solver, "loop_set_setpoints") and hasattr(nmpc.NmpcSolver, "set_setpoints")
