"""The long-double restatement of the interior-point iteration (tests/wv_direction_ref.py) against the two double-precision
restatements, and the harness of tests/test_wv_directions.py proved on the C restatement's truncated solves: no GPU.

Over the whole grid of tests/test_wv_directions.py.  Measured (profiles/wv_direction_parity.txt): the float64 run of the restatement
differs from its long-double run by E64 = 7.6e-14 at the most (relative, iterates after 1..4 iterations; 1e-14 and less for every set
but the CSTR's), from ``rpdip_solve`` by 1.9e-13 and from the C restatement by 3.5e-13; the fit applied to the C restatement's
iterates leaves 4.7e-14.

CPU_TOL, the bound asserted on iterates and fit residuals, is not taken from those figures: an iterate after K = 4 iterations over
N <= 64 blocks of nv <= 10 variables is the end of a chain of at most K N nv dependent roundings, each eps = 2^-52 relative to the
largest entry; with a factor 4 for the two sweeps and the step that follow one another in an iteration that is
4 * 4 * 64 * 10 * 2.2e-16 = 2.3e-12.

The fitted step length is looser than the iterate it is fitted from: a_j = <W_j - R_{j-1}, d_j> / <d_j, d_j> moves by 1e-16 |W| / |d|
for a rounding of W_j, and by the fourth iteration the direction is small against the iterate (measured 6.1e-11, while the float64
run's own step length agrees with the long-double one to 3e-16).  The complementarity at R_j follows the fitted a_j one to one
(measured: half its deviation throughout), so both are held to ALPHA_CAP here, the most a step length may ever differ by; the bound
residual, (1 - a_j) times the one before, is held to CPU_TOL times the condition of the fit (wv_direction_ref.check_truncated).
"""
import copy

import numpy as np
import pytest

import riccati_np as rn
import wv_direction_ref as wd

CPU_TOL = 4 * wd.K_TRUNC * max(wd.HORIZONS) * 10 * wd.EPS64

SETS = [(d, f) for d in wd.VGPR_SETS + wd.BUILTIN_SETS for f in (True, False) if not (d[6] and f)]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float((np.abs(a - b).max(axis=1) / np.maximum(1.0, np.abs(b).max(axis=1))).max())


def _pack(p, z, u):
    B, N = z.shape[0], p.N
    out = np.zeros((B, (N + 1) * p.nx + N * p.nu))
    for k in range(N + 1):
        out[:, k * (p.nx + p.nu):k * (p.nx + p.nu) + p.nx] = z[:, k, :p.nx]
        if k < N:
            out[:, k * (p.nx + p.nu) + p.nx:(k + 1) * (p.nx + p.nu)] = u[:, k]
    return out


@pytest.mark.parametrize("dims,finite", SETS, ids=[wd.set_id(d) + ("-finite" if f else "-mixed") for d, f in SETS])
def test_float64_run_reproduces_both_restatements(dims, finite, oracle_c):
    worst = dict(e64=0.0, np=0.0, c=0.0)
    for N in wd.HORIZONS:
        p = wd.direction_problem(dims, N, finite)
        inp = wd.direction_inputs(p, wd.BATCH, wd.case_seed(dims, N, finite))
        ld = wd.reference_iterations(p, *inp, wd.K_TRUNC, dtype=np.longdouble)
        f64 = wd.reference_iterations(p, *inp, wd.K_TRUNC, dtype=np.float64)
        sd = rn.stage_data(p); inst = rn.instance_data(p, sd, *inp)
        for k in range(1, wd.K_TRUNC + 1):
            assert ld[k - 1]["active"].all() and f64[k - 1]["active"].all(), (dims, N, k)
            worst["e64"] = max(worst["e64"], _rel(f64[k - 1]["W"], ld[k - 1]["W"]))
            r = rn.rpdip_solve(sd, inst, max_iter=k)
            assert (r["status"] == 1).all() and (r["iters"] == k).all(), (dims, N, k, r["status"])
            worst["np"] = max(worst["np"], _rel(_pack(p, r["z"], r["u"]), f64[k - 1]["W"]))
            q = copy.copy(p); q.max_iter = k
            c = oracle_c.OracleC(q).ocp_solve(*inp, want_w=True)
            assert (c["status"] == 1).all() and (c["iters"] == k).all(), (dims, N, k, c["status"])
            worst["c"] = max(worst["c"], _rel(c["w"], f64[k - 1]["W"]))
            # the residuals the solvers report at an unconverged iterate: bound residual and complementarity (the stationarity entry is stale)
            rec = f64[k - 1]
            assert (np.abs(r["res"][:, 1] - rec["res_p"]) <= wd.ALPHA_CAP * rec["res_p_size"] + rec["res_floor"]).all(), (dims, N, k)
            assert (np.abs(r["res"][:, 2] - rec["mu"]) <= wd.ALPHA_CAP * rec["mu_size"]).all(), (dims, N, k)
    print(f"{wd.set_id(dims)} finite={finite}: E64 = {worst['e64']:.2e}, against rpdip_solve {worst['np']:.2e}, against the C restatement {worst['c']:.2e}")
    assert worst["e64"] <= CPU_TOL and worst["np"] <= CPU_TOL and worst["c"] <= CPU_TOL, worst


@pytest.mark.parametrize("dims,finite", SETS, ids=[wd.set_id(d) + ("-finite" if f else "-mixed") for d, f in SETS])
def test_fit_on_the_c_restatement_returns_the_reference_step(dims, finite, oracle_c):
    worst = dict(resid=0.0, dalpha=0.0, dres_p=0.0, dmu=0.0)      # dres_p: over max(1, acond), the condition of the fitted step length
    for N in wd.HORIZONS:
        p = wd.direction_problem(dims, N, finite)
        inp = wd.direction_inputs(p, wd.BATCH, wd.case_seed(dims, N, finite))

        def solve_j(j):
            q = copy.copy(p); q.max_iter = j
            return oracle_c.OracleC(q).ocp_solve(*inp, want_w=True)
        fig = wd.check_truncated(p, inp, solve_j)
        for j, f in enumerate(fig, 1):
            assert f["limit"].all() and f["ref_active"].all(), (dims, N, j)
            f["dres_p"] = f["dres_p"] / np.maximum(1.0, f["acond"])
            for k in worst:
                worst[k] = max(worst[k], float(f[k].max()))
        assert fig[-1]["ref_active_after"].all(), (dims, N)
    print(f"{wd.set_id(dims)} finite={finite}: " + ", ".join(f"{k} = {v:.2e}" for k, v in worst.items()))
    assert worst["resid"] <= CPU_TOL and worst["dres_p"] <= CPU_TOL, worst
    assert worst["dalpha"] <= wd.ALPHA_CAP and worst["dmu"] <= wd.ALPHA_CAP, worst


def test_given_step_lengths_replace_the_reference_own():
    dims = (3, 2, 3, 3, 3, 0, 0)
    p = wd.direction_problem(dims, 5, True)
    inp = wd.direction_inputs(p, 3, 1)
    own = wd.reference_iterations(p, *inp, 3)
    half = [0.5 * own[0]["alpha_ref"]]
    g = wd.reference_iterations(p, *inp, 3, alphas=half)
    assert np.array_equal(g[0]["alpha"], half[0]) and np.array_equal(g[0]["alpha_ref"], own[0]["alpha_ref"])
    assert np.array_equal(g[0]["W"], own[0]["R"] + half[0][:, None] * own[0]["d"])
    assert np.array_equal(g[1]["R"], g[0]["W"]) and np.array_equal(g[1]["alpha"], g[1]["alpha_ref"])      # from the second step on its own again
    assert not np.array_equal(g[1]["W"], own[1]["W"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the harness fails on a wrong direction: the three edits of the sweeps, restated in the float64 run (DirectionRef(edit=...))
# ---------------------------------------------------------------------------------------------------------------------------------
EDIT_SETS = [(d, f) for d in ((3, 2, 3, 3, 3, 0, 0), (4, 2, 2, 2, 4, 0, 0)) for f in (True, False)]
TOUCHED = {1: lambda N: True, 2: lambda N: N % 4 != 0, 3: lambda N: N >= 4}


@pytest.mark.parametrize("edit", (1, 2, 3))
@pytest.mark.parametrize("dims,finite", EDIT_SETS, ids=[wd.set_id(d) + ("-finite" if f else "-mixed") for d, f in EDIT_SETS])
def test_fit_residual_shows_an_edited_sweep(dims, finite, edit):
    """A factor 1 + 1e-9 on K, the neighbour's h_z in the remainder blocks of the corrector's backward sweep, a factor 1 + 1e-9 on the
    stored du of one block in four: at every horizon an edit touches the fit leaves at least 7e-11 (ten times TOL_DIR and more) within four
    iterations (measured 7.2e-11 at the least, profiles/wv_direction_parity.txt), at the others no more than TOL_DIR."""
    row = []
    for N in wd.HORIZONS:
        p = wd.direction_problem(dims, N, finite)
        inp = wd.direction_inputs(p, wd.BATCH, wd.case_seed(dims, N, finite))
        m = wd.DirectionRef(p, *inp, dtype=np.float64, edit=edit)
        its = []
        for j in range(1, wd.K_TRUNC + 1):
            m.direction(); m.advance()
            rp, mu = m.residuals()
            its.append(dict(w=m.w().copy(), status=np.ones(wd.BATCH, int), iters=np.full(wd.BATCH, j), res=np.stack([0.0 * rp, rp, mu], axis=1)))
        left = max(float(f["resid"].max()) for f in wd.check_truncated(p, inp, lambda j: its[j - 1]))
        row.append((N, TOUCHED[edit](N), left))
    print(f"edit {edit} {wd.set_id(dims)} finite={finite}: " + " ".join(f"N{N}{'*' if t else ''}={v:.1e}" for N, t, v in row))
    for N, t, v in row:
        assert (v >= 7e-11 and v >= 10.0 * wd.TOL_DIR) if t else (v <= wd.TOL_DIR), (edit, N, t, v)


def test_build_lists_and_problem_draws_stay_in_step():
    import __graft_entry__ as g
    from mpc_code_amd import capi
    import test_gpu_fuzz
    assert list(g.WV_VGPR_FORM_SETS) == wd.VGPR_SETS and wd.GENERIC_TILES == (capi.WV_GENERIC_TILES_FLAG,)
    built = {(3, 2, 3, 3, 3, 0, 0), (4, 2, 2, 2, 4, 1, 0), (3, 2, 2, 2, 3, 1, 0), (2, 1, 1, 1, 2, 0, 0), (2, 1, 1, 1, 2, 1, 0), (2, 1, 1, 1, 2, 0, 1),      # the default library
             (5, 2, 2, 2, 5, 0, 0)} | set(g.WV_DIRECTION_EXTRA_SETS)
    assert set(wd.VGPR_SETS + wd.BUILTIN_SETS) <= built
    for seed, nx, nu, ny, du in ((101, 3, 2, 3, False), (301, 2, 1, 1, True)):
        a = test_gpu_fuzz.random_problem(seed, nx, nu, ny, du)
        b = wd.direction_problem((nx, nu, ny, ny, nx, int(du), 0), a.N, None, seed=seed)
        for k in ("A", "B", "Bd", "Q", "R", "P", "umin", "umax", "xmin", "xmax", "ymin", "ymax", "K"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert a.DUForm == b.DUForm and a.y_bounded == b.y_bounded
