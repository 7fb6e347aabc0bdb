"""Newton directions of the OCP solvers against the long-double restatement (tests/wv_direction_ref.py), by truncated solves.

A solve with ``max_iter = j`` that stops at the iteration limit returns the iterate after exactly j iterations.  Per case, for
j = 1..4: every instance stops at the limit (in the solver and in the reference); per instance the step length a_j is fitted,
``W_j = R_{j-1} + a_j d_j`` with the reference advanced by the fitted a_1 .. a_{j-1}; what the fit leaves is the error of the
direction (TOL_DIR), a_j is the reference's own step length up to TOL_ALPHA, and the bound residual and the complementarity the
call reports are the reference's at R_j.  The wave solver (``ocp_kernel`` 3: matrix-core tile sweeps, in VGPR form for stage states
<= 4 without cross term, in builtin form else) and the lane solver (1: plain C++ recursions, the yardstick) go through the same
harness.  A converged answer forgives a direction that is wrong in the ninth digit; these iterates do not.

Grid: six dimension sets on the VGPR-form path (stage states 1, 2, 3 with a general output row, 3, 4, 4), five on the builtin path
(one tile with cross term, 2 x 2 tiles up to stage state 8), horizons 2..7 (fewer blocks than a group of the sweeps, then every
remainder of both group sizes), 33 and 64, each with every bound finite (kernels without bound masks) and with some state bounds
infinite; seven instances (one full wave and one with a dead tile), and one instance once per kernel variant.

Measured over the whole grid (profiles/wv_direction_parity.txt, per dimension set):
    E64     float64 run of the restatement against its long-double run (CPU)            7.6e-14
    E_lane  fit residual of the lane solver on an MI355X                                4.16e-14
    E_wave  fit residual of the wave solver on an MI355X                                3.75e-14
    step length |a_j - alpha_ref_j| / alpha_ref_j, either solver                        4.48e-8   (the approximate reciprocal)
    reported bound residual / complementarity against the reference at R_j              3.94e-14 / 3.12e-11
TOL_DIR = 4 E_wave = 1.5e-13 (under 1e-10), TOL_ALPHA = 4 x 4.48e-8 = 1.8e-7 (under 1e-6).  The three edits of the sweeps (a factor
1 + 1e-9 on K, the neighbour's h_z in the remainder blocks of the corrector's backward sweep, a factor 1 + 1e-9 on the stored du of
the last block of a group), restated in the float64 run of the reference, leave 7.2e-11 at the least at every horizon they touch
(asserted in tests/test_wv_direction_ref.py): 480 times TOL_DIR.  The same edits applied to a scratch copy of csrc/mpc_wave.hpp, the
3_2_3_3_3_0_0 and 4_2_2_2_4_0_0 libraries rebuilt from it: this module fails at every horizon an edit touches and passes at the others
(edit 1: 18 of 18 cases per set; edits 2 and 3: 14 of 18, the four that pass being N = 4, 64 and N = 2, 3); the smallest fit residual an
edit leaves is 1.18e-10 (edit 3, N = 6), 790 times TOL_DIR; per horizon in the profile.

The bound residual after a step is (1 - a_j) times the one before it, and slacks and multipliers of the reference advance with the
fitted a_j, which a rounding of W_j moves by acond = sqrt(nw) |W| / (|d| a_j) roundings (printed; up to 2e7 by the fourth
iteration).  Relative to their own values nothing tight can be said of the two (the C restatement, whose truncated solves leave a
fit residual of 4.7e-14, was off by 3e-8 and 4e-10 on them on an earlier draw of these problems), so they are compared relative to the size of the terms they are made of
(wv_direction_ref.DirectionRef.advance), not to their own size, at four times the largest figure measured for either solver:
TOL_RES_P = 1.6e-13, TOL_MU = 1.25e-10.  The bound residual has the rounding floor 8 eps64 (|v| + |s| + |bound|) of its own
evaluation taken off first.  In every set but the CSTR's the cold start leaves no bound residual at all (slack = distance to the
bound), res_p stays a rounding and the printed dres_p = 0.00e+00 says no more than |res[:, 1] - res_p| <= 8 eps64 scale: it is not a
relative agreement.

The second half compares the VGPR form of the sweeps with their builtin form bit for bit: the same library built with
-DMPC_WV_GENERIC_TILES, which takes every stage through the generic path.
"""
import copy
import os

import numpy as np
import pytest

import wv_direction_ref as wd

pytestmark = pytest.mark.gpu

TOL_DIR = wd.TOL_DIR
TOL_ALPHA = wd.TOL_ALPHA
TOL_RES_P = 4 * 3.94e-14
TOL_MU = 4 * 3.12e-11
assert TOL_DIR <= 1e-10 and TOL_DIR <= 7.2e-11 / 10 and TOL_ALPHA <= wd.ALPHA_CAP

SOLVERS = {"wave": 3, "lane": 1}
SETS = [(d, f) for d in wd.VGPR_SETS + wd.BUILTIN_SETS for f in (True, False) if not (d[6] and f)]
CASES = [(d, f, N, wd.BATCH) for d, f in SETS for N in wd.HORIZONS] + [(d, f, 6, 1) for d, f in SETS]


def _case_id(c):
    d, f, N, B = c
    return f"{wd.set_id(d)}-{'finite' if f else 'mixed'}-N{N}-B{B}"


@pytest.mark.parametrize("dims,finite,N,B", CASES, ids=[_case_id(c) for c in CASES])
def test_truncated_solves_follow_the_reference_directions(dims, finite, N, B, solver_factory):
    p = wd.direction_problem(dims, N, finite)
    inp = wd.direction_inputs(p, B, wd.case_seed(dims, N, finite))
    for name, ok in SOLVERS.items():
        def solve_j(j):
            q = copy.copy(p); q.max_iter = j
            s = solver_factory(q); s.set_option("ocp_kernel", ok)
            assert s.get_option("ocp_kernel") == ok
            try:
                return s.ocp_solve(*inp, want_w=True)
            finally:
                s.close()      # (the factory closes what is still open at the end of the session: a handle per truncated solve would pile up)
        fig = wd.check_truncated(p, inp, solve_j)
        for j, f in enumerate(fig, 1):      # every figure, before anything is asserted
            print(f"wvdir {_case_id((dims, finite, N, B))} {name} j={j} resid={f['resid'].max():.3e} dalpha={f['dalpha'].max():.3e} "
                  f"dres_p={f['dres_p'].max():.3e} dmu={f['dmu'].max():.3e} acond={f['acond'].max():.3e} alpha_min={f['alpha'].min():.4f}")
        # nobody is left out: every instance stops at the iteration limit, in the reference and in the solver, at every j
        for j, f in enumerate(fig, 1):
            assert f["ref_active"].all(), (name, j, "the reference does not stop at the iteration limit")
        assert fig[-1]["ref_active_after"].all(), (name, "the reference does not stop at the iteration limit")
        for j, f in enumerate(fig, 1):
            assert f["limit"].all(), (name, j, "status / iters")
            assert f["resid"].max() <= TOL_DIR, (name, j, f["resid"])
            assert f["dalpha"].max() <= TOL_ALPHA, (name, j, f["dalpha"], f["alpha"], f["alpha_ref"])
            assert f["dres_p"].max() <= TOL_RES_P, (name, j, f["dres_p"], f["acond"])
            assert f["dmu"].max() <= TOL_MU, (name, j, f["dmu"], f["acond"])


# ---------------------------------------------------------------------------------------------------------------------------------
# VGPR form of the tile sweeps against the builtin form of the same products
# ---------------------------------------------------------------------------------------------------------------------------------
BIT_CASES = [(d, f, N) for d, f in SETS if d in wd.VGPR_SETS for N in (3, 6, 33)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("dims,finite,N", BIT_CASES, ids=[_case_id(c + (wd.BATCH,)) for c in BIT_CASES])
def test_vgpr_form_equals_the_builtin_form_bit_for_bit(dims, finite, N, solver_factory):
    from mpc_code_amd import capi
    p = wd.direction_problem(dims, N, finite)
    inp = wd.direction_inputs(p, wd.BATCH, wd.case_seed(dims, N, finite))
    generic = capi.build_library(dims=dims, extra_flags=wd.GENERIC_TILES)      # built by build(); here only its path
    assert os.path.basename(generic) != os.path.basename(capi.jit_library_path(dims))
    made = []
    try:
        for mi in (None, 1, 2, 3, 4):
            q = copy.copy(p)
            if mi is not None:
                q.max_iter = mi
            a = solver_factory(q); made.append(a); a.set_option("ocp_kernel", 3)
            b = capi.Solver(q, device=0, lib_path=generic); made.append(b); b.set_option("ocp_kernel", 3)
            # the switch reached the compiler of the one library and not of the other (mpc_build_info names it)
            assert "wv_generic_tiles" in b.build_info().split(";") and "wv_generic_tiles" not in a.build_info().split(";"), (a.build_info(), b.build_info())
            assert a.lib._name != b.lib._name
            ga, gb = a.ocp_solve(*inp, want_w=True), b.ocp_solve(*inp, want_w=True)
            if mi is None:
                assert (ga["status"] == 0).any(), ga["status"]      # the full solves do converge
            else:
                assert (ga["status"] == 1).all() and (ga["iters"] == mi).all(), (mi, ga["status"], ga["iters"])
            for k in ("status", "iters", "u0", "x1", "w", "res"):
                same = _bits(ga[k]) == _bits(gb[k])
                assert same.all(), (mi, k, np.argwhere(~same)[:8], ga[k][~same][:8], gb[k][~same][:8])
    finally:
        for s in made:
            s.close()
