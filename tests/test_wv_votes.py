"""Verdicts of the wave solver at the row boundaries of the DPP network, against the lane solver.

The wave solver (``ocp_kernel`` 3) decides feasibility, complementarity and the multiplier test of an iterate by votes over the lanes
of a wave (lane = block of the horizon) and takes its sums and maxima with DPP moves that carry no ``old`` operand.  Both could pick
up a lane beyond the horizon where the horizon ends at, one before or one after a row of 16 lanes: N = 15, 16, 17, 31, 32, 33, 48,
49, 64, and N = 2.  Per horizon and bound variant (every state bound finite: the kernels without bound masks; some infinite: the
kernels with them) three kinds of instance go through the per-call ``mpc_ocp_solve`` on the wave solver and on the lane solver
(``ocp_kernel`` 1, plain C++ recursions, the yardstick):

    solved      a feasible instance, the first one of the pool the C restatement solves;
    infeasible  one whose state box cannot be met from its initial state: the first one of the pool the C restatement refuses after
                at least INFEAS_MIN_ITERS iterations, i.e. through the multiplier test, not at stage 0;
    truncated   both of them with ``max_iter = 3``.

The pool is drawn per case as in tests/test_gpu_fuzz.py (states up to 0.8 of the box); the kinds are chosen with the C restatement
(oracle/mpc_oracle.c) when the module is first used and asserted on the lane solver's answer, so a case cannot pass by testing
something else than it says.

Tolerances of u0 between the two solvers.  Truncated: the solvers take the corrector's step length with an approximate reciprocal,
which tests/test_wv_directions.py allows TOL_ALPHA (relative) per iteration, on an input step no longer than the input box; three
iterations, plus twice the direction error TOL_DIR on a scale of the box: 3 TOL_ALPHA w + 2 TOL_DIR w with w = max(umax - umin).
Solved: both answers are optima to the solver's tolerances; 1e-6, the figure of tests/test_gpu_fuzz.py for a converged u against a
reference.

The company test puts four instances into one wave - a quick one, an infeasible one, one stopped by the iteration limit and a slow
one, with the limit set two iterations after the infeasible verdict - and compares every instance bit for bit with the same instance
solved alone: a vote or a reduction that looked at a neighbour's lanes would show there.  Its last case puts a NaN state into one
slot.
"""
import copy
import functools

import numpy as np
import pytest

import wv_direction_ref as wd

pytestmark = pytest.mark.gpu

DIMS = (3, 2, 3, 3, 3, 0, 0)      # the benchmark's dimension set
HORIZONS = [2, 15, 16, 17, 31, 32, 33, 48, 49, 64]
POOL = 48
INFEAS_MIN_ITERS = 6      # by the C restatement's count; more than the three iterations of the truncated solves on any solver
WAVE, LANE = 3, 1
TOL_U0_SOLVED = 1e-6


def tol_u0_truncated(p):
    w = float(np.max(p.umax - p.umin))
    return 3 * wd.TOL_ALPHA * w + 2 * wd.TOL_DIR * w


def pool(N, finite):
    p = wd.direction_problem(DIMS, N, finite)
    rng = np.random.default_rng(wd.case_seed(DIMS, N, finite) + 5)
    scale = np.where(np.isfinite(p.xmax), p.xmax, 3.0)
    xh = rng.uniform(-0.8, 0.8, (POOL, p.nx)) * scale
    d = 0.05 * rng.standard_normal((POOL, p.nd))
    xs = 0.1 * rng.standard_normal((POOL, p.nx)); us = 0.1 * rng.standard_normal((POOL, p.nu))
    up = rng.uniform(-0.3, 0.3, (POOL, p.nu))
    return p, (xh, xs, us, d, up)


@functools.lru_cache(maxsize=None)
def oracle_pool(N, finite):
    """The pool and what the C restatement makes of it (status, iters per instance)."""
    import oracle_c
    oracle_c.build()
    p, inp = pool(N, finite)
    o = oracle_c.OracleC(p).ocp_solve(*inp)
    return p, inp, o["status"].copy(), o["iters"].copy()


def take(inp, idx):
    return tuple(np.ascontiguousarray(a[list(idx)]) for a in inp)


def kinds(N, finite):
    """(problem, inputs of [solved, infeasible]) of a case."""
    p, inp, st, it = oracle_pool(N, finite)
    solved = np.flatnonzero((st == 0) & (it >= 5))      # (not done within the truncated solves' three iterations)
    infeas = np.flatnonzero((st == 2) & (it >= INFEAS_MIN_ITERS))
    assert len(solved) and len(infeas), (N, finite, st, it)
    return p, take(inp, (solved[0], infeas[0]))


def company(N):
    """(problem with its iteration limit, inputs of [quick, infeasible, truncated, slow]) at horizon N, every state bound finite: the
    limit lies two iterations after the infeasible one's verdict, the truncated one needs three more than that at the least (to be
    solved or to be refused), the slow one ends two before it at the latest.  The first infeasible instance of the pool, in the
    order of their iteration counts, that finds such company."""
    p, inp, st, it = oracle_pool(N, True)
    solved = np.flatnonzero((st == 0) & (it > 0)); infeas = np.flatnonzero((st == 2) & (it >= INFEAS_MIN_ITERS))
    quick = solved[np.argmin(it[solved])]
    for first in infeas[np.argsort(it[infeas], kind="stable")]:
        limit = int(it[first]) + 2
        later = np.flatnonzero(it >= limit + 3)
        slower = solved[(it[solved] > it[quick]) & (it[solved] <= limit - 2)]
        if len(later) and len(slower):
            q = copy.copy(p); q.max_iter = limit
            return q, take(inp, (quick, first, later[0], slower[np.argmax(it[slower])]))
    raise AssertionError(("no company in the pool", N, st, it))


def solve(solver_factory, p, inp, kernel):
    s = solver_factory(p); s.set_option("ocp_kernel", kernel)
    assert s.get_option("ocp_kernel") == kernel
    try:
        return s.ocp_solve(*inp)
    finally:
        s.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


CASES = [(N, f) for f in (True, False) for N in HORIZONS]


@pytest.mark.parametrize("N,finite", CASES, ids=[f"N{N}-{'finite' if f else 'mixed'}" for N, f in CASES])
def test_verdicts_at_the_row_boundaries_equal_the_lane_solvers(N, finite, solver_factory):
    p, inp = kinds(N, finite)
    p3 = copy.copy(p); p3.max_iter = 3
    for q, kind in ((p, "full"), (p3, "truncated")):
        lane, wave = solve(solver_factory, q, inp, LANE), solve(solver_factory, q, inp, WAVE)
        du = np.abs(wave["u0"] - lane["u0"]).max(axis=1)
        print(f"wvvotes N={N} finite={finite} {kind}: lane status {lane['status']} iters {lane['iters']} | wave status {wave['status']} iters {wave['iters']} | du0 {du}")
        # the case is what it says (the lane solver is the yardstick)
        if kind == "full":
            assert list(lane["status"]) == [0, 2] and lane["iters"][1] > 3, (lane["status"], lane["iters"])
        else:
            assert list(lane["status"]) == [1, 1] and list(lane["iters"]) == [3, 3], (lane["status"], lane["iters"])
        assert np.array_equal(wave["status"], lane["status"]), (kind, wave["status"], lane["status"])
        keep = lane["status"] != 2
        assert np.array_equal(wave["iters"][keep], lane["iters"][keep]), (kind, wave["iters"], lane["iters"])
        tol = TOL_U0_SOLVED if kind == "full" else tol_u0_truncated(p)
        assert (du[keep] <= tol).all(), (kind, du, tol)


@pytest.mark.parametrize("N", HORIZONS)
def test_an_instance_in_company_equals_itself_alone_bit_for_bit(N, solver_factory):
    q, inp = company(N)
    four = solve(solver_factory, q, inp, WAVE)
    lane = solve(solver_factory, q, inp, LANE)
    print(f"wvvotes company N={N} limit {q.max_iter}: wave status {four['status']} iters {four['iters']} | lane status {lane['status']} iters {lane['iters']}")
    # quick, infeasible, truncated, slow - on the yardstick and on the wave solver
    assert list(lane["status"]) == [0, 2, 1, 0] and lane["iters"][2] == q.max_iter and lane["iters"][0] < lane["iters"][3], (lane["status"], lane["iters"])
    assert np.array_equal(four["status"], lane["status"]), (four["status"], lane["status"])
    for b in range(4):
        one = solve(solver_factory, q, take(inp, (b,)), WAVE)
        for k in ("status", "iters", "u0", "res"):
            assert np.array_equal(_bits(four[k][b]), _bits(one[k][0])), (N, b, k, four[k][b], one[k][0])


def test_a_nan_state_in_one_slot_leaves_the_others_alone(solver_factory):
    N = 33
    q, inp = company(N)
    four = solve(solver_factory, q, inp, WAVE)
    bad = tuple(a.copy() for a in inp)
    bad[0][2, :] = np.nan      # the truncated one's slot
    g = solve(solver_factory, q, bad, WAVE)
    print(f"wvvotes nan slot: status {g['status']} iters {g['iters']} (clean: {four['status']} {four['iters']})")
    assert g["status"][2] != 0, g["status"]      # a verdict, not a solution
    for b in (0, 1, 3):
        for k in ("status", "iters", "u0", "res"):
            assert np.array_equal(_bits(g[k][b]), _bits(four[k][b])), (b, k, g[k][b], four[k][b])
