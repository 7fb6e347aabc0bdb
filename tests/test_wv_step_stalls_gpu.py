"""The wave-autonomous kernels after the vector-memory waits and the dead work left their steps (csrc/mpc_wave.hpp): what each of the
three changes could have broken, on the GPU.

Last block.  The gradient of the last block takes the terminal weight Pf where the others take Q, now selected per lane from scalar
loads.  Per-call ``mpc_ocp_solve`` on the wave solver (``ocp_kernel`` 3) against the lane solver (``ocp_kernel`` 1, plain C++
recursions, the yardstick) with ``max_iter`` = 1, 2, 3 - an unconverged iterate cannot forgive a wrong gradient - and a terminal weight
of 50 Q, so that the selection shows.  Horizons 2, 3, 17, 33, 64; the benchmark's dimension set, a Delta-u form set (cross term) and one
with a stage state above 4 (2 x 2 tiles: no tile constants in LDS), and two more one-tile sets for the tile constants themselves - a
Delta-u form (M) and one with fewer states than inputs (R has more rows than A); every state bound finite (kernels without bound masks) and the
draw's mix (kernels with them).  Tolerance of u0: that of tests/test_wv_votes.py for truncated solves, 3 TOL_ALPHA w + 2 TOL_DIR w with
w the widest input box (accounted for there).

Target exit.  The target's loop (target_row16, 16 lanes per instance) now leaves at the verdict of the wave's last instance.  Four
instances of one wave whose target solves end in different trips of that loop - one that carries on warm, one that starts cold after a
refused target, one refused as infeasible (the previous target is kept) and one stopped by a small iteration limit, chosen from a pool
by the C restatement and asserted on the kernel's own answer - against each of them alone in a batch of one: XS, US, the target's
status and iteration count bit for bit, over six steps.  Then batches of 3 and 2 in a wave of four (the unused slots alias slot 0), and
the four once more on examples/cstr_lmpc_ss_rows.py (user rows in the target).

Synchronisation.  The one-wave kernels order their LDS traffic without waiting for global memory.  N = 2, where the estimator's
exchange area reaches the zero row of the tile view and is zeroed again in every step; batches of 5 and 7, six steps in two launches,
kernel 3 against kernel 1 on U, XS, X_HAT and the status words.  Tolerance: 1e-6, what
tests/test_gpu_parity.py:test_both_kernels_leave_the_same_resident_state allows between these kernels' resident states.
"""
import copy
import functools

import numpy as np
import pytest

import wv_direction_ref as wd

pytestmark = pytest.mark.gpu

WAVE, LANE = 3, 1

# ---------------------------------------------------------------------------------------------------------------------------------
# last block
# ---------------------------------------------------------------------------------------------------------------------------------
# CSTR | Delta-u form (stage state 5) | stage state 5 without cross term (these two: 2 x 2 tiles, no tile constants) | Delta-u form on one tile (the
# cross term M from the tile constants) | fewer states than inputs (R reaches beyond the rows of A in the tile constants; built by build())
LAST_SETS = [(3, 2, 3, 3, 3, 0, 0), (3, 2, 2, 2, 3, 1, 0), (5, 2, 2, 2, 5, 0, 0), (2, 1, 1, 1, 2, 1, 0), (1, 2, 1, 1, 1, 0, 0)]
LAST_HORIZONS = [2, 3, 17, 33, 64]
LAST_CASES = [(d, N, f) for d in LAST_SETS for N in LAST_HORIZONS for f in (True, False)]


def tol_u0_truncated(p):
    w = float(np.max(p.umax - p.umin))
    return 3 * wd.TOL_ALPHA * w + 2 * wd.TOL_DIR * w


@pytest.mark.parametrize("dims,N,finite", LAST_CASES, ids=[f"{wd.set_id(d)}-N{N}-{'finite' if f else 'mixed'}" for d, N, f in LAST_CASES])
def test_last_blocks_gradient_takes_the_terminal_weight(dims, N, finite, solver_factory):
    p = wd.direction_problem(dims, N, finite)
    p.P = 50.0 * p.Q
    if p.nu > p.ny:      # more inputs than outputs: the target problem needs a weight on the inputs to have one answer (the solver refuses it otherwise)
        p.Rss = 0.1 * np.eye(p.nu)
    inp = wd.direction_inputs(p, wd.BATCH, wd.case_seed(dims, N, finite) + 11)
    tol = tol_u0_truncated(p)
    for mi in (1, 2, 3):
        q = copy.copy(p); q.max_iter = mi
        out = {}
        for kern in (LANE, WAVE):
            s = solver_factory(q); s.set_option("ocp_kernel", kern)
            assert s.get_option("ocp_kernel") == kern
            try:
                out[kern] = s.ocp_solve(*inp)
            finally:
                s.close()
        lane, wave = out[LANE], out[WAVE]
        du = np.abs(wave["u0"] - lane["u0"]).max(axis=1)
        print(f"laststage {wd.set_id(dims)} N={N} finite={finite} max_iter={mi}: lane status {lane['status']} iters {lane['iters']} | du0 max {du.max():.3e} (tol {tol:.3e})")
        # the case is what it says: nobody is done or refused within the truncated solve
        assert (lane["status"] == 1).all() and (lane["iters"] == mi).all(), (lane["status"], lane["iters"])
        assert np.array_equal(wave["status"], lane["status"]) and np.array_equal(wave["iters"], lane["iters"]), (wave["status"], wave["iters"])
        assert (du <= tol).all(), (mi, du, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# target exit
# ---------------------------------------------------------------------------------------------------------------------------------
T_STEPS, T_POOL, T_LIMIT, T_N = 6, 48, 8, 5
T_KEYS = ("XS", "US", "STATUS_SS", "ITERS_SS")


def target_problem(pkg, example):
    p = pkg.load_problem(pkg.example_path(example), overrides={"N": T_N})
    p.max_iter = T_LIMIT
    return p


def target_pool():
    """Initial states in the benchmark's box and initial disturbance estimates from none to far outside what the target's box can absorb."""
    rng = np.random.default_rng(7)
    x0 = rng.uniform([-0.5, -8.0, -5.0], [0.5, 8.0, 5.0], size=(T_POOL, 3))
    scale = np.repeat([0.0, 0.02, 0.2, 1.0, 5.0, 25.0], T_POOL // 6)[:, None]
    d0 = rng.standard_normal((T_POOL, 3)) * scale * [0.1, 2.0, 1.0]
    return x0, d0


@functools.lru_cache(maxsize=None)
def target_company():
    """(step, [warm, cold, infeasible, limit]): pool members whose target solves at that step are, by the C restatement, a solved one that
    was solved the step before, a solved one that was refused the step before, a refused one and one stopped by the iteration limit - with
    four different iteration counts."""
    import mpc_code_amd as pkg
    import oracle_c
    oracle_c.build()
    p = target_problem(pkg, "cstr_lmpc.py")
    x0, d0 = target_pool()
    c = oracle_c.OracleC(p).closed_loop(T_STEPS, x0, x0, dhat0=d0)
    st, it = c["STATUS_SS"], c["ITERS_SS"]
    for k in range(1, T_STEPS):
        warm = np.flatnonzero((st[k] == 0) & (st[k - 1] == 0)); cold = np.flatnonzero((st[k] == 0) & (st[k - 1] == 2))
        infe = np.flatnonzero(st[k] == 2); lim = np.flatnonzero((st[k] == 1) & (it[k] == T_LIMIT))
        for w in warm:
            for cd in cold:
                for i in infe:
                    for m in lim:
                        if len({int(it[k][w]), int(it[k][cd]), int(it[k][i]), int(it[k][m])}) == 4:
                            return k, (int(w), int(cd), int(i), int(m))
    raise AssertionError(("no such company in the pool", st.T, it.T))


def run_loop(solver_factory, p, x0, d0, wave_instances, launches=(T_STEPS,), kernel=WAVE):
    from mpc_code_amd import capi
    s = solver_factory(p, kernel)
    try:
        if wave_instances:
            s.set_option("wave_instances", wave_instances)
        n = sum(launches)
        s.loop_alloc(len(x0), n, capi.LOG_ALL); s.loop_set_state(x0, x0, dhat=d0); s.loop_set_schedule(p.schedules(n))
        k0 = 0
        for m in launches:
            s.loop_run(k0, m); k0 += m
        s.loop_sync()
        return {k: s.loop_get_log(k) for k in ("U", "X_HAT", "XS", "US", "STATUS_DYN", "STATUS_SS", "ITERS_DYN", "ITERS_SS")}
    finally:
        s.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


@pytest.fixture(scope="module")
def alone(pkg, solver_factory):
    """every member of the company alone in a wave of four, per example: computed once"""
    made = {}

    def get(example):
        if example not in made:
            _, members = target_company()
            p = target_problem(pkg, example)
            x0, d0 = target_pool()
            made[example] = [run_loop(solver_factory, p, x0[[b]], d0[[b]], 4) for b in members]
        return made[example]
    return get


@pytest.mark.parametrize("example,take", [("cstr_lmpc.py", (0, 1, 2, 3)), ("cstr_lmpc.py", (3, 2, 0)), ("cstr_lmpc.py", (1, 3)), ("cstr_lmpc.py", (2, 0)),
                                          ("cstr_lmpc_ss_rows.py", (0, 1, 2, 3))],
                         ids=["four", "three", "two-cold-limit", "two-infeasible-warm", "four-ss-rows"])
def test_target_of_an_instance_in_company_equals_itself_alone(example, take, pkg, solver_factory, alone):
    k, members = target_company()
    p = target_problem(pkg, example)
    x0, d0 = target_pool()
    idx = [members[t] for t in take]
    ones = alone(example)
    got = run_loop(solver_factory, p, x0[idx], d0[idx], 4)
    st = [int(ones[t]["STATUS_SS"][k, 0]) for t in range(4)]; it = [int(ones[t]["ITERS_SS"][k, 0]) for t in range(4)]
    print(f"targetexit {example} take {take}: step {k}, alone status {st} iters {it} | company status {got['STATUS_SS'][k]} iters {got['ITERS_SS'][k]}")
    if example == "cstr_lmpc.py":
        # the case is what it says, on the kernel's own answer: warm, cold (refused the step before), infeasible with the previous target kept, stopped by the limit
        prev = [int(ones[t]["STATUS_SS"][k - 1, 0]) for t in range(4)]
        assert st == [0, 0, 2, 1] and prev[0] == 0 and prev[1] == 2 and it[3] == T_LIMIT and len(set(it)) == 4, (st, prev, it)
        assert np.array_equal(ones[2]["XS"][k], ones[2]["XS"][k - 1]) and np.array_equal(ones[2]["US"][k], ones[2]["US"][k - 1])
    else:
        assert len({(s_, i_) for s_, i_ in zip(st, it)}) > 1, (st, it)      # they do not all end in the same trip
    for slot, t in enumerate(take):
        for key in T_KEYS:
            same = _bits(got[key][:, slot]) == _bits(ones[t][key][:, 0])
            assert same.all(), (example, take, slot, key, np.argwhere(~same)[:4], got[key][:, slot], ones[t][key][:, 0])


# ---------------------------------------------------------------------------------------------------------------------------------
# synchronisation
# ---------------------------------------------------------------------------------------------------------------------------------
TOL_KERNELS = 1e-6      # tests/test_gpu_parity.py:test_both_kernels_leave_the_same_resident_state


@pytest.mark.parametrize("B", [5, 7])
def test_short_horizon_in_two_launches_equals_the_lane_kernel(B, pkg, solver_factory):
    p = pkg.load_problem(pkg.example_path("cstr_lmpc.py"), overrides={"N": 2})
    rng = np.random.default_rng(100 + B)
    x0 = rng.uniform([-0.5, -8.0, -5.0], [0.5, 8.0, 5.0], size=(B, 3))
    d0 = np.zeros((B, 3))
    wave = run_loop(solver_factory, p, x0, d0, 0, launches=(3, 3), kernel=WAVE)
    lane = run_loop(solver_factory, p, x0, d0, 0, launches=(3, 3), kernel=LANE)
    for key in ("STATUS_DYN", "STATUS_SS"):
        assert np.array_equal(wave[key], lane[key]), (key, wave[key], lane[key])
    for key in ("U", "XS", "X_HAT"):
        d = float(np.abs(wave[key] - lane[key]).max())
        print(f"wvsync B={B} {key}: max |wave - lane| = {d:.3e}")
        assert d < TOL_KERNELS, (key, d)
