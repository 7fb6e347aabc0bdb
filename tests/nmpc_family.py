"""A family of small non-linear tracking models at the tile edges of the wave-style kernels (csrc/mpc_nmpc.hip: kernels 3 and 4, the LTV form of
the wave solver), shared by tests/test_nmpc_family.py, tests/golden/make_nmpc_family_golden.py and the build (one library per member).

    member  nx/nu/ny/nd  model, estimator                                        in the family for
    c11     1/1/1/1      continuous, EKF, "nl"                                    stage state 1 (a one-element tile), nd = 1
    d22     2/2/2/2      discrete, lue, "lin" (Bd, Cd != 0), User_vfin, Sss       discrete model, observer, Cd, Pf, duss_form on kernels 3 / 4
    c41     4/1/1/1      continuous, EKF, "nl", y = x[3], xmax = [inf,b,inf,b]    full tile with one input column, last-state output, masked bounds
    d42     4/2/2/2      discrete, EKF, "lin", Pf, every bound finite             discrete Jacobians in the EKF, full tile with two inputs, unmasked tables
    c31r    3/1/2/2 + 1  continuous, EKF, one User_g_ineq row (in x and u)        stage state 4 = 3 + row with nu = 1
    c22     2/2/1/1      continuous, lue, "nl", dmin/dmax, def_pxp, def_pyp       observer with a continuous model, ny < nx, disturbance saturation

Both loaders accept every member as listed: no combination had to be replaced by a neighbour.  The models are tests/nmpc_models/<member>.py, Ex-style
files with equations of their own.  Horizons: c11 8, d22 6, c41 10, d42 9, c31r 7, c22 6.

d22 was redrawn once.  Its first draft asked for a second set point whose input target sat ON a bound of the second input (and N = 11): the OCP's input
then hugs that bound with multipliers near zero, and a QP ended by an interior-point tolerance differs from one ended on an exact active set by 1e-6 - the
oracle itself with its active-set polish taken out moved by 1e-6 on every instance, and every kernel sat 2.8e-6 from the goldens, while E_ref (3e-11) saw
nothing of it.  Now both input targets stay inside their bounds, the first input's bound (0.6) is active through the transient, and the horizon is 6 so that
the saturated transient still feels the terminal weight; the oracle without its polish is then within 9e-8 of itself and the kernels within 2.3e-9.

Cases (names are the prefixes of the arrays in tests/golden/nmpc_family.npz):
    <member>_rti    12 steps, max_sqp = 1, a set-point change inside the run
    <member>_sqp    4 steps, max_sqp = 50, sqp_tol = 1e-9
    <member>_N<n>   d22 and c41 at N = 2, 5, 31, 32, 33, 64: real-time iteration, 6 steps (N is a run-time field: the member's library)
    d22_hold        d22 with two starts outside its output box next to a healthy one, 3 steps: every step of the two is held (status 2), and from the
                    farther one the target is infeasible as well (status 2: the previous target is kept) - the two paths of the hold rule
Each case but the last has 9 instances whose plant and model start apart.  The reference is oracle/nmpc_oracle.py; for c31r its restatement with the rows,
tests/nmpc_rows_ref.py.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_DIR = os.path.join(HERE, "nmpc_models")
GOLDEN = os.path.join(HERE, "golden", "nmpc_family.npz")

MEMBERS = ("c11", "d22", "c41", "d42", "c31r", "c22")
DIMS = {"c11": (1, 1, 1, 1), "d22": (2, 2, 2, 2), "c41": (4, 1, 1, 1), "d42": (4, 2, 2, 2), "c31r": (3, 1, 2, 2), "c22": (2, 2, 1, 1)}
MODES = {"rti": (12, 1), "sqp": (4, 50)}      # mode: (steps, max_sqp)
SQP_CASES = tuple(f"{m}_sqp" for m in MEMBERS)      # the cases whose SQP iteration counts are not 1 by construction: the population of the 5 % cap
SQP_TOL = 1e-9
HORIZON_MEMBERS = ("d22", "c41")
HORIZONS = (2, 5, 31, 32, 33, 64)      # both sides of the paired / unpaired switch (32 | 33), both remainders of the sweep groups, the shortest and the longest
HORIZON_STEPS = 6
B = 9                                  # two full waves of four and one with a single live slot; beyond N = 32 one instance is left without its pair partner
LOGS = ("U", "X_HAT", "XS", "US", "Xp", "D_HAT")
ILOGS = ("STATUS_DYN", "STATUS_SS", "SQP_DYN", "SQP_SS")
HOLD_CASE, HOLD_STEPS = "d22_hold", 3
FD_STEPS = (1e-6, 3e-6)                # nmpc_oracle._fd's own step and the second one: their difference is the reference's uncertainty E_ref

# relative spread of the plant's starts about x0_p, and of the model's starts about the plant's
SPREAD = {"c11": (0.10, 0.05), "d22": (0.10, 0.05), "c41": (0.08, 0.04), "d42": (0.08, 0.04), "c31r": (0.05, 0.03), "c22": (0.08, 0.04)}

# feature switches (overrides of the Ex-file's namespace): the golden run has to feel each of them (tests/golden/make_nmpc_family_golden.py)
_D22_K = np.array([[0.35, 0.00], [0.00, 0.35], [0.30, -0.05], [0.00, 0.30]])
_C22_K = np.array([[0.10], [0.45], [0.30]])
SWITCHES = {
    "d22": {"Pf0": {"User_vfin": None}, "Cd0": {"Cd": np.zeros((2, 2))}, "SssAsRss": {"Sss": None, "Rss": 0.5 * np.eye(2)}, "Khalf": {"K": 0.5 * _D22_K}},
    "d42": {"Pf0": {"User_vfin": None}, "Cd0": {"Cd": np.zeros((2, 2))}},
    "c31r": {"norow": None},           # (the oracle without the row: nmpc_oracle.closed_loop)
    "c22": {"Khalf": {"K": 0.5 * _C22_K}, "nosat": {"dmin": None, "dmax": None}},
}
BITE_INSTANCES = 3                     # the switched-off runs repeat the first instances of the member's rti case


def model_path(member):
    return os.path.join(MODEL_DIR, member + ".py")


def load_product(member, overrides=None):
    """The member as the product's loader reads it (mpc_code_amd.load_problem)."""
    import warnings
    import mpc_code_amd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mpc_code_amd.load_problem(model_path(member), overrides=overrides)


def load_oracle(member, overrides=None, rows=None):
    """The member as the oracle's loader reads it; a member with a user row through tests/nmpc_rows_ref.py (rows = False: without its row)."""
    import warnings
    import nmpc_oracle as no
    if (member == "c31r") if rows is None else rows:
        import nmpc_rows_ref
        return nmpc_rows_ref.load(model_path(member), overrides)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return no.load_problem(model_path(member), overrides)


def case_names():
    names = [f"{m}_{mode}" for m in MEMBERS for mode in MODES]
    names += [f"{m}_N{n}" for m in HORIZON_MEMBERS for n in HORIZONS]
    return names + [HOLD_CASE]


def case_spec(name):
    """(member, steps, max_sqp, overrides) of a case."""
    member, tag = name.split("_")
    if tag in MODES:
        return (member,) + MODES[tag] + (None,)
    if tag == "hold":
        return member, HOLD_STEPS, 1, None
    return member, HORIZON_STEPS, 1, {"N": int(tag[1:])}


def starts(name, x0_p):
    """Plant and model starts of a case, [B, nx] each: drawn about the member's x0_p, apart from each other."""
    member, tag = name.split("_")
    x0_p = np.asarray(x0_p, dtype=np.float64)
    if tag == "hold":      # the first output far above its box (ymax = 1.6; the held input does not bring it back within the run): from 6.0 the target is
        x0 = np.array([[6.0, 0.45], [4.0, 0.45], x0_p])      # infeasible too (the previous one is kept), from 4.0 the OCP alone is held; next to a healthy start
        return x0, x0.copy()
    rng = np.random.default_rng([MEMBERS.index(member), sum(map(ord, tag))])
    sp, sm = SPREAD[member]
    x0 = x0_p * (1.0 + sp * rng.uniform(-1, 1, size=(B, x0_p.size)))
    xm = x0 * (1.0 + sm * rng.uniform(-1, 1, size=(B, x0_p.size)))
    return x0, xm


def oracle_instance(member, overrides, nsteps, max_sqp, x0, xm, fd_step=FD_STEPS[0], rows=None):
    """One instance of a case run by the oracle (finite-difference step ``fd_step``); returns its logs."""
    import nmpc_oracle as no
    p = load_oracle(member, overrides, rows)
    saved = no._fd.__defaults__
    no._fd.__defaults__ = (fd_step,)
    try:
        if hasattr(p, "g_user"):
            import nmpc_rows_ref
            return nmpc_rows_ref.closed_loop(p, nsteps, x0_p=x0, x0_m=xm, max_sqp=max_sqp, sqp_tol=SQP_TOL)
        return no.closed_loop(p, nsteps, x0_p=x0, x0_m=xm, max_sqp=max_sqp, sqp_tol=SQP_TOL)
    finally:
        no._fd.__defaults__ = saved


def expected_status(name, shape):
    """(STATUS_DYN, STATUS_SS) a case's golden logs have to show: zero everywhere, but for the held instances of the hold case."""
    dyn, ss = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
    if name == HOLD_CASE:
        dyn[:, :2] = 2; ss[:, 0] = 2
    return dyn, ss


def rel_diff(a, g):
    """max |a - g| / (1 + |g|): the measure of every comparison of this family."""
    a, g = np.asarray(a, dtype=np.float64), np.asarray(g, dtype=np.float64)
    return float(np.max(np.abs(a - g) / (1.0 + np.abs(g)))) if g.size else 0.0


def sqp_counts_within_cap(pairs):
    """SQP iteration counts against the reference's, ``pairs`` = [(counts, reference counts), ...]: no count apart by more than 1, and at most 5 % of the
    instance-steps of all pairs together apart at all."""
    a = np.concatenate([np.ravel(x) for x, _ in pairs]).astype(np.int64)
    g = np.concatenate([np.ravel(y) for _, y in pairs]).astype(np.int64)
    return bool(np.abs(a - g).max(initial=0) <= 1 and (a != g).mean() <= 0.05)
