"""The yardstick of per-instance set points on the non-linear tracking path (nmpc_set_setpoints; tests/test_inst_setpoints_host.py,
tests/test_nmpc_inst_setpoints.py), without touching oracle/: nmpc_oracle.closed_loop run instance by instance on a shallow copy of the oracle problem whose
defSP is a closure over that instance's rows - the device tests/nmpc_state_noise_ref.with_state_noise uses for def_pxp, which this module takes for w.

The inputs follow tests/inst_setpoints_ref.py: three schedules s_0, s_1, s_2 per model, instance b tracks s_{b mod 3}; each is the model's own schedule plus a
step in ysp and usp at the steps 2, 5 and 8, small enough that every target is solved at every step (a set point enters the target's cost alone: none drives it
infeasible).  Models: examples/cstr_nmpc.py (N = 30; Rss = 0, usp is not
read) and tests/nmpc_models/cl21.py at N = 32 and 33 (Rss != 0: usp is read; the paired and the four-instance form of the wave-style kernels)."""
import copy
import functools
import os
import warnings

import numpy as np

import nmpc_lin_family as lin
import nmpc_state_noise_ref as snr

HERE = os.path.dirname(os.path.abspath(__file__))
B, STEPS, SEED = 9, 10, 20252          # two full waves of four and a lone slot, or four pairs and a lone slot
CHANGES = (2, 5, 8)
LOGS, ILOGS = snr.LOGS, snr.ILOGS
CASES = {"cstr": ("cstr_nmpc.py", None), "cl21_N32": ("cl21", {"N": 32}), "cl21_N33": ("cl21", {"N": 33})}
# noise for the one case that runs together with v and w: cl21 at N = 32, with the matrices tests/test_nmpc_state_noise.py gives this model
NOISY_CASE = "cl21_N32"
CL21_NOISE = {"G_wn": np.array([[1.0, 0.2], [0.0, 1.0]]), "Q_wn": np.diag([4e-6, 1e-6]), "R_wn": 1e-7 * np.eye(2)}
_DY = {"cstr": ([[0.010, 0.020], [-0.015, -0.010], [0.005, 0.030]],
                [[-0.020, -0.015], [0.010, 0.025], [0.015, -0.020]],
                [[0.015, -0.025], [-0.012, 0.018], [-0.010, 0.015]]),
       "cl21": ([[0.04, -0.03], [-0.05, 0.02], [0.03, 0.04]],
                [[-0.03, 0.05], [0.05, -0.04], [-0.02, -0.03]],
                [[0.05, 0.03], [-0.04, -0.05], [-0.04, 0.05]])}
_DU = {"cstr": ([[1.0, 0.02], [-1.5, -0.01], [0.5, 0.03]], [[-1.0, -0.02], [2.0, 0.01], [1.5, -0.03]], [[0.5, 0.01], [-0.5, 0.02], [1.0, -0.02]]),
       "cl21": ([[0.05], [-0.08], [0.03]], [[-0.06], [0.07], [-0.04]], [[0.08], [-0.03], [0.06]])}


def _member(case):
    return "cstr" if case == "cstr" else "cl21"


@functools.lru_cache(maxsize=None)
def problem(case, noise=False):
    """(product problem, oracle problem, plant starts [B, nxp], model starts [B, nx])"""
    import mpc_code_amd
    import nmpc_oracle as no
    name, over = CASES[case]
    over = dict(over or {}, **(CL21_NOISE if noise else {})) or None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if case == "cstr":
            path = mpc_code_amd.example_path(name)
            p, o = mpc_code_amd.load_problem(path, overrides=over), no.load_problem(path, over)
        else:
            p, o = lin.load_product(name, over), lin.load_oracle(name, over)
    if case == "cstr":
        rng = np.random.default_rng(SEED)
        x0 = p.x0_p * (1.0 + 0.004 * rng.uniform(-1, 1, size=(B, p.nxp)))
        xm = x0.copy()
    else:
        x0, xm = lin.starts("cl21_rti", p.x0_p)
    return p, o, x0, xm


def schedule(case, j, n=STEPS):
    """(ysp [n, ny], usp [n, nu]) of s_j"""
    p = problem(case)[0]
    s = p.schedules(n)
    ysp, usp = np.array(s["ysp"][:n], dtype=np.float64), np.array(s["usp"][:n], dtype=np.float64)
    dy, du = np.asarray(_DY[_member(case)][j]), np.asarray(_DU[_member(case)][j])
    for i, k in enumerate(CHANGES):
        hi = CHANGES[i + 1] if i + 1 < len(CHANGES) else n
        ysp[k:hi] += dy[i]; usp[k:hi] += du[i]
    return ysp, usp


def shared_sched(case, j, n=STEPS):
    p = problem(case)[0]
    ysp, usp = schedule(case, j, n)
    return dict({k: np.array(a[:n]) for k, a in p.schedules(n).items()}, ysp=ysp, usp=usp)


@functools.lru_cache(maxsize=None)
def arrays(case, nb=B, n=STEPS):
    """(ysp [n, nb, ny], usp [n, nb, nu]): instance b tracks s_{b mod 3}; read-only"""
    s = [schedule(case, j, n) for j in range(3)]
    ysp = np.stack([s[b % 3][0] for b in range(nb)], axis=1); usp = np.stack([s[b % 3][1] for b in range(nb)], axis=1)
    ysp.setflags(write=False); usp.setflags(write=False)
    return ysp, usp


def with_setpoints(o, ysp_b, usp_b):
    """A shallow copy of the oracle problem ``o`` whose defSP returns the rows ysp_b [nsteps, ny], usp_b [nsteps, nu] of one instance (xsp stays its own)."""
    q = copy.copy(o)
    own, h = o.defSP, o.h
    ysp_b, usp_b = np.asarray(ysp_b, dtype=np.float64), np.asarray(usp_b, dtype=np.float64)

    def defSP(t):
        k = int(round(t / h))
        xsp = np.zeros(o.nx) if own is None else np.ravel(own(t)[2])
        return [ysp_b[k], usp_b[k], xsp]
    q.defSP = defSP
    return q


def closed_loop(o, nsteps, x0_p, x0_m, ysp, usp, v=None, w=None, max_sqp=1, sqp_tol=1e-9):
    """The batch run by the oracle, instance by instance, each with its own set points (and its own noise); logs [nsteps, B, dim]."""
    import nmpc_oracle as no
    runs = []
    for b in range(len(x0_p)):
        q = with_setpoints(o, ysp[:, b], usp[:, b])
        if w is not None:
            q = snr.with_state_noise(q, w[:, b])
        with np.errstate(all="ignore"):
            runs.append(no.closed_loop(q, nsteps, x0_p=x0_p[b], x0_m=x0_m[b], max_sqp=max_sqp, sqp_tol=sqp_tol, v_wn=None if v is None else v[:, b]))
    out = {k: np.stack([r[k] for r in runs], axis=1) for k in LOGS + ILOGS}
    for k in ILOGS:
        out[k] = out[k].astype(np.int32)
    return out


GOLDEN = os.path.join(HERE, "golden", "nmpc_inst_setpoints.npz")
GOLDEN_CASES = (("cstr", False), ("cl21_N32", False), ("cl21_N32", True), ("cl21_N33", False))      # (case, with v and w)


def noise(case):
    from mpc_code_amd import nmpc
    return nmpc.path_noise(problem(case, True)[0], STEPS, B, SEED)


def inputs(case, noisy=False):
    """(ysp, usp, v, w) of a golden case"""
    return arrays(case) + (noise(case) if noisy else (None, None))


def oracle_run(case, noisy=False, instances=None):
    """the per-instance oracle loops of a golden case (minutes for the CSTR: tests read tests/golden/nmpc_inst_setpoints.npz, written by
    tests/golden/make_nmpc_inst_setpoints_golden.py, and tests/test_inst_setpoints_host.py recomputes a few instances of it)"""
    p, o, x0, xm = problem(case, noisy)
    ysp, usp, v, w = inputs(case, noisy)
    sel = slice(None) if instances is None else list(instances)
    return closed_loop(o, STEPS, x0[sel], xm[sel], ysp[:, sel], usp[:, sel], None if v is None else v[:, sel], None if w is None else w[:, sel])


def golden_key(case, noisy, log):
    return f"{case}{'_vw' if noisy else ''}_{log}"


@functools.lru_cache(maxsize=None)
def reference(case, noisy=False):
    """the recorded oracle loops of a golden case, logs [STEPS, B, dim]"""
    with np.load(GOLDEN) as g:
        return {k: g[golden_key(case, noisy, k)] for k in LOGS + ILOGS}
