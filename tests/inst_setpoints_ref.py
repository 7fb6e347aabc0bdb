"""The yardstick of per-instance set points on the linear path (mpc_loop_set_setpoints; tests/test_inst_setpoints_host.py, tests/test_inst_setpoints.py),
built from the restatements under oracle/ as they are: a batch in which every instance tracks its own schedule is, instance by instance, the C restatement's
loop of that one instance with its own rows as the schedule (``c_loops``, as lin_noise_ref.folded_c_loops does for the noise), and the NumPy restatement,
whose target solve broadcasts ysp / usp to [B, .], takes the arrays for all instances at once (``np_loop``).

The inputs.  Three schedules s_0, s_1, s_2 per problem, instance b tracks s_{b mod 3}.  Each is the example's own schedule plus a step in ysp (and in usp)
at the steps 2, 5 and 8.  The target problem of a tracking MPC is feasible or not whatever the set point is - the set point enters its cost alone - so no
finite step drives it infeasible, and none gives status 2: the sizes below leave the targets of s_0 and s_1 reachable, and s_2 has a stretch (the steps 5, 6, 7)
whose set point lies far outside the bounds, so that the target of those instances rides its bounds next to neighbours whose targets move freely.  (Rows of
NaN do give status 2 in both restatements; the device's target solvers return NaN targets for them, on the shared schedule as well - not an input a test can
hold the kernels to today.)

Problems: "cstr" (Kalman filter; Rss = 0, so its target does not read usp), "wb" (fixed gain, input-move form; Rss = 0 too), and "cstr_rss": the CSTR with
Rss = diag(2, 1) by override, the case in which usp is read."""
import functools
import warnings

import numpy as np

import lin_noise_ref as lnr

B, NSTEPS = lnr.B, lnr.NSTEPS          # 70 instances (padded stride 128, a last wave with two of four slots empty), 12 steps
CHANGES = (2, 5, 8)
EXAMPLES = {"cstr": ("cstr_lmpc.py", None), "wb": ("wood_berry_lmpc.py", None), "cstr_rss": ("cstr_lmpc.py", {"Rss": np.diag([2.0, 1.0]).tolist()})}
# the steps of s_j: rows = the three changes, added to the example's own row from that step on
_DY = {"cstr": ([[0.10, 0.0, 0.05], [-0.15, 0.0, 0.20], [0.05, 0.0, -0.10]],
                [[-0.20, 0.0, 0.15], [0.10, 0.0, -0.05], [0.25, 0.0, 0.10]],
                [[0.15, 0.0, -0.20], [0.0, 0.0, 0.0], [-0.10, 0.0, 0.25]]),
       "wb": ([[0.4, -0.2], [-0.3, 0.5], [0.2, 0.1]],
              [[-0.5, 0.3], [0.6, -0.4], [-0.1, -0.3]],
              [[0.3, 0.4], [0.0, 0.0], [-0.4, 0.2]])}
_DU = ([[0.5, -0.3], [-0.4, 0.6], [0.2, 0.2]],
       [[-0.6, 0.4], [0.3, -0.5], [-0.2, 0.7]],
       [[0.4, 0.5], [-0.5, -0.2], [0.6, -0.4]])
FAR_STRETCH, FAR = (5, 8), 50.0        # s_2: the tracked outputs' set points far outside the bounds at the steps 5, 6, 7


@functools.lru_cache(maxsize=None)
def problem(which, noise=False):
    import mpc_code_amd
    ex, over = EXAMPLES[which]
    if noise:      # the three noise matrices of tests/lin_noise_ref.py on top (the draws of noise_seed = 7 are its own)
        return lnr.with_noise(mpc_code_amd, ex, **(over or {}))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mpc_code_amd.load_problem(mpc_code_amd.example_path(ex), overrides=over)


def start_states(which, nb=B):
    return lnr.start_states("wb" if which == "wb" else "cstr", nb)


def schedule(which, j, n=NSTEPS, shift=0, p=None):
    """(ysp [n, ny], usp [n, nu]) of s_j; shift: every change that many steps later; p: another problem of the same dimensions (the soft CSTR, the CSTR with
    def_px / def_py), whose own schedule the steps are added to"""
    p = problem(which) if p is None else p
    s = p.schedules(n)
    ysp, usp = np.array(s["ysp"][:n], dtype=np.float64), np.array(s["usp"][:n], dtype=np.float64)
    dy = np.asarray(_DY["wb" if which == "wb" else "cstr"][j]); du = np.asarray(_DU[j])
    for i, k in enumerate(CHANGES):
        lo, hi = k + shift, (CHANGES[i + 1] + shift if i + 1 < len(CHANGES) else n)
        ysp[lo:hi] += dy[i]; usp[lo:hi] += du[i]
    if j == 2:
        ysp[FAR_STRETCH[0] + shift:FAR_STRETCH[1] + shift] += FAR * (np.asarray(_DY["wb" if which == "wb" else "cstr"][0][0]) != 0)
    return ysp, usp


def shared_sched(which, j, n=NSTEPS):
    """the example's schedule dict with s_j in it: what a plain shared-schedule run of the whole batch on s_j is given"""
    p = problem(which)
    ysp, usp = schedule(which, j, n)
    return dict({k: np.array(a[:n]) for k, a in p.schedules(n).items()}, ysp=ysp, usp=usp)


@functools.lru_cache(maxsize=None)
def _arrays(which, nb, n):
    s = [schedule(which, j, n) for j in range(3)]
    ysp = np.stack([s[b % 3][0] for b in range(nb)], axis=1); usp = np.stack([s[b % 3][1] for b in range(nb)], axis=1)
    ysp.setflags(write=False); usp.setflags(write=False)
    return ysp, usp


def arrays(which, nb=B, n=NSTEPS):
    """(ysp [n, nb, ny], usp [n, nb, nu]): instance b tracks s_{b mod 3}; read-only, shared"""
    return _arrays(which, nb, n)


def arrays_for(p, which, nb, n):
    """the same for another problem ``p`` of ``which``'s dimensions"""
    s = [schedule(which, j, n, p=p) for j in range(3)]
    return np.stack([s[b % 3][0] for b in range(nb)], axis=1), np.stack([s[b % 3][1] for b in range(nb)], axis=1)


def c_loops(oc, p, n, x0, xm, ysp=None, usp=None, v=None, w=None):
    """the C restatement instance by instance, each with its own rows as the schedule (and its own noise folded in, as lin_noise_ref does); logs [n, B, .]"""
    s0 = {k: np.array(a[:n]) for k, a in p.schedules(n).items()}
    o = oc.OracleC(p)
    runs = []
    for b in range(len(x0)):
        s = dict(s0)
        if ysp is not None:
            s["ysp"] = np.ascontiguousarray(ysp[:n, b])
        if usp is not None:
            s["usp"] = np.ascontiguousarray(usp[:n, b])
        if v is not None:
            s["pyp"] = s0["pyp"] + v[:n, b]
        if w is not None:
            s["pxp"] = s0["pxp"] + w[:n, b]
        r = o.closed_loop(n, x0[b:b + 1], xm[b:b + 1], sched=s, nthreads=1)
        runs.append({k: a for k, a in r.items() if k != "final"})
    return {k: np.concatenate([r[k] for r in runs], axis=1) for k in runs[0]}


def np_loop(p, n, x0, xm, ysp=None, usp=None):
    """the NumPy restatement for the whole batch at once: sched["ysp"][k] is [B, ny]"""
    import riccati_np as rn
    s = {k: np.array(a[:n]) for k, a in p.schedules(n).items()}
    if ysp is not None:
        s["ysp"] = np.asarray(ysp[:n])
    if usp is not None:
        s["usp"] = np.asarray(usp[:n])
    with np.errstate(all="ignore"):
        return rn.closed_loop_batch(p, n, x0, xm, sched=s)


_c = {}


def c_reference(oc, which, mode="yu"):
    """the per-instance C loops of the shared inputs, once per process, read-only.  mode: "yu" both arrays, "y" / "u" one alone, "yuvw": both, together with
    both noises of noise_seed = 7 (on the problem with the noise matrices)"""
    if (which, mode) not in _c:
        noisy = "v" in mode
        p, x0 = problem(which, noisy), start_states(which)
        ysp, usp = arrays(which)
        v, w = (None, None)
        if noisy:
            from mpc_code_amd.noise import loop_noise
            v, w = loop_noise(p, NSTEPS, B, lnr.SEED)
        r = c_loops(oc, p, NSTEPS, x0, x0, ysp if "y" in mode else None, usp if "u" in mode else None, v, w)
        for a in r.values():
            a.setflags(write=False)
        _c[which, mode] = r
    return _c[which, mode]
