"""Reference of the non-linear tracking loop with white noise on measurement AND plant state (MPC_code.py:537-541, 822-827), without a GPU and without
touching oracle/: nmpc_oracle.closed_loop run instance by instance on a shallow copy of the oracle problem whose def_pxp is a closure returning
pxp_k + w_k[b] - the algebraic slot of a state noise, x_p <- Fx_p + (pxp_k + w_k) - with v_wn = v[:, b].  tests/test_nmpc_lin_host.py checks this
reference itself; tests/test_nmpc_state_noise.py checks the kernels against it.
"""
import copy

import numpy as np

LOGS = ("U", "X_HAT", "XS", "US", "Xp", "D_HAT")
ILOGS = ("STATUS_DYN", "STATUS_SS", "SQP_DYN", "SQP_SS")


def with_state_noise(p, w_b):
    """A shallow copy of the oracle problem ``p`` whose plant disturbance schedule carries w_b [nsteps, nxp] of one instance on top of its own."""
    q = copy.copy(p)
    own, h = p.def_pxp, p.h
    w_b = np.asarray(w_b, dtype=np.float64)

    def def_pxp(t):
        k = int(round(t / h))
        base = np.zeros(p.nxp) if own is None else np.ravel(own(t)[0])
        return [base + w_b[k]]
    q.def_pxp = def_pxp
    return q


def closed_loop(p, nsteps, x0_p, x0_m, v=None, w=None, max_sqp=1, sqp_tol=1e-9):
    """The batch [B, .] run by the oracle, instance by instance; v [nsteps, B, ny], w [nsteps, B, nxp] or None.  Logs [nsteps, B, dim]."""
    import nmpc_oracle as no
    runs = []
    for b in range(len(x0_p)):
        q = p if w is None else with_state_noise(p, w[:, b])
        runs.append(no.closed_loop(q, nsteps, x0_p=x0_p[b], x0_m=x0_m[b], max_sqp=max_sqp, sqp_tol=sqp_tol, v_wn=None if v is None else v[:, b]))
    out = {k: np.stack([r[k] for r in runs], axis=1) for k in LOGS + ILOGS}
    for k in ILOGS:
        out[k] = out[k].astype(np.int32)
    return out
