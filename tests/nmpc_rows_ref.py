"""Test-side restatement of the non-linear tracking OCP with user inequality rows (``User_g_ineq(x, u, y, d, t, px, py) <= 0`` at the stages
k = 0..N-1, reference Control_Calc.py:94-100,132-147; MPC_code.py:306-314), built from the unchanged functions of oracle/nmpc_oracle.py.

* the Ex-file is read by the oracle's own loader (``nmpc_oracle.load_problem`` -> ``exnum.load``); the rows are the user function called on numbers,
  with y = Fy_model(x, u, d, t) (``model_fy``) and px = py = 0 - nothing of the product's loader, tracer or generated code;
* their Jacobians are central differences (``nmpc_oracle._fd``);
* each SQP iteration is the oracle's dense QP (``ocp_qp_ltv``) with the rows of stages 0..N-1, linearised at the iterate, appended to G with the
  bounds (-inf, -(g - Gx x - Gu u)], solved by ``qp_ipm_dense`` and polished by ``qp_polish``;
* the loop is the oracle's ``closed_loop`` (the same cold start, shift and hold rules) with this OCP.  One rule is the device's: after a step whose
  OCP was infeasible the next OCP starts from the first guess again, (x, u) of the model state before the measurement update and the held input in
  every stage - the oracle would keep the trajectory of the step before that;
* ``kkt_rows`` is ``kkt_nlp``'s certificate with the rows: their finite-difference Jacobians join the active constraints of the stationarity fit.
"""
from __future__ import annotations

import numpy as np

import exnum
import mpc_oracle as o
import nmpc_oracle as no

STATUS_SOLVED, STATUS_MAXITER, STATUS_INFEASIBLE = no.STATUS_SOLVED, no.STATUS_MAXITER, no.STATUS_INFEASIBLE


def load(path, overrides=None):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = no.load_problem(path, overrides)
        ns = exnum.load(path, overrides)
    p.g_user = ns["User_g_ineq"]
    p.ng = rows(p, p.x0_m, p.u0, p.dhat0).size
    return p


def rows(p, x, u, d, t=0.0):
    """G(x, u, Fy_model(x, u, d, t), d, t, 0, 0): the Ex-file's function on numbers."""
    y = no.model_fy(p, x, u, d, t)
    out = p.g_user(no._sm(x), no._sm(u), no._sm(y), no._sm(d), t, no._sm(np.zeros(p.nx)), no._sm(np.zeros(p.ny)))
    if isinstance(out, (list, tuple)):      # (a list of rows: numbers or one-element containers)
        return np.concatenate([np.asarray(e, dtype=np.float64).ravel() for e in out])
    return np.asarray(out, dtype=np.float64).ravel()


def rows_jac(p, x, u, d, t=0.0):
    J = no._fd(lambda v: rows(p, v[:p.nx], v[p.nx:], d, t), np.concatenate([x, u]))
    return J[:, :p.nx], J[:, p.nx:], rows(p, x, u, d, t)


def _append_rows(p, w, d, t, G, lo, hi):
    n, m, N = p.nx, p.nu, p.N
    nxu = n + m
    R, L, H = [G], [lo], [hi]
    for k in range(N):
        xk, uk = w[nxu * k:nxu * k + n], w[nxu * k + n:nxu * (k + 1)]
        Gx, Gu, gv = rows_jac(p, xk, uk, d, t)
        blk = np.zeros((p.ng, w.size)); blk[:, nxu * k:nxu * k + n] = Gx; blk[:, nxu * k + n:nxu * (k + 1)] = Gu
        R.append(blk); L.append(np.full(p.ng, -np.inf)); H.append(-(gv - Gx @ xk - Gu @ uk))
    return np.vstack(R), np.concatenate(L), np.concatenate(H)


def row_values(p, w, d, t=0.0):
    """g(x_k, u_k) for k = 0..N-1 of an opt_dyn-ordered point, [N, ng]."""
    n, m, N = p.nx, p.nu, p.N
    nxu = n + m
    return np.array([rows(p, w[nxu * k:nxu * k + n], w[nxu * k + n:nxu * (k + 1)], d, t) for k in range(N)])


def ocp_solve(p, xhat, xs, us, d, w_guess, max_sqp=50, tol=1e-9, t=0.0, u_prev=None):
    """nmpc_oracle.ocp_solve with the rows: SQP from ``w_guess``; returns dict(u0, x1, w, status, sqp_iters, step)."""
    n, m, N = p.nx, p.nu, p.N
    nxu = n + m
    w = np.array(w_guess, dtype=np.float64); w[:n] = xhat
    y0 = no.model_fy(p, xhat, us, d, t)
    rl = o.BOUND_RELAX * np.maximum(1.0, np.abs(p.ymin)); rh = o.BOUND_RELAX * np.maximum(1.0, np.abs(p.ymax))
    if np.any(y0 < p.ymin - rl) or np.any(y0 > p.ymax + rh):
        return dict(u0=None, x1=None, w=w, status=STATUS_INFEASIBLE, sqp_iters=0, step=np.inf)
    step = np.inf
    for it in range(max_sqp):
        Ak, Bk, ck = [], [], []
        for k in range(N):
            xk, uk = w[nxu * k:nxu * k + n], w[nxu * k + n:nxu * (k + 1)]
            A, B, _, F = no.linearize(p, xk, uk, d, t)
            Ak.append(A); Bk.append(B); ck.append(F - A @ xk - B @ uk)
        C, _ = no.output_jac(p, xhat, us, d, t)
        e = no.model_fy(p, xhat, us, d, t) - C @ xhat
        H, g, E, ee, G, lo, hi = no.ocp_qp_ltv(p, Ak, Bk, ck, C, e, xhat, xs, us, u_prev)
        G, lo, hi = _append_rows(p, w, d, t, G, lo, hi)
        r = o.qp_ipm_dense(H, g, E, ee, G, lo, hi, tol=1e-11)
        if r["status"] == STATUS_INFEASIBLE:
            return dict(u0=None, x1=None, w=w, status=STATUS_INFEASIBLE, sqp_iters=it, step=step)
        pol = o.qp_polish(H, g, E, ee, G, lo, hi, r["w"], r["z_lo"], r["z_hi"]) if r["status"] == STATUS_SOLVED else None
        wn = pol["w"] if pol is not None else r["w"]
        step = float(np.abs(wn - w).max())
        w = wn
        if step < tol:
            break
    return dict(u0=w[n:n + m].copy(), x1=w[n + m:2 * n + m].copy(), w=w, status=STATUS_SOLVED if step < tol or max_sqp == 1 else STATUS_MAXITER,
                sqp_iters=it + 1, step=step)


def ocp_solve_plain(p, xhat, xs, us, d, w_guess, max_sqp=50, tol=1e-9, t=0.0, u_prev=None):
    """The same OCP without the rows (the oracle's own ocp_solve)."""
    return no.ocp_solve(p, xhat, xs, us, d, w_guess, max_sqp=max_sqp, tol=tol, t=t, u_prev=u_prev)


def kkt_rows(p, w, xhat, xs, us, d, t=0.0, u_prev=None, act_tol=1e-7):
    """kkt_nlp's certificate with the rows: dynamics defects, the least-squares stationarity residual with the active bounds AND the active rows
    (within act_tol of zero; Jacobians by central differences), the largest bound violation and the largest row value."""
    n, m, N = p.nx, p.nu, p.N
    nxu = n + m
    defect = 0.0
    Ak, Bk = [], []
    for k in range(N):
        xk, uk = w[nxu * k:nxu * k + n], w[nxu * k + n:nxu * (k + 1)]
        A, B, _, F = no.linearize(p, xk, uk, d, t)
        Ak.append(A); Bk.append(B)
        defect = max(defect, np.abs(F - w[nxu * (k + 1):nxu * (k + 1) + n]).max())
    C, _ = no.output_jac(p, xhat, us, d, t)
    e = no.model_fy(p, xhat, us, d, t) - C @ xhat
    H, g, E, ee, G, lo, hi = no.ocp_qp_ltv(p, Ak, Bk, [np.zeros(n)] * N, C, e, xhat, xs, us, u_prev)
    grad = H @ w + g
    Gw = G @ w
    act = (np.abs(Gw - lo) < act_tol) | (np.abs(Gw - hi) < act_tol)
    gv = row_values(p, w, d, t)
    J = []
    for k in range(N):
        xk, uk = w[nxu * k:nxu * k + n], w[nxu * k + n:nxu * (k + 1)]
        Gx, Gu, _ = rows_jac(p, xk, uk, d, t)
        for i in range(p.ng):
            if abs(gv[k, i]) < act_tol:
                r = np.zeros(w.size); r[nxu * k:nxu * k + n] = Gx[i]; r[nxu * k + n:nxu * (k + 1)] = Gu[i]
                J.append(r)
    M = np.vstack([E, G[act]] + ([np.array(J)] if J else [])).T
    lam = np.linalg.lstsq(M, -grad, rcond=None)[0]
    return dict(defect=defect, stationarity=float(np.abs(grad + M @ lam).max()), n_active=int(act.sum()), n_rows_active=len(J),
                bound_violation=float(max(0.0, (lo - Gw).max(initial=0.0), (Gw - hi).max(initial=0.0))), row_max=float(gv.max()))


def closed_loop(p, nsteps, x0_p=None, x0_m=None, max_sqp=50, sqp_tol=1e-9):
    """nmpc_oracle.closed_loop with the rows (logs: U, X_HAT, XS, US, Xp, D_HAT, STATUS_DYN, STATUS_SS, SQP_DYN, ROW0: g at stage 0 of every step)."""
    n, m, N = p.nx, p.nu, p.N
    nxu = n + m
    x = np.array(p.x0_p if x0_p is None else x0_p, dtype=np.float64)
    xhat = np.array(p.x0_m if x0_m is None else x0_m, dtype=np.float64)
    u = p.u0.copy(); dhat = p.dhat0.copy(); Pk = p.P0.copy()
    lue = getattr(p, "estimator", "ekf") == "lue"
    xs, us = xhat.copy(), u.copy()
    sched = p.schedules(nsteps)
    w = None
    L = {k: [] for k in ("U", "X_HAT", "XS", "US", "Xp", "D_HAT", "STATUS_DYN", "STATUS_SS", "SQP_DYN", "SQP_SS", "ROW0", "W")}
    for k in range(nsteps):
        t = k * p.h
        L["Xp"].append(x.copy()); L["X_HAT"].append(xhat.copy())
        if w is None:                                                          # first guess (MPC_code.py:740-756)
            w = np.concatenate([np.tile(np.concatenate([xhat, u]), N), xhat])
        y = no.plant_fy(p, x, u, t, sched["pyp"][k])
        if lue:
            xi = np.concatenate([xhat, dhat]) + p.K @ (y - no.model_fy(p, xhat, u, dhat, t))
        else:
            xi, Pk = no.ekf(p, np.concatenate([xhat, dhat]), Pk, y, u, t)
        xhat, dhat = xi[:n].copy(), xi[n:].copy()
        if p.dmin is not None:
            dhat = np.minimum(np.maximum(dhat, p.dmin), p.dmax)
        L["D_HAT"].append(dhat.copy())
        us_prev, xs_prev = us.copy(), xs.copy()
        tg = no.target_solve(p, sched["usp"][k], sched["ysp"][k], dhat, xs, us, t=t, us_prev=us_prev)
        if tg["status"] != STATUS_INFEASIBLE:
            xs, us = tg["xs"], tg["us"]
        L["XS"].append(xs.copy()); L["US"].append(us.copy()); L["STATUS_SS"].append(tg["status"]); L["SQP_SS"].append(tg["sqp_iters"])
        r = ocp_solve(p, xhat, xs, us, dhat, w, max_sqp=max_sqp, tol=sqp_tol, t=t, u_prev=u)
        L["W"].append(r["w"].copy())
        if r["status"] != STATUS_INFEASIBLE:
            L["ROW0"].append(rows(p, xhat, r["u0"], dhat, t))
            u, xhat = r["u0"], r["x1"]
            w = np.concatenate([r["w"][nxu:], us_prev, xs_prev])               # :764
        else:
            L["ROW0"].append(np.full(p.ng, np.nan))
            xhat = no.model_fx(p, xhat, u, dhat, t)                           # :804-805
            w = None                                                           # (the device's rule: the next OCP starts from the first guess)
        L["U"].append(u.copy()); L["STATUS_DYN"].append(r["status"]); L["SQP_DYN"].append(r["sqp_iters"])
        x = no.plant_fx(p, x, u, t, sched["pxp"][k])
    return {k: np.array(v) for k, v in L.items()}
