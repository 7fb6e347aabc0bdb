"""Test infrastructure: the Riccati interior-point iteration of ``oracle/riccati_np.py:rpdip_solve`` restated step by step in
``numpy.longdouble`` (80-bit extended on x86-64, eps 1.1e-19), and the harness that compares a solver's truncated solves with it.

A solve that stops at the iteration limit (status 1) returns its current iterate.  With ``max_iter = j`` that is the iterate after
exactly j iterations: nothing has converged, so an error in one Newton direction is still in the result.  The solvers on the GPU
take the corrector's step length with an approximate reciprocal, the restatements divide exactly, so the step length is fitted, not
compared: ``W_j = R_{j-1} + a_j d_j`` with ``R_{j-1}`` the reference advanced by the fitted ``a_1 .. a_{j-1}`` and ``d_j`` its corrector
direction there.  What is left after the fit is the error of the direction itself.

Same constants, cold start, predictor, centring and corrector as ``rpdip_solve``; the recursions are sequential over the blocks and
vectorised over the instances; the inverse of the m x m matrix Lambda (m <= 2) is written out.  ``dtype=np.float64`` runs the same
statements in double precision (tests/test_wv_direction_ref.py compares that run with ``rpdip_solve`` and the C restatement).
"""
import numpy as np
import scipy.linalg as scla

import riccati_np as rn

EPS64 = float(np.finfo(np.float64).eps)


# ---------------------------------------------------------------------------------------------------------------------------------
# problems and inputs of the truncated-solve tests
# ---------------------------------------------------------------------------------------------------------------------------------
# dimension sets as in MPC_DIM_LIST: (nx, nu, ny, nd, nxp, du_form, general_output_rows)
VGPR_SETS = [(1, 1, 1, 1, 1, 0, 0), (2, 1, 1, 1, 2, 0, 0), (2, 1, 1, 1, 2, 0, 1), (3, 2, 3, 3, 3, 0, 0), (4, 1, 1, 1, 4, 0, 0), (4, 2, 2, 2, 4, 0, 0)]
BUILTIN_SETS = [(2, 1, 1, 1, 2, 1, 0), (3, 2, 2, 2, 3, 1, 0), (5, 2, 2, 2, 5, 0, 0), (4, 2, 2, 2, 4, 1, 0), (8, 2, 2, 2, 8, 0, 0)]
HORIZONS = [2, 3, 4, 5, 6, 7, 33, 64]
K_TRUNC = 4
GENERIC_TILES = ("-DMPC_WV_GENERIC_TILES",)      # build switch: the tile sweeps of every stage size on the generic (builtin) path
# What the fit of the step length may leave of an iterate, and what the fitted step length may differ from the reference's by: four times the
# largest figures of the wave solver / of either solver on an MI355X (tests/test_wv_directions.py, where they are accounted for).
E_WAVE, E_LANE, D_ALPHA = 3.75e-14, 4.16e-14, 4.48e-8
TOL_DIR = 4 * E_WAVE
TOL_ALPHA = 4 * D_ALPHA
ALPHA_CAP = 1e-6      # what a step length may differ by at the most: an approximate reciprocal does not explain more
BATCH = 7      # one full wave of four tiles and one with a dead tile


def set_id(dims):
    return "_".join(str(v) for v in dims)


def direction_problem(dims, N, finite, seed=None):
    """The random problem of tests/test_gpu_fuzz.py:random_problem (same draws in the same order: tests/test_wv_direction_ref.py holds the
    two together) with the horizon given.  ``finite`` True: every state bound finite (with finite input bounds the kernels without
    bound masks); False: the draw's own mix of finite and infinite state bounds, one of them forced infinite and one finite (the
    kernels with bound masks); None: the bounds as drawn.  The set with a general output row is the double integrator of
    tests/conftest.py; a stage with such a row always takes the kernels with bound masks (the row's state is free at the terminal
    stage), so that set has no ``finite`` variant."""
    from mpc_code_amd.problem import LinearMPCProblem
    nx, nu, ny, nd, nxp, du, ng = dims
    if ng:
        from conftest import double_integrator_with_output_row
        assert dims == (2, 1, 1, 1, 2, 0, 1)
        return double_integrator_with_output_row(N=N)
    seed = 9000 + 100 * nx + 10 * nu + du if seed is None else seed
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nx, nx)); A *= rng.uniform(0.6, 1.04) / np.abs(np.linalg.eigvals(A)).max()
    B = rng.standard_normal((nx, nu))
    C = np.eye(ny, nx)
    Bd = 0.3 * rng.standard_normal((nx, nd)); Cd = np.zeros((ny, nd))
    Q = np.diag(rng.uniform(0.05, 2.0, nx)); R = np.diag(rng.uniform(0.05, 1.0, nu))
    P = scla.solve_discrete_are(A, B, Q, R); P = 0.5 * (P + P.T)
    inf = np.inf
    umax = rng.uniform(0.5, 2.0, nu); umin = -rng.uniform(0.5, 2.0, nu)
    hi_on = rng.random(nx) < 0.6; xhi = rng.uniform(1.0, 4.0, nx); lo_on = rng.random(nx) < 0.6; xlo = -rng.uniform(1.0, 4.0, nx)
    xmax = np.where(hi_on, xhi, inf); xmin = np.where(lo_on, xlo, -inf)
    ymax = np.where(rng.random(ny) < 0.5, rng.uniform(1.0, 3.0, ny), inf); ymin = np.where(rng.random(ny) < 0.5, -rng.uniform(1.0, 3.0, ny), -inf)
    if finite:
        xmax, xmin = xhi, xlo
    elif finite is not None:
        xmax[nx - 1] = inf
        if nx > 1:
            xmin[0] = xlo[0]
    y_bounded = bool(np.isfinite(ymax).any() or np.isfinite(ymin).any())
    Ca = np.hstack([C, Cd]); Aa = np.eye(nx + nd); Aa[:nx, :nx] = A; Aa[:nx, nx:] = Bd
    Pe = scla.solve_discrete_are(Aa.T, Ca.T, np.eye(nx + nd) * 0.1, np.eye(ny) * 0.1)
    K = Pe @ Ca.T @ np.linalg.inv(Ca @ Pe @ Ca.T + 0.1 * np.eye(ny))
    return LinearMPCProblem(nx=nx, nu=nu, ny=ny, nd=nd, nxp=nxp, N=N, h=1.0, Nsim=10, A=A, B=B, C=C, Bd=Bd, Cd=Cd,
                            fx_const=np.zeros(nx), fy_const=np.zeros(ny), Ap=A, Bp=B, Cp=C, Q=Q, R=R, DUForm=bool(du), P=P,
                            Qss=np.eye(ny), Rss=np.zeros((nu, nu)), DUssForm=False, umin=umin, umax=umax, xmin=xmin, xmax=xmax, ymin=ymin, ymax=ymax,
                            y_bounded=y_bounded, umin_ss=umin, umax_ss=umax, xmin_ss=xmin, xmax_ss=xmax, ymin_ss=np.full(ny, -inf), ymax_ss=np.full(ny, inf),
                            estimator="kalss", K=K, x0_p=np.zeros(nx), x0_m=np.zeros(nx), u0=np.zeros(nu), dhat0=np.zeros(nd))


def direction_inputs(p, B, seed):
    """(xhat, xs, us, dhat, u_prev) of B instances: well inside the boxes, so that no instance converges or is refused in four iterations."""
    rng = np.random.default_rng(seed)
    scale = np.where(np.isfinite(p.xmax), p.xmax, 3.0)
    xh = rng.uniform(-0.3, 0.3, (B, p.nx)) * scale
    d = 0.05 * rng.standard_normal((B, p.nd))
    if p.y_bounded:
        # bounded outputs are checked at stage 0, where they are given numbers: an instance that fails there is refused before the first
        # iteration.  Halve its state until C xhat + Cd d + const lies inside the output box (by a tenth of the box at least).
        e = p.fy_const + d @ p.Cd.T
        ylo, yhi = np.where(np.isfinite(p.ymin), p.ymin, 0.0), np.where(np.isfinite(p.ymax), p.ymax, 0.0)
        lo = np.where(np.isfinite(p.ymin), ylo + 0.1 * np.abs(ylo), -np.inf); hi = np.where(np.isfinite(p.ymax), yhi - 0.1 * np.abs(yhi), np.inf)
        for _ in range(8):
            y0 = xh @ p.C.T + e
            out = ~np.all((y0 >= lo) & (y0 <= hi), axis=1)
            xh[out] *= 0.5
    xs = 0.1 * rng.standard_normal((B, p.nx)); us = 0.1 * rng.standard_normal((B, p.nu))
    up = rng.uniform(-0.3, 0.3, (B, p.nu))
    return xh, xs, us, d, up


def case_seed(dims, N, finite):
    return 1000003 * (hash_dims(dims) + 1) + 17 * N + int(finite)


def hash_dims(dims):
    h = 0
    for v in dims:
        h = 11 * h + int(v)
    return h


# ---------------------------------------------------------------------------------------------------------------------------------
# the iteration, one step at a time
# ---------------------------------------------------------------------------------------------------------------------------------
def _inv_small(L):
    """Inverse of [B, m, m], m <= 2, written out (np.linalg.inv does not take long double)."""
    m = L.shape[-1]
    if m == 1:
        return 1.0 / L
    assert m == 2, "the wave solver takes nu <= 2"
    a, b, c, d = L[:, 0, 0], L[:, 0, 1], L[:, 1, 0], L[:, 1, 1]
    det = a * d - b * c
    out = np.empty_like(L)
    out[:, 0, 0] = d / det; out[:, 0, 1] = -b / det; out[:, 1, 0] = -c / det; out[:, 1, 1] = a / det
    return out


def _diag(d):
    out = np.zeros(d.shape + (d.shape[-1],), dtype=d.dtype)
    i = np.arange(d.shape[-1])
    out[..., i, i] = d
    return out


class DirectionRef:
    """The iterate (u, z, s, lambda) of B instances and the corrector direction at it.

    ``direction()`` computes the Newton direction of the corrector and the reference's own step length at the current iterate;
    ``advance(alpha)`` takes the step with the given lengths [B] (its own when left out).  ``w()`` / ``dw()`` are the iterate and
    the direction in the layout of ``opt_dyn``'s decision vector [x_0, u_0, ..., x_N]."""

    def __init__(self, p, xhat, xs, us, dhat, u_prev, dtype=np.longdouble, edit=0):
        # edit: a deliberate error of one sweep, restated from the three edits of csrc/mpc_wave.hpp that tests/test_wv_directions.py must
        # fail on (profiles/wv_direction_parity.txt), for the sets whose sweeps run in groups of four blocks (stage state <= 4):
        #   1  K of every block times 1 + 1e-9 before anything uses it;
        #   2  corrector's backward sweep: the N mod 4 blocks after the full groups take the h_z of the block in front of them;
        #   3  both forward sweeps: the du that is stored (not the one carried on) of the last block of every full group times 1 + 1e-9.
        self.p, self.dtype, self.edit = p, dtype, edit
        sd = rn.stage_data(p)
        inst = rn.instance_data(p, sd, xhat, xs, us, dhat, u_prev)
        f = lambda a: np.asarray(a, dtype=dtype)
        self.A, self.Bm, self.Q, self.M, self.R, self.Pf = (f(sd[k]) for k in ("A", "B", "Q", "M", "R", "Pf"))
        n, m, N = sd["n"], sd["m"], sd["N"]
        self.n, self.m, self.N = n, m, N
        self.z0, self.zr, self.ur, self.c = (f(inst[k]) for k in ("z0", "zr", "ur", "c"))
        self.ok0 = inst["ok0"].copy()
        Bsz = self.z0.shape[0]; self.Bsz = Bsz
        nv = m + n
        lo = np.empty((Bsz, N, nv)); hi = np.empty((Bsz, N, nv))
        lo[:, :, :m] = sd["ulo"]; hi[:, :, :m] = sd["uhi"]
        lo[:, :N - 1, m:] = inst["zlo_m"][:, None, :]; hi[:, :N - 1, m:] = inst["zhi_m"][:, None, :]
        lo[:, N - 1, m:] = inst["zlo_e"]; hi[:, N - 1, m:] = inst["zhi_e"]
        self.fl, self.fh = np.isfinite(lo), np.isfinite(hi)
        self.ncon = f((self.fl.sum(axis=(1, 2)) + self.fh.sum(axis=(1, 2))).astype(float))
        self.lo_f = f(np.where(self.fl, lo, 0.0)); self.hi_f = f(np.where(self.fh, hi, 0.0))
        # ---- cold start (in double precision data, as every solver sees it; the arithmetic from here on in dtype)
        ulo, uhi = sd["ulo"], sd["uhi"]
        both = np.isfinite(ulo) & np.isfinite(uhi)
        push = np.where(both, 0.1 * (np.where(both, uhi, 0) - np.where(both, ulo, 0)),
                        0.1 * np.maximum(1.0, np.abs(np.where(np.isfinite(ulo), ulo, np.where(np.isfinite(uhi), uhi, 0)))))
        push, ulo, uhi = f(push), f(ulo), f(uhi)
        u = np.broadcast_to(f(inst["us"])[:, None, :], (Bsz, N, m)).copy()
        u = np.minimum(np.maximum(u, np.where(np.isfinite(ulo), ulo + push, -np.inf)), np.where(np.isfinite(uhi), uhi - push, np.inf))
        self.u = u; self.z = self._simulate(u)
        v = self._v()
        one, zero = f(1.0), f(0.0)
        self.s_lo = np.where(self.fl, np.maximum(v - self.lo_f, f(rn.S_MIN)), one); self.s_hi = np.where(self.fh, np.maximum(self.hi_f - v, f(rn.S_MIN)), one)
        self.l_lo = np.where(self.fl, f(rn.MU0) / self.s_lo, zero); self.l_hi = np.where(self.fh, f(rn.MU0) / self.s_hi, zero)
        self.it = 0
        self.gscale = None
        self.stall = np.zeros(Bsz, dtype=np.int64)
        self.active = self.ok0.copy()
        self._dir = None

    def _simulate(self, u):
        z = np.empty((self.Bsz, self.N + 1, self.n), dtype=self.dtype); z[:, 0] = self.z0
        for k in range(self.N):
            z[:, k + 1] = z[:, k] @ self.A.T + u[:, k] @ self.Bm.T + self.c
        return z

    def _v(self):
        return np.concatenate([self.u, self.z[:, 1:]], axis=2)

    # -- the iterate in the layout of the solvers' w
    def _pack(self, z, u):
        nx, nu, N = self.p.nx, self.p.nu, self.N
        out = np.zeros((self.Bsz, (N + 1) * nx + N * nu), dtype=self.dtype)
        for k in range(N + 1):
            out[:, k * (nx + nu):k * (nx + nu) + nx] = z[:, k, :nx]
            if k < N:
                out[:, k * (nx + nu) + nx:(k + 1) * (nx + nu)] = u[:, k]
        return out

    def w(self):
        return self._pack(self.z, self.u)

    def dw(self):
        return self._pack(self._dir["d_z"], self._dir["d_u"])

    def residuals(self):
        """(res_p, mu) of the current iterate: the largest bound residual and the mean of slack times multiplier."""
        v = self._v()
        r_lo = np.where(self.fl, v - self.s_lo - self.lo_f, 0.0); r_hi = np.where(self.fh, v + self.s_hi - self.hi_f, 0.0)
        mu = ((self.s_lo * self.l_lo).sum(axis=(1, 2)) + (self.s_hi * self.l_hi).sum(axis=(1, 2))) / np.maximum(self.ncon, 1.0)
        res_p = np.maximum(np.abs(r_lo).max(axis=(1, 2)), np.abs(r_hi).max(axis=(1, 2)))
        return res_p, mu

    def residual_scale(self):
        """Size of the terms a bound residual v -+ s - bound is the difference of, per instance: its rounding floor is eps times this."""
        v = np.abs(self._v())
        t = np.maximum(np.where(self.fl, v + self.s_lo + np.abs(self.lo_f), 0.0), np.where(self.fh, v + self.s_hi + np.abs(self.hi_f), 0.0))
        return np.maximum(1.0, t.max(axis=(1, 2))).astype(np.float64)

    def direction(self):
        """Verdict of the current iterate (as rpdip_solve takes it before a step), then factorisation, predictor, centring, corrector.
        Returns ``alpha_ref`` [B].  ``self.active`` afterwards: the instances that neither converged nor were refused so far."""
        f = lambda a: np.asarray(a, dtype=self.dtype)
        A, Bm, Q, M, R, Pf = self.A, self.Bm, self.Q, self.M, self.R, self.Pf
        n, m, N, Bsz = self.n, self.m, self.N, self.Bsz
        u, z, s_lo, s_hi, l_lo, l_hi, fl, fh = self.u, self.z, self.s_lo, self.s_hi, self.l_lo, self.l_hi, self.fl, self.fh
        v = self._v()
        r_lo = np.where(fl, v - s_lo - self.lo_f, 0.0); r_hi = np.where(fh, v + s_hi - self.hi_f, 0.0)
        mu = ((s_lo * l_lo).sum(axis=(1, 2)) + (s_hi * l_hi).sum(axis=(1, 2))) / np.maximum(self.ncon, 1.0)
        sig = l_lo / s_lo + l_hi / s_hi
        dl = l_hi - l_lo
        dz = z - self.zr[:, None, :]; du = u - self.ur[:, None, :]
        gz = np.empty((Bsz, N + 1, n), dtype=self.dtype); gu = np.empty((Bsz, N, m), dtype=self.dtype)
        gz[:, :N] = dz[:, :N] @ Q.T + du @ M.T
        gz[:, N] = dz[:, N] @ Pf.T
        gu[:] = du @ R.T + dz[:, :N] @ M
        gz[:, 1:] += dl[:, :, m:]; gu += dl[:, :, :m]
        pi = gz[:, N].copy(); r_u = np.empty((Bsz, N, m), dtype=self.dtype)
        for k in range(N - 1, -1, -1):
            r_u[:, k] = gu[:, k] + pi @ Bm
            pi = gz[:, k] + pi @ A
        if self.gscale is None:
            self.gscale = np.maximum(1.0, np.abs(r_u).max(axis=(1, 2)))
        res_s = np.abs(r_u).max(axis=(1, 2)); res_p = np.maximum(np.abs(r_lo).max(axis=(1, 2)), np.abs(r_hi).max(axis=(1, 2)))
        comp = lambda s, l: np.minimum(np.minimum(s, l) / rn.TOL_C, s * l / rn.TOL_MU)
        cres = np.maximum(comp(s_lo, l_lo).max(axis=(1, 2)), comp(s_hi, l_hi).max(axis=(1, 2)))
        ok_cp = (cres <= 1.0) & (res_p <= rn.TOL_FEAS)
        self.stall = np.where(ok_cp, self.stall + 1, 0)
        conv = ok_cp & ((res_s <= rn.TOL_STAT * self.gscale) | ((self.stall > rn.STALL_MAX) & (res_s <= rn.TOL_STAT_ACC * self.gscale)))
        lmax = np.maximum(l_lo.max(axis=(1, 2)), l_hi.max(axis=(1, 2)))
        bad = (lmax > rn.INFEAS_Z * self.gscale) | ~np.isfinite(mu)
        self.active = self.active & ~conv & ~bad
        # ---- factorisation
        K = np.empty((Bsz, N, m, n), dtype=self.dtype); Linv = np.empty((Bsz, N, m, m), dtype=self.dtype); Acl = np.empty((Bsz, N, n, n), dtype=self.dtype)
        Pn = np.broadcast_to(Pf, (Bsz, n, n)) + _diag(sig[:, N - 1, m:])
        for k in range(N - 1, -1, -1):
            PB = Pn @ Bm
            Lam = R + _diag(sig[:, k, :m]) + Bm.T @ PB
            Psi = M.T + np.swapaxes(PB, 1, 2) @ A
            Li = _inv_small(Lam)
            Linv[:, k] = Li
            K[:, k] = -Li @ Psi
            if self.edit == 1:
                K[:, k] = K[:, k] * f(1.0 + 1e-9)
            Acl[:, k] = A + Bm @ K[:, k]
            if k > 0:
                Kk = K[:, k]; Rt = R + _diag(sig[:, k, :m])
                MK = M @ Kk
                Pn = (Q + _diag(sig[:, k - 1, m:]) + np.swapaxes(Acl[:, k], 1, 2) @ Pn @ Acl[:, k]
                      + np.swapaxes(Kk, 1, 2) @ Rt @ Kk + MK + np.swapaxes(MK, 1, 2))
                Pn = 0.5 * (Pn + np.swapaxes(Pn, 1, 2))

        def mv(Mx, x):       # [B, i, j] x [B, j] -> [B, i]
            return (Mx @ x[:, :, None])[:, :, 0]

        def mtv(Mx, x):      # [B, j, i]' x [B, j] -> [B, i]
            return (np.swapaxes(Mx, 1, 2) @ x[:, :, None])[:, :, 0]

        rem = N % 4      # blocks after the full groups of four (the sweeps of a one-tile stage)

        def solve(rc_lo, rc_hi, corrector=False):
            h = (-rc_hi + l_hi * r_hi) / s_hi + (rc_lo + l_lo * r_lo) / s_lo
            qz = gz.copy(); qu = gu.copy()
            qz[:, 1:] += h[:, :, m:]; qu += h[:, :, :m]
            kff = np.empty((Bsz, N, m), dtype=self.dtype)
            shifted = lambda kb: self.edit == 2 and corrector and 0 <= kb < rem      # block kb reads the h_z of block kb - 1 (block 0: the guard cells, zero)
            pv = (qz[:, N - 1] if N > 1 else 0.0 * qz[:, N]) if shifted(N - 1) else qz[:, N].copy()
            for k in range(N - 1, -1, -1):
                psi = qu[:, k] + pv @ Bm
                kff[:, k] = -mv(Linv[:, k], psi)
                hz = (qz[:, k - 1] if k > 1 else 0.0 * qz[:, k]) if shifted(k - 1) else qz[:, k]
                pv = hz + mtv(Acl[:, k], pv) + mtv(K[:, k], qu[:, k])
            d_z = np.zeros((Bsz, N + 1, n), dtype=self.dtype); d_u = np.empty((Bsz, N, m), dtype=self.dtype)
            for k in range(N):
                d_u[:, k] = mv(K[:, k], d_z[:, k]) + kff[:, k]
                d_z[:, k + 1] = d_z[:, k] @ A.T + d_u[:, k] @ Bm.T
            if self.edit == 3:
                for k in range(3, N - rem, 4):
                    d_u[:, k] = d_u[:, k] * f(1.0 + 1e-9)
            dv = np.concatenate([d_u, d_z[:, 1:]], axis=2)
            ds_hi = np.where(fh, -r_hi - dv, 0.0); ds_lo = np.where(fl, r_lo + dv, 0.0)
            dl_hi = np.where(fh, (-rc_hi - l_hi * ds_hi) / s_hi, 0.0)
            dl_lo = np.where(fl, (-rc_lo - l_lo * ds_lo) / s_lo, 0.0)
            return d_u, d_z, ds_lo, ds_hi, dl_lo, dl_hi

        def maxstep(xs_, dxs_, cap):
            out = np.full(Bsz, cap, dtype=self.dtype)
            for x_, d_ in zip(xs_, dxs_):
                with np.errstate(divide="ignore", invalid="ignore"):
                    r = np.where(d_ < 0, -x_ / np.where(d_ < 0, d_, -1.0), np.inf)
                out = np.minimum(out, r.min(axis=(1, 2)))
            return out

        d_u, d_z, ds_lo, ds_hi, dl_lo, dl_hi = solve(np.where(fl, s_lo * l_lo, 0.0), np.where(fh, s_hi * l_hi, 0.0))
        a_aff = maxstep((s_lo, s_hi, l_lo, l_hi), (ds_lo, ds_hi, dl_lo, dl_hi), 1.0)
        aa = a_aff[:, None, None]
        mu_aff = (((s_lo + aa * ds_lo) * (l_lo + aa * dl_lo)).sum(axis=(1, 2)) + ((s_hi + aa * ds_hi) * (l_hi + aa * dl_hi)).sum(axis=(1, 2))) / np.maximum(self.ncon, 1.0)
        sigma = np.where(mu > 0, (mu_aff / np.where(mu > 0, mu, 1.0)) ** 3, 0.0)
        sm = np.maximum(sigma * mu, f(rn.MU_FLOOR))[:, None, None]
        d_u, d_z, ds_lo, ds_hi, dl_lo, dl_hi = solve(
            np.where(fl, s_lo * l_lo - np.maximum(sm, l_lo * f(rn.S_FLOOR)) + ds_lo * dl_lo, 0.0),
            np.where(fh, s_hi * l_hi - np.maximum(sm, l_hi * f(rn.S_FLOOR)) + ds_hi * dl_hi, 0.0), corrector=True)
        alpha = np.minimum(1.0, f(rn.TAU) * maxstep((s_lo, s_hi, l_lo, l_hi), (ds_lo, ds_hi, dl_lo, dl_hi), np.inf))
        self._dir = dict(d_u=d_u, d_z=d_z, ds_lo=ds_lo, ds_hi=ds_hi, dl_lo=dl_lo, dl_hi=dl_hi, alpha=alpha, res=np.stack([res_s, res_p, mu], axis=1))
        return alpha

    def advance(self, alpha=None):
        d = self._dir
        a = d["alpha"] if alpha is None else np.asarray(alpha, dtype=self.dtype)
        a = a[:, None, None]
        # size of the terms the new iterate's residuals are made of: the bound residuals are (1 - alpha) times the old ones, the mean of
        # slack times multiplier a sum of products (s + alpha ds)(l + alpha dl) - each as small as the step makes it, and known no
        # better than the step length times these
        self.res_p_size = d["res"][:, 1].astype(np.float64)
        self.mu_size = ((((np.abs(self.s_lo) + a * np.abs(d["ds_lo"])) * (np.abs(self.l_lo) + a * np.abs(d["dl_lo"]))).sum(axis=(1, 2))
                         + ((np.abs(self.s_hi) + a * np.abs(d["ds_hi"])) * (np.abs(self.l_hi) + a * np.abs(d["dl_hi"]))).sum(axis=(1, 2)))
                        / np.maximum(self.ncon, 1.0)).astype(np.float64)
        self.u = self.u + a * d["d_u"]; self.z = self.z + a * d["d_z"]
        self.s_lo = self.s_lo + a * d["ds_lo"]; self.s_hi = self.s_hi + a * d["ds_hi"]
        self.l_lo = self.l_lo + a * d["dl_lo"]; self.l_hi = self.l_hi + a * d["dl_hi"]
        self.it += 1
        self._dir = None


def reference_iterations(p, xhat, xs, us, dhat, u_prev, K, dtype=np.longdouble, alphas=None):
    """K iterations.  Per iteration j = 1..K a dict: ``R`` the iterate before the step (w layout) with ``s_lo, s_hi, l_lo, l_hi``, ``d`` the
    corrector direction (w layout), ``alpha_ref`` the reference's own step length there, ``alpha`` the one taken (``alphas[j-1]`` where given),
    ``res_p`` / ``mu`` of the new iterate, ``active`` the instances that had not stopped before the step.  ``final``: the last iterate."""
    ref = DirectionRef(p, xhat, xs, us, dhat, u_prev, dtype=dtype)
    out = []
    for j in range(1, K + 1):
        a_ref = ref.direction()
        rec = dict(R=ref.w(), d=ref.dw(), alpha_ref=a_ref, active=ref.active.copy(), s_lo=ref.s_lo, s_hi=ref.s_hi, l_lo=ref.l_lo, l_hi=ref.l_hi)
        a = a_ref if alphas is None or len(alphas) < j else np.asarray(alphas[j - 1], dtype=dtype)
        ref.advance(a)
        rec["alpha"] = a
        rec["res_p"], rec["mu"] = ref.residuals()
        rec["res_p_size"], rec["mu_size"], rec["res_floor"] = ref.res_p_size, ref.mu_size, 8.0 * EPS64 * ref.residual_scale()
        rec["W"] = ref.w()
        out.append(rec)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the harness: truncated solves of a solver against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def fit_step(W, R, d):
    """Per instance the step length a = <W - R, d> / <d, d> and what the fit leaves: max|W - R - a d| / max(1, max|R|, max|d|)."""
    W, R, d = (np.asarray(a, dtype=np.longdouble) for a in (W, R, d))
    a = ((W - R) * d).sum(axis=1) / (d * d).sum(axis=1)
    left = np.abs(W - R - a[:, None] * d).max(axis=1)
    scale = np.maximum(1.0, np.maximum(np.abs(R).max(axis=1), np.abs(d).max(axis=1)))
    return a, (left / scale).astype(np.float64)


def check_truncated(p, inputs, solve_j, K=K_TRUNC):
    """``solve_j(j)`` -> dict(w, status, iters, res) of the solver under test with ``max_iter = j``.  Returns per j the figures the tests
    assert on, each [B]:
      ``resid``   what the fit of the step length leaves of W_j - R_{j-1} (fit_step);
      ``dalpha``  |a_j - alpha_ref_j| / alpha_ref_j;
      ``acond``   what an error of the iterate of one unit of ``resid`` may move the fitted step length by, relative to alpha_ref_j:
                  sqrt(nw) scale / (|d_j|_2 alpha_ref_j);
      ``dres_p``, ``dmu``  error of the call's bound residual res[:, 1] and complementarity res[:, 2] against the reference's at R_j (the
                  reference advanced with a_j), relative to the size of the terms they are made of (DirectionRef.advance): the bound
                  residual is (1 - a_j) times the one before the step, so with a_j near one it is a small difference of two numbers
                  known to the precision of the fit only - relative to its own value nothing is known about it.  The bound residual
                  has the rounding floor 8 eps64 (|v| + |s| + |bound|) of its own evaluation taken off first.
      ``limit``   the call stopped at the iteration limit (status 1, iters == j);  ``ref_active``: so does the reference at j - 1
                  (``ref_active_after`` in the last entry: and at K)."""
    ref = DirectionRef(p, *inputs, dtype=np.longdouble)
    out = []
    for j in range(1, K + 1):
        alpha_ref = ref.direction()
        active = ref.active.copy()
        R, d = ref.w(), ref.dw()
        g = solve_j(j)
        limit = (np.asarray(g["status"]) == 1) & (np.asarray(g["iters"]) == j)
        a, resid = fit_step(g["w"], R, d)
        dalpha = (np.abs(a - alpha_ref) / alpha_ref).astype(np.float64)
        scale = np.maximum(1.0, np.maximum(np.abs(R).max(axis=1), np.abs(d).max(axis=1)))
        acond = (np.sqrt(R.shape[1]) * scale / (np.sqrt((d * d).sum(axis=1)) * alpha_ref)).astype(np.float64)
        ref.advance(a)
        res_p, mu = ref.residuals()
        floor = 8.0 * EPS64 * ref.residual_scale()
        gp, gm = np.asarray(g["res"])[:, 1], np.asarray(g["res"])[:, 2]
        over = np.maximum(np.abs(gp - res_p.astype(np.float64)) - floor, 0.0)
        dres_p = np.where(over > 0.0, over / np.where(over > 0.0, ref.res_p_size, 1.0), 0.0)
        dmu = (np.abs(gm - mu) / ref.mu_size).astype(np.float64)
        out.append(dict(resid=resid, dalpha=dalpha, acond=acond, dres_p=dres_p, dmu=dmu, limit=limit, ref_active=active,
                        alpha=a.astype(np.float64), alpha_ref=alpha_ref.astype(np.float64)))
    ref.direction()
    out[-1]["ref_active_after"] = ref.active.copy()
    return out
