"""The draws of the reference's white noises (``MPC_code.py:537-541, 822-827``), shared by the paths whose loops carry both of them: the
linear path (:mod:`driver`) and the economic path (:mod:`enmpc`, which re-exports :func:`loop_noise` under its own name)."""
from __future__ import annotations

import numpy as np


def loop_noise(problem, nsteps: int, B: int, seed: int):
    """The draws of the reference's white noises for nsteps x B instances from ``numpy.random.default_rng(seed)``: ``V_WN`` = sqrtm(R_wn) N(0, I) on the measurement
    (MPC_code.py:537-541) and ``W_WN`` = G_wn sqrtm(Q_wn) N(0, I) on the plant state after its step (:822-827) - None where the example does not define them.  Per step
    first the measurement's draws, then the state's."""
    def root(S):
        ev, evec = np.linalg.eigh(0.5 * (S + S.T))      # the symmetric square root scipy.linalg.sqrtm returns for a covariance
        return (evec * np.sqrt(np.maximum(ev, 0.0))) @ evec.T
    p, rng = problem, np.random.default_rng(seed)
    if getattr(p, "R_wn", None) is None and getattr(p, "G_wn", None) is None:
        raise ValueError("noise_seed: the example defines neither R_wn nor G_wn / Q_wn")
    Rv = None if p.R_wn is None else root(p.R_wn)
    Gw = None if p.G_wn is None else p.G_wn @ root(p.Q_wn)
    V, W = [], []
    for _ in range(nsteps):
        if Rv is not None:
            V.append(rng.standard_normal((B, p.ny)) @ Rv.T)
        if Gw is not None:
            W.append(rng.standard_normal((B, Gw.shape[1])) @ Gw.T)      # (one draw per noise component: nxp of them where G_wn is square)
    return (np.stack(V) if V else None), (np.stack(W) if W else None)
