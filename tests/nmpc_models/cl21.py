"""Family member cl21 (tests/nmpc_lin_family.py): two states, one input, two outputs (the states), two disturbances - a CONTINUOUS model
with a quadratic and a bilinear term and the LINEAR disturbance model (offree = "lin"): the model step is RK4 of the right-hand side, then
+ Bd d; the output is x + Cd d.  Extended Kalman filter whose covariance feels Bd (P0 and the disturbance part of Q_kf are large next to
the state part: G = Bd moves the gain within a few steps).  The plant's coefficients are not the model's.  Its twin cl21sf states the same
problem with StateFeedback = True.  Written for this project in the Ex-file surface.
"""
from casadi import *
import numpy as np
import scipy.linalg as scla

Nsim, N, h = 40, 6, 0.5

xp = SX.sym("xp", 2)
x = SX.sym("x", 2)
u = SX.sym("u", 1)
y = SX.sym("y", 2)
d = SX.sym("d", 2)

Mx = 4


def _rhs(s, v, a, b):
    return vertcat(-a * s[0] + 0.3 * s[1] - 0.2 * s[0] * s[0] + v[0],
                   0.5 * s[0] - b * s[1] + 0.1 * s[0] * s[1])


def User_fxp_Cont(x, t, u, pxp, pxmp):
    return _rhs(x, u, 1.06, 0.76)


def User_fyp(x, u, t, pyp, pymp):
    return vertcat(x[0], x[1])


def User_fxm_Cont(x, u, d, t, px):
    return _rhs(x, u, 1.0, 0.8)


def User_fym(x, u, d, t, py):
    return vertcat(x[0], x[1])


offree = "lin"
Bd = np.array([[0.20, 0.00], [0.05, 0.15]])
Cd = np.array([[0.30, 0.00], [0.10, 0.40]])

x0_p = np.array([0.45, 0.30])
x0_m = np.array([0.45, 0.30])
u0 = np.array([0.40])
dhat0 = np.array([0.0, 0.0])

ekf = True
Q_kf = scla.block_diag(1.0e-5 * np.eye(2), 2.0e-2 * np.eye(2))
R_kf = 1.0e-4 * np.eye(2)
P0 = scla.block_diag(1.0e-3 * np.eye(2), 5.0e-2 * np.eye(2))


def defSP(t):
    ysp = np.array([0.45, 0.30]) if t <= 2.2 else np.array([0.60, 0.41])
    return [ysp, np.array([0.40]), np.zeros(2)]


umin = np.array([0.0])
umax = np.array([0.62])
xmin = np.array([0.0, 0.0])
xmax = np.array([2.0, 2.0])

Qss = np.diag([5.0, 2.0])
Rss = 1.0e-3 * np.eye(1)
Q = np.diag([2.0, 1.0])
R = np.diag([0.02])
