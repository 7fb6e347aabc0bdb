"""Family member d42 (tests/nmpc_family.py): four states, two inputs, two outputs, two disturbances - two pairs of vessels given as a
SAMPLED map (User_fxm_Dis) with quadratic and bilinear terms.  Extended Kalman filter on the discrete map (its Jacobians are the
map's own), linear disturbance model (offree = "lin": Bd in the model, Cd on the output rows), a terminal weight with an off-diagonal
term, every bound finite: a full tile with two inputs on the unmasked tables.  The plant's coefficients are not the model's.  Written
for this project in the Ex-file surface.
"""
from casadi import *
import numpy as np
import scipy.linalg as scla

Nsim, N, h = 40, 9, 1.0

xp = SX.sym("xp", 4)
x = SX.sym("x", 4)
u = SX.sym("u", 2)
y = SX.sym("y", 2)
d = SX.sym("d", 2)


def _map(s, v, a00, a22):
    nxt = SX(4, 1)
    nxt[0] = a00 * s[0] + 0.10 * s[2] - 0.05 * s[0] * s[0] + 0.25 * v[0]
    nxt[1] = 0.10 * s[0] + 0.75 * s[1] + 0.05 * s[0] * s[1]
    nxt[2] = a22 * s[2] + 0.05 * s[3] - 0.03 * s[2] * s[2] + 0.20 * v[1]
    nxt[3] = 0.10 * s[1] + 0.10 * s[2] + 0.70 * s[3]
    return nxt


def User_fxp_Dis(x, t, u, pxp, pxmp):
    return _map(x, u, 0.78, 0.83)


def User_fxm_Dis(x, u, d, t, px):
    return _map(x, u, 0.80, 0.85)


def User_fyp(x, u, t, pyp, pymp):
    return vertcat(x[1], x[3])


def User_fym(x, u, d, t, py):
    return vertcat(x[1], x[3])


offree = "lin"
Bd = np.array([[0.10, 0.00], [0.00, 0.00], [0.00, 0.10], [0.02, 0.00]])
Cd = np.array([[0.30, 0.00], [0.10, 0.40]])

x0_p = np.array([0.70, 0.33, 0.55, 0.29])
x0_m = np.array([0.70, 0.33, 0.55, 0.29])
u0 = np.array([0.40, 0.40])
dhat0 = np.array([0.0, 0.0])

ekf = True
Q_kf = scla.block_diag(1.0e-5 * np.eye(4), 1.0e-2 * np.eye(2))
R_kf = 1.0e-4 * np.eye(2)
P0 = 1.0e-2 * np.eye(6)


def defSP(t):
    ysp = np.array([0.33, 0.29]) if t <= 4.5 else np.array([0.50, 0.38])
    return [ysp, np.array([0.0, 0.0]), np.zeros(4)]


umin = np.array([0.0, 0.0])
umax = np.array([0.8, 0.9])
xmin = np.array([-0.2, -0.2, -0.2, -0.2])
xmax = np.array([0.95, 1.5, 1.5, 1.5])
ymin = np.array([-0.5, -0.5])
ymax = np.array([2.0, 2.0])

Qss = np.diag([2.0, 1.0])
Rss = 1.0e-3 * np.eye(2)
Q = np.diag([0.1, 2.0, 0.1, 1.0])
R = np.diag([0.05, 0.05])


def User_vfin(x, xs):
    return 1.0 * x[0] * x[0] + 4.0 * x[1] * x[1] + 1.0 * x[2] * x[2] + 3.0 * x[3] * x[3] + 1.5 * x[1] * x[3]
