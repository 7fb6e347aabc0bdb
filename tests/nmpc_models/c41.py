"""Family member c41 (tests/nmpc_family.py): four states, ONE input, one output, one disturbance - four vessels in a row, the first fed
by u and an unknown flow d, two of them with a non-linear outflow.  Continuous model, extended Kalman filter, disturbance inside the
model, the output is the LAST state, upper bounds on the second and the fourth state only (no lower ones): a full tile with a
single-column input and boxes with infinite sides.  The plant's first vessel drains faster than the model's.  Written for this project
in the Ex-file surface.
"""
from casadi import *
import numpy as np
import scipy.linalg as scla

Nsim, N, h = 40, 10, 0.5

xp = SX.sym("xp", 4)
x = SX.sym("x", 4)
u = SX.sym("u", 1)
y = SX.sym("y", 1)
d = SX.sym("d", 1)

Mx = 4


def _chain(s, inflow, drain):
    return vertcat(-drain * s[0] + inflow,
                   s[0] - s[1] - 0.2 * s[1] * s[1],
                   s[1] - s[2],
                   s[2] - s[3] - 0.1 * s[3] * s[3] * s[3])


def User_fxp_Cont(x, t, u, pxp, pxmp):
    return _chain(x, u[0], 1.3)


def User_fyp(x, u, t, pyp, pymp):
    return vertcat(x[3])


def User_fxm_Cont(x, u, d, t, px):
    return _chain(x, u[0] + d[0], 1.2)


def User_fym(x, u, d, t, py):
    return vertcat(x[3])


offree = "nl"

x0_p = np.array([0.50, 0.46, 0.46, 0.45])
x0_m = np.array([0.50, 0.46, 0.46, 0.45])
u0 = np.array([0.60])
dhat0 = np.array([0.0])

ekf = True
Q_kf = scla.block_diag(1.0e-5 * np.eye(4), 1.0e-2 * np.eye(1))
R_kf = 1.0e-4 * np.eye(1)
P0 = 1.0e-2 * np.eye(5)


def defSP(t):
    ysp = np.array([0.45]) if t <= 2.2 else np.array([0.80])
    return [ysp, np.array([0.0]), np.zeros(4)]


umin = np.array([0.0])
umax = np.array([1.6])
xmax = np.array([inf, 0.95, inf, 1.0])

Qss = np.eye(1)
Rss = np.zeros((1, 1))
Q = np.diag([0.1, 0.1, 0.1, 5.0])
R = 0.01 * np.eye(1)

slacks = False
