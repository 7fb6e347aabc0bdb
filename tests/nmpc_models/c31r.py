"""Family member c31r (tests/nmpc_family.py): three states, ONE input, two outputs, two disturbances and one user inequality row of the
OCP that is non-linear in the state and in the input,

    u x1 + 0.2 x0^2 <= 0.70

(a load that the second set point asks to exceed: the OCP rides the row).  Continuous model with a bilinear term, extended Kalman
filter, disturbances inside the model.  The stage state is 3 + 1 row = 4 with a single-column input.  The plant's first state decays
faster than the model's.  Written for this project in the Ex-file surface.
"""
from casadi import *
import numpy as np
import scipy.linalg as scla

Nsim, N, h = 40, 7, 0.5

xp = SX.sym("xp", 3)
x = SX.sym("x", 3)
u = SX.sym("u", 1)
y = SX.sym("y", 2)
d = SX.sym("d", 2)

Mx = 4
ROW_LIMIT = 0.70


def _rhs(s, inflow, decay, extra):
    return vertcat(-decay * s[0] + inflow,
                   s[0] - s[1] - 0.3 * s[1] * s[2],
                   0.5 * s[1] - 0.8 * s[2] + extra)


def User_fxp_Cont(x, t, u, pxp, pxmp):
    return _rhs(x, u[0], 1.1, 0.02)


def User_fyp(x, u, t, pyp, pymp):
    return vertcat(x[1], x[2])


def User_fxm_Cont(x, u, d, t, px):
    return _rhs(x, u[0] + d[0], 1.0, d[1])


def User_fym(x, u, d, t, py):
    return vertcat(x[1], x[2])


def User_g_ineq(x, u, y, d, t, px, py):
    return vertcat(u[0] * x[1] + 0.2 * x[0] * x[0] - ROW_LIMIT)


offree = "nl"

x0_p = np.array([0.60, 0.545, 0.34])
x0_m = np.array([0.60, 0.545, 0.34])
u0 = np.array([0.60])
dhat0 = np.array([0.0, 0.0])

ekf = True
Q_kf = scla.block_diag(1.0e-5 * np.eye(3), 1.0e-2 * np.eye(2))
R_kf = 1.0e-4 * np.eye(2)
P0 = 1.0e-2 * np.eye(5)


def defSP(t):
    ysp = np.array([0.545, 0.0]) if t <= 2.2 else np.array([0.75, 0.0])      # the second output carries no weight
    return [ysp, np.array([0.0]), np.zeros(3)]


umin = np.array([0.0])
umax = np.array([1.0])
xmin = np.array([0.0, 0.0, 0.0])
xmax = np.array([2.0, 2.0, 2.0])

Qss = np.diag([5.0, 0.0])
Rss = np.zeros((1, 1))
Q = np.diag([0.1, 4.0, 0.1])
R = 0.02 * np.eye(1)

slacks = False
