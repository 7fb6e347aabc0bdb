"""Family member c11 (tests/nmpc_family.py): one state, one input, one output, one disturbance - a stirred vessel whose temperature
rise x is driven by a heater u and lost to the surroundings by a linear and a cubic term.  Continuous model, extended Kalman filter,
the disturbance (an unknown heat flow) inside the model.  Stage state 1: a one-element tile of the wave-style kernels.  The plant
loses more heat than the model believes.  Written for this project in the Ex-file surface.
"""
from casadi import *
import numpy as np
import scipy.linalg as scla

Nsim, N, h = 40, 8, 0.5

xp = SX.sym("xp", 1)
x = SX.sym("x", 1)
u = SX.sym("u", 1)
y = SX.sym("y", 1)
d = SX.sym("d", 1)

LOSS, LOSS_PLANT, CUBIC = 0.8, 0.95, 0.3
Mx = 4


def User_fxp_Cont(x, t, u, pxp, pxmp):
    return vertcat(-LOSS_PLANT * x[0] - CUBIC * x[0] * x[0] * x[0] + u[0])


def User_fyp(x, u, t, pyp, pymp):
    return vertcat(x[0])


def User_fxm_Cont(x, u, d, t, px):
    return vertcat(-LOSS * x[0] - CUBIC * x[0] * x[0] * x[0] + u[0] + d[0])


def User_fym(x, u, d, t, py):
    return vertcat(x[0])


offree = "nl"

x0_p = np.array([0.60])
x0_m = np.array([0.60])
u0 = np.array([0.55])
dhat0 = np.array([0.0])

ekf = True
Q_kf = scla.block_diag(1.0e-4 * np.eye(1), 1.0e-2 * np.eye(1))
R_kf = 1.0e-3 * np.eye(1)
P0 = 1.0e-2 * np.eye(2)


def defSP(t):
    ysp = np.array([0.6]) if t <= 2.2 else np.array([1.1])
    return [ysp, np.array([0.0]), np.array([0.0])]


umin = np.array([0.0])
umax = np.array([1.6])
xmin = np.array([0.0])
xmax = np.array([2.0])

Qss = np.eye(1)
Rss = np.zeros((1, 1))
Q = np.eye(1)
R = 0.02 * np.eye(1)

slacks = False
