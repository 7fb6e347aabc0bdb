"""Family member c22 (tests/nmpc_family.py): two states, two inputs, ONE output (the second state), one disturbance - continuous model
with a bilinear term, FIXED-GAIN observer (lue, K) on a continuous model, the disturbance inside the model and saturated by
dmin / dmax (the plant's mismatch asks for more than dmax), plant and measurement disturbance schedules (def_pxp, def_pyp).
Written for this project in the Ex-file surface.
"""
from casadi import *
import numpy as np

Nsim, N, h = 40, 6, 0.5

xp = SX.sym("xp", 2)
x = SX.sym("x", 2)
u = SX.sym("u", 2)
y = SX.sym("y", 1)
d = SX.sym("d", 1)

Mx = 4


def _rhs(s, v, leak, extra):
    return vertcat(-s[0] + v[0] - 0.2 * s[0] * s[1],
                   s[0] - leak * s[1] + 0.5 * v[1] + extra)


def User_fxp_Cont(x, t, u, pxp, pxmp):
    return _rhs(x, u, 0.6, 0.0)


def User_fyp(x, u, t, pyp, pymp):
    return vertcat(x[1])


def User_fxm_Cont(x, u, d, t, px):
    return _rhs(x, u, 0.7, d[0])


def User_fym(x, u, d, t, py):
    return vertcat(x[1])


def def_pxp(t):
    return [np.array([0.0, 0.01])] if 1.2 <= t <= 3.2 else [np.zeros(2)]


def def_pyp(t):
    return [np.array([0.005])] if t >= 1.8 else [np.zeros(1)]


offree = "nl"

x0_p = np.array([0.45, 0.80])
x0_m = np.array([0.45, 0.80])
u0 = np.array([0.50, 0.20])
dhat0 = np.array([0.0])

lue = True
K = np.array([[0.10], [0.45], [0.30]])

dmin = np.array([-0.03])
dmax = np.array([0.03])


def defSP(t):
    ysp = np.array([0.80]) if t <= 2.2 else np.array([1.20])
    return [ysp, np.array([0.50, 0.20]), np.zeros(2)]


umin = np.array([0.0, 0.0])
umax = np.array([1.0, 0.6])
xmin = np.array([0.0, 0.0])
xmax = np.array([2.0, 2.0])

Qss = 10.0 * np.eye(1)
Rss = np.diag([0.1, 0.1])
Q = np.diag([0.1, 3.0])
R = np.diag([0.02, 0.05])

slacks = False
