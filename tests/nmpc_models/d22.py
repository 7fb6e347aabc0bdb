"""Family member d22 (tests/nmpc_family.py): two states, two inputs, two outputs, two disturbances - two coupled vessels given as a
SAMPLED map (User_fxm_Dis) with a quadratic and a bilinear term.  Fixed-gain observer (lue, K), linear disturbance model
(offree = "lin") with non-zero Bd AND Cd, both outputs boxed (their rows carry Cd d), a non-diagonal terminal weight (User_vfin) and a
target that weighs the move of the input target (Sss).  The plant's coefficients are not the model's.  Written for this project in
the Ex-file surface.
"""
from casadi import *
import numpy as np

Nsim, N, h = 40, 6, 1.0

xp = SX.sym("xp", 2)
x = SX.sym("x", 2)
u = SX.sym("u", 2)
y = SX.sym("y", 2)
d = SX.sym("d", 2)


def _map(s, v, a00, a11, q):
    nxt = SX(2, 1)
    nxt[0] = a00 * s[0] + 0.10 * s[1] - q * s[0] * s[0] + 0.20 * v[0] + 0.02 * v[1]
    nxt[1] = 0.08 * s[0] + a11 * s[1] - 0.03 * s[0] * s[1] + 0.05 * v[0] + 0.25 * v[1]
    return nxt


def User_fxp_Dis(x, t, u, pxp, pxmp):
    return _map(x, u, 0.82, 0.78, 0.05)


def User_fxm_Dis(x, u, d, t, px):
    return _map(x, u, 0.85, 0.80, 0.04)


def User_fyp(x, u, t, pyp, pymp):
    return vertcat(x[0], x[1])


def User_fym(x, u, d, t, py):
    return vertcat(x[0], x[1])


offree = "lin"
Bd = np.array([[0.10, 0.00], [0.02, 0.08]])
Cd = np.array([[0.60, 0.10], [0.00, 0.70]])

x0_p = np.array([0.50, 0.45])
x0_m = np.array([0.50, 0.45])
u0 = np.array([0.30, 0.25])

lue = True
K = np.array([[0.35, 0.00], [0.00, 0.35], [0.30, -0.05], [0.00, 0.30]])


def defSP(t):
    ysp = np.array([0.50, 0.45]) if t <= 4.5 else np.array([0.80, 0.55])      # (targets of both inputs inside their bounds: a target ON a bound leaves the OCP's bound weakly active)
    return [ysp, np.array([0.0, 0.0]), np.array([0.0, 0.0])]


umin = np.array([0.0, 0.0])
umax = np.array([0.6, 0.9])
xmin = np.array([-1.0, -1.0])
xmax = np.array([2.0, 2.0])
ymin = np.array([0.0, 0.0])
ymax = np.array([1.6, 1.6])

Qss = np.diag([1.0, 2.0])
Sss = 0.5 * np.eye(2)
Q = np.diag([1.0, 2.0])
R = np.diag([0.1, 0.2])


def User_vfin(x, xs):
    return 20.0 * x[0] * x[0] + 10.0 * x[0] * x[1] + 15.0 * x[1] * x[1]      # 1/2 dx' [[40, 10], [10, 30]] dx
