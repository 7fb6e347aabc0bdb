"""Family member cl42 (tests/nmpc_lin_family.py): four states, two inputs, two outputs, two disturbances - two pairs of vessels as a
CONTINUOUS model with quadratic and bilinear terms and the LINEAR disturbance model (offree = "lin": RK4 of the right-hand side, then
+ Bd d; Cd on the output rows).  Fixed-gain observer (lue, K), saturation of the estimate (dmin / dmax), every bound finite: a full tile
with two input columns on the unmasked tables.  The plant's coefficients are not the model's.  Written for this project in the Ex-file
surface.
"""
from casadi import *
import numpy as np

Nsim, N, h = 40, 9, 0.5

xp = SX.sym("xp", 4)
x = SX.sym("x", 4)
u = SX.sym("u", 2)
y = SX.sym("y", 2)
d = SX.sym("d", 2)

Mx = 3


def _rhs(s, v, a0, a2):
    return vertcat(-a0 * s[0] + 0.3 * s[2] - 0.2 * s[0] * s[0] + v[0],
                   0.4 * s[0] - 0.8 * s[1] + 0.1 * s[0] * s[1],
                   -a2 * s[2] + 0.2 * s[3] - 0.1 * s[2] * s[2] + 0.8 * v[1],
                   0.3 * s[1] + 0.3 * s[2] - 0.9 * s[3])


def User_fxp_Cont(x, t, u, pxp, pxmp):
    return _rhs(x, u, 0.96, 0.74)


def User_fyp(x, u, t, pyp, pymp):
    return vertcat(x[1], x[3])


def User_fxm_Cont(x, u, d, t, px):
    return _rhs(x, u, 0.90, 0.70)


def User_fym(x, u, d, t, py):
    return vertcat(x[1], x[3])


offree = "lin"
Bd = np.array([[0.10, 0.00], [0.00, 0.05], [0.00, 0.10], [0.02, 0.00]])
Cd = np.array([[0.30, 0.00], [0.10, 0.40]])

x0_p = np.array([0.52, 0.28, 0.50, 0.26])
x0_m = np.array([0.52, 0.28, 0.50, 0.26])
u0 = np.array([0.40, 0.40])
dhat0 = np.array([0.0, 0.0])

lue = True
K = np.array([[0.10, 0.00], [0.30, 0.00], [0.00, 0.10], [0.00, 0.30], [0.30, -0.05], [0.00, 0.30]])

dmin = np.array([-0.08, -0.08])
dmax = np.array([0.08, 0.08])


def defSP(t):
    ysp = np.array([0.28, 0.26]) if t <= 2.2 else np.array([0.40, 0.33])
    return [ysp, np.array([0.0, 0.0]), np.zeros(4)]


umin = np.array([0.0, 0.0])
umax = np.array([0.75, 0.9])
xmin = np.array([-0.2, -0.2, -0.2, -0.2])
xmax = np.array([1.5, 1.5, 1.5, 1.5])
ymin = np.array([-0.5, -0.5])
ymax = np.array([1.2, 1.2])

Qss = np.diag([2.0, 1.0])
Rss = 1.0e-3 * np.eye(2)
Q = np.diag([0.1, 2.0, 0.1, 1.0])
R = np.diag([0.05, 0.05])
