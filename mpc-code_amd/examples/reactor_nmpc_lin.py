"""Non-linear offset-free tracking MPC of the isothermal reactor A -> B -> C with the LINEAR disturbance model and full state feedback.

Written for this project in the Ex-file surface of CPCLAB-UNIPI/MPC-code (names documented in its User_Guide.pdf ch. 3).  The reactor is
the one of ``examples/reactor_nmpc.py`` (balances and parameters of the reference's ``Ex_ENMPC.py:42-49, 64-65``), stated the way that
file states its model: a continuous-time model that does not see the disturbance (``User_fxm_Cont`` without ``d``), ``offree = "lin"`` with
an output disturbance (``Bd = 0``, ``Cd = I``, ``Ex_ENMPC.py:98-100``), ``StateFeedback = True`` (``:33``: both concentrations are measured, so
the output maps are the loader's and ``User_fym / User_fyp`` are left out), extended Kalman filter, white noise on the measurement
(``R_wn``) and on the plant state (``G_wn / Q_wn``, which ``Ex_ENMPC.py:68-69`` carries commented out).  The reference optimises an economic
cost there; this file tracks a set point of the product concentration: the combination the non-linear tracking path refused before
(``reactor_nmpc.py`` had to put its disturbances inside the model, ``offree = "nl"``, to get onto it).
"""
from casadi import *
import numpy as np
import scipy.linalg as scla

Nsim, N, h = 60, 25, 2.0

xp = SX.sym("xp", 2)     # plant state: concentrations of A and B [kmol/m^3]
x = SX.sym("x", 2)
u = SX.sym("u", 1)       # dilution rate F / V [1/min]
y = SX.sym("y", 2)
d = SX.sym("d", 2)

StateFeedback = True     # y = x (+ Cd d on the model's side)

FEED_CONC = 1.0
K1, K2 = 1.0, 0.05
K1_PLANT = 1.1           # the plant's first reaction is 10 % faster than the model believes
Mx = 10


def _balances(c_a, c_b, dilution, k1):
    return vertcat(dilution * (FEED_CONC - c_a) - k1 * c_a, -dilution * c_b + k1 * c_a - K2 * c_b)


def User_fxp_Cont(x, t, u, pxp, pxmp):
    return _balances(x[0], x[1], u[0], K1_PLANT)


def User_fxm_Cont(x, u, d, t, px):
    return _balances(x[0], x[1], u[0], K1)


offree = "lin"           # x+ = RK4(model)(x, u) + Bd d, y = x + Cd d
Bd = np.zeros((2, 2))
Cd = np.eye(2)

# white noise of the simulation (unseeded in the reference: simulated here only with noise_seed=...)
R_wn = 1.0e-7 * np.eye(2)      # measurement: sqrtm(R_wn) N(0, I)
G_wn = 1.0e-2 * np.eye(2)      # plant state after its step: G_wn sqrtm(Q_wn) N(0, I)
Q_wn = 1.0e-3 * np.eye(2)

x0_p = np.array([0.45, 0.50])
x0_m = np.array([0.45, 0.50])
u0 = np.array([0.8])
dhat0 = np.array([0.0, 0.0])

ekf = True
Q_kf = scla.block_diag(1.0e-6 * np.eye(2), 1.0e-2 * np.eye(2))
R_kf = 1.0e-4 * np.eye(2)
P0 = 1.0e-2 * np.eye(4)


def defSP(t):
    xsp = np.array([0.0, 0.0])
    ysp = np.array([0.0, 0.56]) if t <= 40 else np.array([0.0, 0.48])     # product concentration; the first output carries no weight
    usp = np.array([0.0])
    return [ysp, usp, xsp]


umin = np.array([0.05])
umax = np.array([2.0])
xmin = np.array([0.0, 0.0])
xmax = np.array([1.0, 1.0])

dmin = -0.5 * np.ones((2, 1))
dmax = 0.5 * np.ones((2, 1))

Qss = np.diag([0.0, 10.0])
Rss = np.zeros((1, 1))
Q = np.diag([0.1, 1.0])
R = 0.05 * np.eye(1)

slacks = False
