"""The shipped CSTR scenario (cstr_lmpc.py) with affine user rows in the TARGET problem (the reference's ``User_g_ineq_SS`` / ``User_h_eq_SS``,
Target_Calc.py:87-110,139-155; MPC_code.py:295-300), on the target's own variables (Xs, Us, Ys):
the third output follows the first input, ``y_2 - 0.02 u_0 + 0.01 d_0 = 0``, and the first output is capped together with the first input,
``y_0 + 0.02 u_0 - 0.2 <= 0``.  Along the scenario the equality binds at every step; the inequality binds from the fourth step on, before and after
the set-point change at t = 15 (until the plant disturbance changes at t = 20); at the third step the rows leave no feasible target, and the previous
one is kept."""
import os
import runpy

globals().update({k: v for k, v in runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "cstr_lmpc.py")).items() if not k.startswith("__")})


def User_h_eq_SS(x, u, y, d, t, px, py):
    return y[2] - 0.02 * u[0] + 0.01 * d[0]


def User_g_ineq_SS(x, u, y, d, t, px, py):
    return y[0] + 0.02 * u[0] - 0.2
