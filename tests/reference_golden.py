"""The reference's side of the tests that hold the shipped examples against the reference's own Ex-files: what
tests/golden/make_reference_golden.py read of the unmodified reference files, stored in tests/golden/reference_examples.npz."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_examples.npz")

# the reference's Ex-files and their counterparts under mpc-code_amd/examples/
EX_FILES = {"Ex_LMPC_CSTR.py": "cstr_lmpc.py", "Ex_LMPC_WB.py": "wood_berry_lmpc.py", "Ex_LMPC_nlplant.py": "cstr_nlplant_lmpc.py",
            "Ex_LMPCxp_nlplant.py": "cstr_xp_nlplant_lmpc.py", "Ex_NMPC.py": "cstr_nmpc.py", "Ex_NMPC_dis.py": "quadtank_nmpc_dis.py",
            "Ex_ENMPC.py": "reactor_enmpc.py"}
LMPC_EX = ("Ex_LMPC_CSTR.py", "Ex_LMPC_WB.py", "Ex_LMPC_nlplant.py", "Ex_LMPCxp_nlplant.py")
EX_FIELDS = ["A", "B", "C", "Bd", "Cd", "Ap", "Bp", "Cp", "Q", "R", "P", "Qss", "Rss", "umin", "umax", "xmin", "xmax",
             "ymin", "ymax", "x0_p", "x0_m", "u0", "fx_const", "fy_const", "Q_kf", "R_kf", "P0"]
EX_SP_TIMES = (0, 10, 11, 15, 16, 20, 21, 99)
KIND_REFUSALS = ({"slacks": True}, {"Collocation": True}, {"mhe_up": "other"})
NMPC_FIELDS = ("Q", "R", "Qss", "Rss", "umin", "umax", "xmin", "xmax", "ymin", "ymax", "dmin", "dmax", "Q_kf", "R_kf", "P0", "x0_p", "x0_m",
               "u0", "dhat0", "umin_ss", "umax_ss", "xmin_ss", "xmax_ss", "ymin_ss", "ymax_ss")
DIS_FIELDS = ("Q", "R", "Qss", "Rss", "umin", "umax", "xmin", "xmax", "ymin", "ymax", "Dumin", "Dumax", "K", "Pf", "Bd", "Cd", "x0_p", "x0_m", "u0", "dhat0")
DIS_TIMES = (10, 60, 1500, 2500, 3500, 4500, 6000)
RX_POINT = {"x[0]": 0.4, "x[1]": 0.55, "u[0]": 0.7, "d[0]": 0.0, "d[1]": 0.0, "t": 0.0}
# fields the loader computes by a numerical solve or a matrix product from the file's data (Riccati equations, the affine terms of a
# linearisation): stored on one host, compared to rounding on another; every other field is the file's data and compared bit for bit
SOLVED = ("P", "K", "Pf", "fx_const", "fy_const")


def load():
    return np.load(GOLD)


def assert_fields(obj, g, pre, names):
    """Every named attribute of obj is the reference's: None where it was None, else the same array."""
    none = set(g[pre + "none"].tolist())
    for f in names:
        v = getattr(obj, f)
        if f in none:
            assert v is None, f
        elif f in SOLVED:
            np.testing.assert_allclose(np.asarray(v, dtype=float), g[pre + f], rtol=1e-12, atol=1e-15, err_msg=f)
        else:
            assert np.array_equal(np.asarray(v), g[pre + f]), f
