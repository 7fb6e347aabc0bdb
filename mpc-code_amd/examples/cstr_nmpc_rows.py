"""The non-linear CSTR problem (examples/cstr_nmpc.py = the reference's Ex_NMPC.py) with a USER INEQUALITY ROW in the OCP:
``User_g_ineq(x, u, y, d, t, px, py) <= 0`` at every stage of the horizon (reference Control_Calc.py:94-100,132-147; MPC_code.py:306-314):

    u[1] c_A <= 0.87 q_feed    the molar flow of unconverted A leaving the reactor (outlet flow times outlet concentration) is at most 87 %
                               of the A fed (feed concentration 1; q_feed: the estimated feed flow d[1]) - a conversion of at least 13 %

At the initial steady state 12.6 % is converted: the row binds from the first step on, through the feed-flow steps of the scenario.
The stage state is 3 + 1 = 4, so the wave-autonomous kernels take the problem.
"""
import os as _os

exec(open(_os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "cstr_nmpc.py")).read())      # the example's data and functions


def User_g_ineq(x, u, y, d, t, px, py):
    return vertcat(u[1] * x[0] - 0.87 * d[1])
