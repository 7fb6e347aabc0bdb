import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def gpu_available():
    try:
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        return hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        return False


@pytest.fixture(scope="session")
def pkg():
    import mpc_code_amd
    return mpc_code_amd


@pytest.fixture(scope="session")
def ref_gold():
    """The reference's Ex-files as the loaders read them (tests/golden/reference_examples.npz, tests/reference_golden.py)."""
    import reference_golden
    return reference_golden.load()


@pytest.fixture(scope="session")
def cstr(pkg):
    return pkg.load_problem(pkg.example_path("cstr_lmpc.py"))


@pytest.fixture(scope="session")
def wb(pkg):
    return pkg.load_problem(pkg.example_path("wood_berry_lmpc.py"))


@pytest.fixture(scope="session")
def nlplant(pkg):
    return pkg.load_problem(pkg.example_path("cstr_nlplant_lmpc.py"))


@pytest.fixture(scope="session")
def xp_nlplant(pkg):
    return pkg.load_problem(pkg.example_path("cstr_xp_nlplant_lmpc.py"))


def double_integrator_with_output_row(N=20, du=False):
    """nx=2, nu=1 with the bounded output y = x0 + x1: a general row of C (no single state carries it)."""
    import scipy.linalg as scla
    from mpc_code_amd.problem import LinearMPCProblem
    A = np.array([[1.0, 0.1], [0.0, 1.0]]); Bm = np.array([[0.005], [0.1]]); C = np.array([[1.0, 1.0]])
    Q = np.diag([1.0, 0.1]); R = np.array([[0.01]])
    P = scla.solve_discrete_are(A, Bm, Q, R)
    inf = np.inf
    return LinearMPCProblem(nx=2, nu=1, ny=1, nd=1, nxp=2, N=N, h=0.1, Nsim=10, A=A, B=Bm, C=C, Bd=np.array([[0.0], [0.1]]), Cd=np.array([[0.3]]),
                            fx_const=np.zeros(2), fy_const=np.array([0.05]), Ap=A, Bp=Bm, Cp=C, Q=Q, R=R, DUForm=du, P=P,
                            Qss=np.eye(1), Rss=np.zeros((1, 1)), DUssForm=False, umin=np.array([-1.0]), umax=np.array([1.0]),
                            xmin=np.array([-inf, -0.8]), xmax=np.array([2.0, inf]), ymin=np.array([-0.4]), ymax=np.array([0.7]), y_bounded=True,
                            umin_ss=np.array([-1.0]), umax_ss=np.array([1.0]), xmin_ss=np.array([-inf, -0.8]), xmax_ss=np.array([2.0, inf]),
                            ymin_ss=np.array([-inf]), ymax_ss=np.array([inf]), estimator="kalss", K=np.array([[0.5], [0.1], [0.2]]),
                            x0_p=np.zeros(2), x0_m=np.zeros(2), u0=np.zeros(1), dhat0=np.zeros(1))


def five_state_problem(N=30):
    """nx = 5, nu = 2, ny = 2, nd = 2: a stable random plant with bounded inputs and two bounded states - a dimension set outside the
    default library (capi builds it on demand), stage blocks of 2 x 2 tiles in the wave-autonomous kernel."""
    import scipy.linalg as scla
    from mpc_code_amd.problem import LinearMPCProblem
    rng = np.random.default_rng(2025)
    A = rng.standard_normal((5, 5)); A *= 0.92 / np.abs(np.linalg.eigvals(A)).max()
    Bm = rng.standard_normal((5, 2)) * 0.5
    C = np.zeros((2, 5)); C[0, 0] = 1.0; C[1, 3] = 1.0
    Bd = Bm.copy(); Cd = np.zeros((2, 2))
    Q = np.diag([1.0, 0.1, 0.1, 1.0, 0.1]); R = np.diag([0.1, 0.2])
    P = scla.solve_discrete_are(A, Bm, Q, R)
    inf = np.inf
    xmin = np.array([-2.0, -inf, -inf, -1.5, -inf]); xmax = np.array([2.0, inf, inf, 1.5, inf])
    K = np.vstack([0.3 * np.linalg.pinv(C), 0.1 * np.eye(2)])
    return LinearMPCProblem(nx=5, nu=2, ny=2, nd=2, nxp=5, N=N, h=1.0, Nsim=20, A=A, B=Bm, C=C, Bd=Bd, Cd=Cd,
                            fx_const=np.zeros(5), fy_const=np.zeros(2), Ap=A, Bp=Bm, Cp=C, Q=Q, R=R, DUForm=False, P=P,
                            Qss=np.eye(2), Rss=np.zeros((2, 2)), DUssForm=False, umin=np.array([-1.0, -1.0]), umax=np.array([1.0, 1.0]),
                            xmin=xmin, xmax=xmax, ymin=np.full(2, -inf), ymax=np.full(2, inf), y_bounded=False,
                            umin_ss=np.array([-1.0, -1.0]), umax_ss=np.array([1.0, 1.0]), xmin_ss=xmin, xmax_ss=xmax,
                            ymin_ss=np.full(2, -inf), ymax_ss=np.full(2, inf), estimator="kalss", K=K,
                            x0_p=np.zeros(5), x0_m=np.zeros(5), u0=np.zeros(2), dhat0=np.zeros(2))


@pytest.fixture(scope="session")
def five_state(pkg):
    return five_state_problem()


@pytest.fixture(scope="session")
def dint_yrow(pkg):
    return double_integrator_with_output_row()


@pytest.fixture(scope="session")
def oracle_c():
    import oracle_c as oc
    oc.build()
    return oc


@pytest.fixture(scope="session")
def solver_factory(pkg):
    """Solver on cuda:0 - the HIP path, loudly required for -m gpu tests."""
    from mpc_code_amd import capi
    made = []

    def make(problem, loop_kernel=0):
        s = capi.Solver(problem, device=0)
        made.append(s)
        try:
            s.set_option("loop_kernel", loop_kernel)      # 0 auto, 1 instance per lane, 2 horizon-parallel, 3 wave-autonomous
        except capi.MpcAmdError:
            if loop_kernel == 3:      # stage does not fit a 4x4 tile (Wood-Berry) or N > 64
                pytest.skip("the wave-autonomous kernel does not take this problem")
            raise
        return s

    yield make
    for s in made:
        s.close()


def bench_x0(B, seed=20250614):
    """Initial states of BASELINE.md section 3: x0 ~ U([-0.5,0.5] x [-8,8] x [-5,5])."""
    rng = np.random.default_rng(seed)
    return rng.uniform([-0.5, -8.0, -5.0], [0.5, 8.0, 5.0], size=(B, 3))
