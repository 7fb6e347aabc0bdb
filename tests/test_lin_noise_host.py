"""White noise on the linear path, the parts that need no GPU: the loader, the draws, the yardstick the GPU tests compare with (the C restatement with
the noise folded into its schedule, tests/lin_noise_ref.py, against two independent witnesses) and the host staging of the noise arrays."""
import os
import subprocess
import warnings

import numpy as np
import pytest

import lin_noise_ref as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "mpc-code_amd", "csrc")
TOL = 1e-7      # the tolerance of the GPU test against this reference (tests/test_lin_noise.py)


def test_loader_keeps_the_noise_matrices_and_says_that_loops_run_noise_free(pkg, cstr):
    over = ref.noise_overrides(cstr)
    with pytest.warns(UserWarning, match="noise_seed"):
        p = pkg.load_problem(pkg.example_path("cstr_lmpc.py"), overrides=over)
    assert isinstance(p, pkg.LinearMPCProblem)
    assert np.array_equal(p.R_wn, 1e-4 * np.eye(3)) and np.array_equal(p.G_wn, np.eye(3)) and np.array_equal(p.Q_wn, 1e-4 * np.eye(3))
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # an example without noise loads silently and carries none
        q = pkg.load_problem(pkg.example_path("cstr_lmpc.py"))
    assert q.R_wn is None and q.G_wn is None and q.Q_wn is None
    for half in ("G_wn", "Q_wn"):
        with pytest.raises(pkg.UnsupportedProblem, match="G_wn and Q_wn"):
            pkg.load_problem(pkg.example_path("cstr_lmpc.py"), overrides={half: over[half]})
    with pytest.raises(ValueError, match="R_wn"):
        pkg.load_problem(pkg.example_path("cstr_lmpc.py"), overrides={"R_wn": np.eye(2).tolist()})
    with pytest.raises(pkg.UnsupportedProblem, match="def_pxmp"):
        pkg.load_problem(pkg.example_path("cstr_lmpc.py"), overrides={"def_pxmp": lambda t: [np.zeros(3)]})


def test_draws_are_the_economic_paths_and_do_not_depend_on_the_number_of_ranks(pkg):
    from mpc_code_amd import driver, enmpc, noise
    p = ref.with_noise(pkg, "cstr_xp_nlplant_lmpc.py")      # ny = 2, nxp = 3: the two arrays differ in shape
    n, B = 5, 70
    v, w = driver.shard_noise(p, n, B, 7)
    assert v.shape == (n, B, p.ny) and w.shape == (n, B, p.nxp) and p.ny != p.nxp
    assert enmpc.loop_noise is noise.loop_noise      # one function, under the name it had
    # its order, restated: per step first the measurement's draws, then the state's, from one generator; symmetric square roots (diagonal here)
    rng = np.random.default_rng(7)
    for k in range(n):
        assert np.array_equal(v[k], rng.standard_normal((B, p.ny)) @ (1e-2 * np.eye(p.ny)))
        assert np.array_equal(w[k], rng.standard_normal((B, p.nxp)) @ (1e-2 * np.eye(p.nxp)))
    ve, we = enmpc.loop_noise(p, n, B, 7)
    assert np.array_equal(v, ve) and np.array_equal(w, we)
    v1, w1 = driver.shard_noise(p, n, 35, 7, total=70, rank=1, world=2)
    assert np.array_equal(v1, v[:, 35:70]) and np.array_equal(w1, w[:, 35:70])
    v0, _ = driver.shard_noise(p, n, 24, 7, total=70, rank=0, world=3)      # 70 = 24 + 23 + 23
    assert np.array_equal(v0, v[:, :24])
    with pytest.raises(ValueError, match="owns"):
        driver.shard_noise(p, n, 35, 7, total=70, rank=0, world=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        only_v = pkg.load_problem(pkg.example_path("cstr_lmpc.py"), overrides={"R_wn": (1e-4 * np.eye(3)).tolist()})
    vv, ww = driver.shard_noise(only_v, n, B, 7)
    assert vv.shape == (n, B, 3) and ww is None
    with pytest.raises(ValueError, match="neither"):
        driver.shard_noise(pkg.load_problem(pkg.example_path("cstr_lmpc.py")), n, B, 7)


@pytest.mark.parametrize("which", ["cstr", "wb"])
def test_folded_c_loops_against_the_numpy_restatement(which, oracle_c):
    """The reference of the GPU test - the C restatement instance by instance with v in pyp and w in pxp - against the NumPy restatement, which takes the sums
    for all instances at once: equal status words, every log within the GPU test's tolerance (measured: 1.3e-9 on CSTR, 3e-15 on Wood-Berry).  And the noise is
    felt: v alone and w alone each move every instance's U by at least 100 tolerances from the noise-free loop; w cannot act at step 0, v does."""
    import riccati_np as rn
    p, x0 = ref.problem(which), ref.start_states(which)
    v, w = ref.draws(which)
    c = ref.c_reference(oracle_c, which)
    r = rn.closed_loop_batch(p, ref.NSTEPS, x0, x0, sched=ref.folded_sched(p, ref.NSTEPS, v, w))
    assert np.array_equal(c["STATUS_DYN"], r["STATUS_DYN"]) and np.array_equal(c["STATUS_SS"], r["STATUS_SS"])
    for k in ("U", "XS", "US", "YS", "X_HAT", "Xp", "D_HAT"):
        d = np.abs(c[k] - r[k]).max()
        print(which, k, d)
        assert d < TOL, (k, d)
    free = ref.c_reference(oracle_c, which, "none")
    plain = oracle_c.OracleC(p).closed_loop(ref.NSTEPS, x0, x0)      # ... and folding nothing is the batch loop, to the bit
    assert all(np.array_equal(free[k], plain[k]) for k in free)
    for mode in ("v", "w"):
        one = ref.c_reference(oracle_c, which, mode)
        moved = np.abs(one["U"] - free["U"]).max(axis=(0, 2))
        print(which, mode, "alone moves U by at least", moved.min())
        assert moved.min() >= 100 * TOL, (mode, moved.min())
    assert np.abs(ref.c_reference(oracle_c, which, "w")["U"][0] - free["U"][0]).max() == 0.0
    assert np.abs(ref.c_reference(oracle_c, which, "v")["U"][0] - free["U"][0]).max() > 100 * TOL
    if which == "cstr":      # the hold branch is part of the comparison
        assert (c["STATUS_DYN"] == 2).any()


def test_folded_c_loops_against_the_dense_oracle(oracle_c):
    """Two CSTR instances over six steps against the dense statement of the loop with the same folded schedule, at the bound
    test_gpu_parity.test_plant_and_model_starting_apart uses for this pair."""
    import mpc_oracle as mo
    p, x0 = ref.problem("cstr"), ref.start_states("cstr")
    v, w = ref.draws("cstr")
    c = ref.c_reference(oracle_c, "cstr")
    s0 = p.schedules(6)
    for b in (0, 1):
        s = dict(s0, pyp=s0["pyp"] + v[:6, b], pxp=s0["pxp"] + w[:6, b])
        o = mo.closed_loop(p, 6, x0_p=x0[b], x0_m=x0[b], sched=s)
        assert np.array_equal(np.asarray(o["STATUS_DYN"]).ravel(), c["STATUS_DYN"][:6, b])
        for k in ("U", "XS", "X_HAT", "D_HAT"):
            d = np.max(np.abs(np.asarray(o[k]).reshape(6, -1) - c[k][:6, b]))
            print(b, k, d)
            assert d < 2e-6, (b, k, d)


def test_noise_staging_under_sanitizers(tmp_path):
    """tests/noise_staging_check.cpp - a program of its own that includes mpc_host.hpp and makes no HIP call - with its host side under ASan and UBSan, run
    as a child process: [nsteps][B][d] -> [step][d][Bs] and back for B in {1, 63, 64, 65, 130}, d in {0, 2, 3}, 1 and 3 steps, the padding lanes zero."""
    exe = str(tmp_path / "noise_staging_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "noise_staging_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "noise staging ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
