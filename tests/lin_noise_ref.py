"""The yardstick of the linear path's white noise (tests/test_lin_noise_host.py, tests/test_lin_noise.py), built from the restatements under
oracle/ as they are: measurement noise v_k is algebraically an addition to pyp_k and state noise w_k an addition to pxp_k, and the restatements
take a schedule - so the noisy loop of instance b is the C restatement's loop of that one instance with the sums as its schedule
(``folded_c_loops``), and the NumPy restatement, whose schedule entries broadcast, takes the sums for all instances at once (``folded_sched``).
The inputs both test files share - problems, start states, draws - and the C loops, computed once per process, live here."""
import functools
import warnings

import numpy as np

B, NSTEPS, SEED = 70, 12, 7          # 70: no multiple of 4 (a last wave of the wave kernel with two of four instances), padded stride 128
EXAMPLES = {"cstr": "cstr_lmpc.py", "wb": "wood_berry_lmpc.py"}


def noise_overrides(p, sigma2=1e-4):
    """R_wn = sigma2 I, G_wn = I, Q_wn = sigma2 I for a loaded problem's dimensions"""
    return {"R_wn": (sigma2 * np.eye(p.ny)).tolist(), "G_wn": np.eye(p.nxp).tolist(), "Q_wn": (sigma2 * np.eye(p.nxp)).tolist()}


def with_noise(pkg, example, sigma2=1e-4, **extra):
    """an example with the three noise matrices as overrides (the loader's warning is the host test's business)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p0 = pkg.load_problem(pkg.example_path(example), overrides=extra or None)
        return pkg.load_problem(pkg.example_path(example), overrides={**extra, **noise_overrides(p0, sigma2)})


@functools.lru_cache(maxsize=None)
def problem(which):
    import mpc_code_amd
    return with_noise(mpc_code_amd, EXAMPLES[which])


def start_states(which, nb=B):
    """x0 of test_gpu_parity.test_plant_and_model_starting_apart (default_rng(3)); the model starts where the plant does"""
    rng = np.random.default_rng(3)
    p = problem(which)
    return rng.uniform([-0.5, -8.0, -5.0], [0.5, 8.0, 5.0], size=(nb, 3)) if which == "cstr" else 0.05 * rng.standard_normal((nb, p.nx))


def draws(which, mode="vw", nb=B, n=NSTEPS):
    """(v, w) of noise_seed = 7; mode "v" / "w": one of them alone (the same numbers), "none": neither"""
    from mpc_code_amd.noise import loop_noise
    v, w = loop_noise(problem(which), n, nb, SEED)
    return (v if "v" in mode else None), (w if "w" in mode else None)


def folded_sched(p, n, v, w):
    """the schedule with the noise folded in: pyp [n, B, ny] and pxp [n, B, nxp] where there is noise (entries broadcast over the batch otherwise)"""
    s = {k: np.array(a[:n]) for k, a in p.schedules(n).items()}
    if v is not None:
        s["pyp"] = s["pyp"][:, None, :] + v[:n]
    if w is not None:
        s["pxp"] = s["pxp"][:, None, :] + w[:n]
    return s


def folded_c_loops(oc, p, n, x0, xm, v, w):
    """the C restatement instance by instance, each with its own folded schedule; logs stacked to [n, B, dim] / [n, B]"""
    s0 = {k: np.array(a[:n]) for k, a in p.schedules(n).items()}
    o = oc.OracleC(p)
    runs = []
    for b in range(len(x0)):
        s = dict(s0)
        if v is not None:
            s["pyp"] = s0["pyp"] + v[:n, b]
        if w is not None:
            s["pxp"] = s0["pxp"] + w[:n, b]
        r = o.closed_loop(n, x0[b:b + 1], xm[b:b + 1], sched=s, nthreads=1)
        runs.append({k: a for k, a in r.items() if k != "final"})
    return {k: np.concatenate([r[k] for r in runs], axis=1) for k in runs[0]}


_c_loops = {}


def c_reference(oc, which, mode="vw"):
    """the folded C loops of the shared inputs, computed once per process and handed out read-only"""
    if (which, mode) not in _c_loops:
        p, x0 = problem(which), start_states(which)
        r = folded_c_loops(oc, p, NSTEPS, x0, x0, *draws(which, mode))
        for a in r.values():
            a.setflags(write=False)
        _c_loops[which, mode] = r
    return _c_loops[which, mode]
