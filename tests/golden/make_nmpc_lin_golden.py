#!/usr/bin/env python3
"""Generate tests/golden/nmpc_lin_family.npz: the oracle's logs of every case of tests/nmpc_lin_family.py, from oracle/nmpc_oracle.py alone, on the CPU
(about a minute on eight cores).

Per case <c> the file holds <c>_U, _X_HAT, _XS, _US, _Xp, _D_HAT, _STATUS_DYN, _STATUS_SS, _SQP_DYN, _SQP_SS (shaped [steps, instances, dim]), the starts
<c>_x0 / <c>_xm, and <c>_eref: the largest difference (relative to 1 + |value|) between the oracle at its own finite-difference step (1e-6) and at
3e-6 - the reference's own uncertainty.  Further:
    bite_<member>_<switch>   how far the member's rti logs move (same measure) when the feature is switched off (nmpc_lin_family.SWITCHES: Bd = 0, Cd = 0, K halved;
                             Gcov0: G = Bd left out of the covariance update of the EKF only)
    cl21_gain_bite           how far the disturbance estimate of cl21_rti moves within the 12 steps with G out of the covariance: Bd is felt by the gain
    E_ref                    the largest <c>_eref

Asserted here, and again from the file by tests/test_nmpc_lin_host.py: every status word 0 but for the five held instances of cl42_hold (STATUS_DYN 2 at every
step), every switch moves its member by at least 100 x TOL_CAP (the cap of the tests' tolerance), and, per case, the status words of the two
finite-difference steps equal and their SQP iteration counts within 1 of each other at no more than 5 % of the instance-steps.
"""
import os
import sys
import time
from multiprocessing import Pool

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):      # one worker per core: BLAS threads of their own only fight each other (18 s against an hour)
    os.environ.setdefault(_v, "1")

import numpy as np          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for q in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, q)
import nmpc_lin_family as lf          # noqa: E402

TOL_CAP = 2e-7


def _task(a):
    key, member, over, ns, ms, x0, xm, fd, no_g = a
    r = lf.oracle_instance(member, over, ns, ms, x0, xm, fd, no_g)
    return key, {k: v for k, v in r.items() if k in lf.LOGS + lf.ILOGS}


def main():
    t0 = time.time()
    tasks, meta = [], {}
    for name in lf.case_names():
        member, ns, ms, over = lf.case_spec(name)
        p = lf.load_oracle(member, over)
        x0, xm = lf.starts(name, p.x0_p)
        meta[name] = (member, p, x0, xm)
        for b in range(len(x0)):
            for fd in lf.FD_STEPS:
                tasks.append(((name, b, fd), member, over, ns, ms, x0[b], xm[b], fd, False))
    for member, sw in lf.SWITCHES.items():
        name = member + "_rti"
        _, ns, ms, _ = lf.case_spec(name)
        _, _, x0, xm = meta[name]
        for tag, over in sw.items():
            for b in range(lf.BITE_INSTANCES):
                tasks.append((("bite", member, tag, b), member, over, ns, ms, x0[b], xm[b], lf.FD_STEPS[0], tag == "Gcov0"))
    tasks.sort(key=lambda a: -(a[3] * a[4] ** 0.3 * (a[2] or {}).get("N", 10) ** 2))      # the long ones first
    with Pool(int(os.environ.get("FAMILY_JOBS", os.cpu_count() or 2))) as pool:
        res = dict(pool.imap_unordered(_task, tasks, chunksize=1))
    print(f"{len(tasks)} oracle runs in {time.time() - t0:.0f} s", flush=True)

    out, e_ref = {}, 0.0
    for name, (member, p, x0, xm) in meta.items():
        runs = {fd: [res[(name, b, fd)] for b in range(len(x0))] for fd in lf.FD_STEPS}
        g = {k: np.stack([r[k] for r in runs[lf.FD_STEPS[0]]], axis=1) for k in lf.LOGS + lf.ILOGS}
        g2 = {k: np.stack([r[k] for r in runs[lf.FD_STEPS[1]]], axis=1) for k in lf.LOGS + lf.ILOGS}
        for k in lf.ILOGS:
            g[k] = g[k].astype(np.int32)
        out.update({f"{name}_{k}": v for k, v in g.items()})
        out[name + "_x0"], out[name + "_xm"] = x0, xm
        er = max(lf.rel_diff(g2[k], g[k]) for k in lf.LOGS)
        out[name + "_eref"] = np.float64(er); e_ref = max(e_ref, er)
        for k in ("STATUS_DYN", "STATUS_SS"):
            assert np.array_equal(g[k], g2[k]), (name, k)
        assert lf.sqp_counts_within_cap([(g2["SQP_DYN"], g["SQP_DYN"])]), (name, "SQP_DYN of the two finite-difference steps", g["SQP_DYN"].T, g2["SQP_DYN"].T)
        if name == lf.HOLD_CASE:
            held = np.isin(np.arange(lf.B), lf.HELD)
            assert (g["STATUS_DYN"][:, held] == 2).all() and (g["STATUS_DYN"][:, ~held] == 0).all() and (g["STATUS_SS"] == 0).all(), (g["STATUS_DYN"].T, g["STATUS_SS"].T)
        else:
            assert not g["STATUS_DYN"].any() and not g["STATUS_SS"].any(), (name, g["STATUS_DYN"].T, g["STATUS_SS"].T)
        U = g["U"].reshape(-1, p.nu)
        sat = bool((np.abs(U - p.umin) < 1e-7).any() or (np.abs(U - p.umax) < 1e-7).any())
        dsat = bool(p.dmin is not None and ((g["D_HAT"] == p.dmin).any() or (g["D_HAT"] == p.dmax).any()))
        print(f"{name:10s} eref {er:.2e}  sqp iterations up to {int(g['SQP_DYN'].max())}  input bound active: {sat}  estimate saturated: {dsat}", flush=True)
    out["E_ref"] = np.float64(e_ref)

    weak = []
    for member, sw in lf.SWITCHES.items():
        for tag in sw:
            bite = 0.0
            for k in lf.LOGS:
                a = np.stack([res[("bite", member, tag, b)][k] for b in range(lf.BITE_INSTANCES)], axis=1)
                bite = max(bite, lf.rel_diff(a, out[f"{member}_rti_{k}"][:, :lf.BITE_INSTANCES]))
            out[f"bite_{member}_{tag}"] = np.float64(bite)
            print(f"bite {member} {tag}: {bite:.2e}", flush=True)
            weak += [(member, tag, bite)] if bite < 100 * TOL_CAP else []
    a = np.stack([res[("bite", "cl21", "Gcov0", b)]["D_HAT"] for b in range(lf.BITE_INSTANCES)], axis=1)
    out["cl21_gain_bite"] = np.float64(lf.rel_diff(a, out["cl21_rti_D_HAT"][:, :lf.BITE_INSTANCES]))
    print(f"cl21: the estimate without G in the covariance moves by {float(out['cl21_gain_bite']):.2e}")
    weak += [("cl21", "gain", float(out["cl21_gain_bite"]))] if out["cl21_gain_bite"] < 100 * TOL_CAP else []
    assert not weak, weak
    np.savez_compressed(lf.GOLDEN, **out)
    print(f"E_ref {e_ref:.2e}; {os.path.getsize(lf.GOLDEN)} bytes; {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
