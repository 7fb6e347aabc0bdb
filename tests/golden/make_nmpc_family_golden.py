#!/usr/bin/env python3
"""Generate tests/golden/nmpc_family.npz: the oracle's logs of every case of tests/nmpc_family.py (about two minutes on eight cores).

Per case <c> the file holds <c>_U, _X_HAT, _XS, _US, _Xp, _D_HAT, _STATUS_DYN, _STATUS_SS, _SQP_DYN, _SQP_SS (shaped [steps, 9, dim]), the starts
<c>_x0 / <c>_xm, and <c>_eref: the largest difference (relative to 1 + |value|) between the oracle at its own finite-difference step (1e-6) and at
3e-6 - the reference's own uncertainty.  The trajectories W are not stored; what the tests need of them is:
    <member>_xgap      c41, d42: the smallest distance of a predicted state to a finite state bound over every W of the member's cases
    c31r_<mode>_ROW0   the row's value at stage 0 of every step
    bite_<member>_<switch>   how far the member's rti logs move (same measure) when the feature is switched off (nmpc_family.SWITCHES)
    E_ref              the largest <c>_eref

Asserted here, and again from the file by tests/test_nmpc_family.py: every status word 0 (the held instances of d22_hold: 2 at every step), an input bound
active in every member, a state bound active in c41 and d42, the row active in c31r, the estimate on dmax in c22, every switch moves its member by at least
100 x 2e-7 (the cap of the tests' tolerance), and, per case, the SQP iteration counts of the two finite-difference steps within 1 of each other and at most 5 % of them apart.
"""
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for q in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, q)
import nmpc_family as fam          # noqa: E402

TOL_CAP = 2e-7


def _task(a):
    key, member, over, ns, ms, x0, xm, fd, rows = a
    r = fam.oracle_instance(member, over, ns, ms, x0, xm, fd, rows)
    return key, {k: v for k, v in r.items() if k in fam.LOGS + fam.ILOGS + ("W", "ROW0")}


def main():
    t0 = time.time()
    tasks, meta = [], {}
    for name in fam.case_names():
        member, ns, ms, over = fam.case_spec(name)
        p = fam.load_oracle(member, over)
        x0, xm = fam.starts(name, p.x0_p)
        meta[name] = (member, p, x0, xm)
        for b in range(len(x0)):
            for fd in fam.FD_STEPS:
                tasks.append(((name, b, fd), member, over, ns, ms, x0[b], xm[b], fd, None))
    for member, sw in fam.SWITCHES.items():
        name = member + "_rti"
        _, ns, ms, _ = fam.case_spec(name)
        _, _, x0, xm = meta[name]
        for tag, over in sw.items():
            for b in range(fam.BITE_INSTANCES):
                tasks.append((("bite", member, tag, b), member, over, ns, ms, x0[b], xm[b], fam.FD_STEPS[0], False if tag == "norow" else None))
    tasks.sort(key=lambda a: -(a[3] * a[4] ** 0.3 * (a[2] or {}).get("N", 10) ** 2))      # the long ones first
    with Pool(int(os.environ.get("FAMILY_JOBS", os.cpu_count() or 2))) as pool:
        res = dict(pool.imap_unordered(_task, tasks, chunksize=1))
    print(f"{len(tasks)} oracle runs in {time.time() - t0:.0f} s", flush=True)

    out, e_ref = {}, 0.0
    for name, (member, p, x0, xm) in meta.items():
        runs = {fd: [res[(name, b, fd)] for b in range(len(x0))] for fd in fam.FD_STEPS}
        g = {k: np.stack([r[k] for r in runs[fam.FD_STEPS[0]]], axis=1) for k in fam.LOGS + fam.ILOGS}
        g2 = {k: np.stack([r[k] for r in runs[fam.FD_STEPS[1]]], axis=1) for k in fam.LOGS + fam.ILOGS}
        for k in fam.ILOGS:
            g[k] = g[k].astype(np.int32)
        out.update({f"{name}_{k}": v for k, v in g.items()})
        out[name + "_x0"], out[name + "_xm"] = x0, xm
        er = max(fam.rel_diff(g2[k], g[k]) for k in fam.LOGS)
        out[name + "_eref"] = np.float64(er); e_ref = max(e_ref, er)
        for k in ("STATUS_DYN", "STATUS_SS"):
            assert np.array_equal(g[k], g2[k]), (name, k)
        assert fam.sqp_counts_within_cap([(g2["SQP_DYN"], g["SQP_DYN"])]), (name, "SQP_DYN of the two finite-difference steps", g["SQP_DYN"].T, g2["SQP_DYN"].T)
        dyn, ss = fam.expected_status(name, g["STATUS_DYN"].shape)
        assert np.array_equal(g["STATUS_DYN"], dyn) and np.array_equal(g["STATUS_SS"], ss), (name, g["STATUS_DYN"].T, g["STATUS_SS"].T)
        if member == "c31r":
            out[name + "_ROW0"] = np.stack([r["ROW0"] for r in runs[fam.FD_STEPS[0]]], axis=1)
        print(f"{name:10s} eref {er:.2e}  sqp iterations up to {int(g['SQP_DYN'].max())}", flush=True)
    out["E_ref"] = np.float64(e_ref)

    for member in fam.MEMBERS:
        p = meta[member + "_rti"][1]
        names = [n for n in meta if meta[n][0] == member]
        U = np.concatenate([out[n + "_U"].reshape(-1, p.nu) for n in names])
        assert (np.abs(U - p.umin) < 1e-7).any() or (np.abs(U - p.umax) < 1e-7).any(), (member, "no input bound active")
        if member in ("c41", "d42"):
            gap, nxu = np.inf, p.nx + p.nu
            for n in names:
                for b in range(len(meta[n][2])):
                    W = res[(n, b, fam.FD_STEPS[0])]["W"]
                    N = (W.shape[1] - p.nx) // nxu
                    X = np.stack([W[:, nxu * k:nxu * k + p.nx] for k in range(1, N + 1)], axis=1)
                    with np.errstate(invalid="ignore"):
                        gap = min(gap, float(np.min(np.where(np.isfinite(p.xmax), p.xmax - X, np.inf))), float(np.min(np.where(np.isfinite(p.xmin), X - p.xmin, np.inf))))
            out[member + "_xgap"] = np.float64(gap)
            assert abs(gap) < 1e-7, (member, "no state bound active", gap)
        if member == "c31r":
            assert min(np.nanmin(np.abs(out[f"c31r_{m}_ROW0"])) for m in fam.MODES) < 1e-7, "the row is never active"
        if member == "c22":
            assert (np.concatenate([out[n + "_D_HAT"].ravel() for n in names]) == p.dmax[0]).any(), "the estimate never reaches dmax"
    weak = []
    for member, sw in fam.SWITCHES.items():
        for tag in sw:
            bite = 0.0
            for k in fam.LOGS:
                a = np.stack([res[("bite", member, tag, b)][k] for b in range(fam.BITE_INSTANCES)], axis=1)
                bite = max(bite, fam.rel_diff(a, out[f"{member}_rti_{k}"][:, :fam.BITE_INSTANCES]))
            out[f"bite_{member}_{tag}"] = np.float64(bite)
            print(f"bite {member} {tag}: {bite:.2e}", flush=True)
            weak += [(member, tag, bite)] if bite < 100 * TOL_CAP else []
    assert not weak, weak
    np.savez_compressed(fam.GOLDEN, **out)
    print(f"E_ref {e_ref:.2e}; {os.path.getsize(fam.GOLDEN)} bytes; {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
