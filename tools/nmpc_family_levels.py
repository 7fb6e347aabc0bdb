#!/usr/bin/env python3
"""Measured levels of the non-linear tracking family (tests/nmpc_family.py) on the GPU, per member, mode and kernel: the largest difference relative to
1 + |value| over U, X_HAT, XS, US, Xp, D_HAT against the oracle's committed logs (tests/golden/nmpc_family.npz) and, for kernels 3 and 4, against
kernel 1 - what tests/test_nmpc_family.py takes TOL_ORACLE and TOL_KERNELS from.  Writes profiles/nmpc_family_parity.txt (or the path given).

    python tools/nmpc_family_levels.py [OUT]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, q)
import nmpc_family as fam              # noqa: E402
import test_nmpc_family as t           # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nmpc_family_parity.txt")
    gold = {k: v for k, v in np.load(fam.GOLDEN).items()}
    lines = ["# tools/nmpc_family_levels.py on one MI355X: max |gpu - ref| / (1 + |ref|) over U, X_HAT, XS, US, Xp, D_HAT",
             "# case        kernel  vs oracle  vs kernel 1  status words  SQP_DYN within 1 of the oracle's  (E_ref of the case: the oracle at finite-difference steps 1e-6 | 3e-6)"]
    worst_o = worst_k = 0.0
    pairs = {}
    for name in fam.case_names():
        for kernel in (1, 3, 4):
            r = t.gpu_run(name, kernel, gold)
            lo = max(fam.rel_diff(r[k], gold[f"{name}_{k}"]) for k in fam.LOGS)
            lk = 0.0 if kernel == 1 else max(fam.rel_diff(r[k], t.gpu_run(name, 1, gold)[k]) for k in fam.LOGS)
            st = all(np.array_equal(r[k], gold[f"{name}_{k}"]) for k in ("STATUS_DYN", "STATUS_SS"))
            cap = int(np.abs(r["SQP_DYN"].astype(np.int64) - gold[name + "_SQP_DYN"]).max()) <= 1
            if name in fam.SQP_CASES:
                pairs.setdefault(kernel, []).append((r["SQP_DYN"], gold[name + "_SQP_DYN"]))
            ndiff = int((r["SQP_DYN"] != gold[name + "_SQP_DYN"]).sum())
            worst_o, worst_k = max(worst_o, lo), max(worst_k, lk)
            lines.append(f"{name:12s}  {kernel}       {lo:.2e}   {'-' if kernel == 1 else f'{lk:.2e}':9s}    {'equal' if st else 'DIFFER'}         {'yes' if cap else 'NO'} ({ndiff} of {r['SQP_DYN'].size} apart)      {float(gold[name + '_eref']):.1e}")
            print(lines[-1], flush=True)
    e_ref = float(gold["E_ref"])
    lines += [f"# largest level against the oracle {worst_o:.2e}, between the kernels {worst_k:.2e}; E_ref {e_ref:.2e}",
              f"# TOL_ORACLE = min(2e-7, max(4 x {worst_o:.2e}, 10 x {e_ref:.2e})) = {min(2e-7, max(4 * worst_o, 10 * e_ref)):.1e};  TOL_KERNELS = min(1e-7, 4 x {worst_k:.2e}) = {min(1e-7, 4 * worst_k):.1e}"]
    for kernel, pr in pairs.items():
        lines.append(f"# kernel {kernel}: {sum(int((a != g).sum()) for a, g in pr)} of {sum(g.size for _, g in pr)} SQP iteration counts of the sqp cases apart from the oracle's (cap: 5 %): "
                     + ("within" if fam.sqp_counts_within_cap(pr) else "NOT within"))
    print("\n".join(lines[-5:]))
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
