"""Writes tests/golden/nmpc_inst_setpoints.npz: the oracle's loops (oracle/nmpc_oracle.py, instance by instance, tests/nmpc_inst_setpoints_ref.py) of the
cases the GPU tests of per-instance set points compare with, and the inputs they were run on.  Minutes on one core, no GPU:

    python tests/golden/make_nmpc_inst_setpoints_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)

import nmpc_inst_setpoints_ref as ref      # noqa: E402

out = {}
for case, noisy in ref.GOLDEN_CASES:
    r = ref.oracle_run(case, noisy)
    ysp, usp, v, w = ref.inputs(case, noisy)
    for k, a in r.items():
        out[ref.golden_key(case, noisy, k)] = a
    out[ref.golden_key(case, noisy, "ysp")] = ysp; out[ref.golden_key(case, noisy, "usp")] = usp
    print(case, noisy, "STATUS_SS", np.unique(r["STATUS_SS"]).tolist(), "STATUS_DYN", np.unique(r["STATUS_DYN"]).tolist())
np.savez_compressed(ref.GOLDEN, **out)
print("wrote", ref.GOLDEN, os.path.getsize(ref.GOLDEN), "bytes")
