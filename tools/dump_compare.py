#!/usr/bin/env python3
"""Compare two bench.py --dump-outputs directories array by array: tools/dump_compare.py DIR_A DIR_B [label]

Prints one line per .npy (numpy.array_equal, and for arrays that differ the largest absolute difference) and exits 1 unless every
array of DIR_A is in DIR_B with the same bits.  Integer-valued logs (STATUS_DYN, ITERS_DYN) are compared like the others."""
import os
import sys
import numpy as np

a_dir, b_dir = sys.argv[1], sys.argv[2]
label = sys.argv[3] if len(sys.argv) > 3 else f"{a_dir} vs {b_dir}"
names = sorted(f for f in os.listdir(a_dir) if f.endswith(".npy"))
ok = bool(names) and names == sorted(f for f in os.listdir(b_dir) if f.endswith(".npy"))
print(f"# {label}: {len(names)} arrays")
for f in names:
    if not os.path.exists(os.path.join(b_dir, f)):
        print(f"{f[:-4]:12s} MISSING in {b_dir}"); ok = False
        continue
    a, b = np.load(os.path.join(a_dir, f)), np.load(os.path.join(b_dir, f))
    eq = a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    diff = 0.0 if eq or a.shape != b.shape else float(np.nanmax(np.abs(a.astype(float) - b.astype(float))))
    print(f"{f[:-4]:12s} shape {str(a.shape):14s} array_equal={eq}" + ("" if eq else f" max|a-b|={diff:.3e}"))
    ok = ok and eq
print("IDENTICAL" if ok else "DIFFERENT")
sys.exit(0 if ok else 1)
