"""ops_ab_compare.py DIR_A DIR_B LABEL (recordings of tools/ops_ab_record.py): bit equality (np.array_equal on the raw bytes) of every recorded op output"""
import glob
import os
import sys

import numpy as np

a_dir, b_dir, label = sys.argv[1:4]
fa = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a_dir, "*.npz")))
fb = sorted(os.path.basename(p) for p in glob.glob(os.path.join(b_dir, "*.npz")))
bad, arrays, per_op = [], 0, {}
if fa != fb:
    bad.append(f"different test files recorded: {len(fa)} vs {len(fb)}: {sorted(set(fa) ^ set(fb))[:10]}")
for f in sorted(set(fa) & set(fb)):
    A, B = np.load(os.path.join(a_dir, f)), np.load(os.path.join(b_dir, f))
    node = A["nodeid"].tobytes().decode()
    if sorted(A.files) != sorted(B.files):
        bad.append(f"{node}: different calls {sorted(set(A.files) ^ set(B.files))}")
        continue
    for k in A.files:
        if k == "nodeid":
            continue
        x, y = A[k], B[k]
        op = k.split("_", 1)[1]
        same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(np.frombuffer(x.tobytes(), np.uint8), np.frombuffer(y.tobytes(), np.uint8))
        arrays += 1
        n, m = per_op.get(op, (0, 0))
        per_op[op] = (n + 1, m + (0 if same else 1))
        if not same:
            d = float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) if x.shape == y.shape and x.dtype.kind == "f" else None
            bad.append(f"{node}: {k} differs (max abs diff {d})")
print(f"[{label}] {len(set(fa) & set(fb))} tests, {arrays} recorded outputs, {len(bad)} differences")
for op, (n, m) in sorted(per_op.items()):
    print(f"  {op}: {n} outputs, {m} differ")
for b in bad[:60]:
    print("  DIFF", b)
sys.exit(1 if bad else 0)
