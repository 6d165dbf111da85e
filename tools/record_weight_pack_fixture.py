"""Writes tests/golden/weight_pack_bits.npz: every case of tests/weight_pack_cases.py on the loaded library.

    SDXL_LIB_PATH=<library of the parent commit> timeout -k 10 900 python tools/record_weight_pack_fixture.py --parent <commit> [--out ...]

The fixture was recorded ONCE, from a library built from commit a9939e9 -- the last one with six packing routines in WeightBuilder (linear,
linear_hilo, fused_linear, linear_ln, fused_linear_ln, fold_ln) and arenas sized by WeightBuilder::arena_bound; `git diff a9939e9 -- csrc/` was
empty when it was built.  It pins what the one routine that replaced them packs and lays out.  Do not run this again to make
tests/test_gpu_weight_pack.py or tests/test_cpu_weight_layout.py pass: a failing case there means a packed byte or an arena offset changed.  It
stays in the tree as the record of how the file was made, and for a case a new packing form needs (record the new case alone, from a library
that passes the old ones, and merge it into the file).  Every case runs twice and must give equal bits; one the loaded library does not reproduce
is named in the meta record and left out (at most one in ten).  `--parent` is written into the meta record as given.  Layout: the cases module.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def hipcc_version():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c:
            try:
                out = subprocess.run([c, "--version"], capture_output=True, text=True).stdout
            except OSError:
                continue
            return "; ".join(ln.strip() for ln in out.splitlines() if "version" in ln.lower()) or out.strip()
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="hash of the commit the loaded library was compiled from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "weight_pack_bits.npz"))
    args = ap.parse_args()

    import __graft_entry__ as ge
    import weight_pack_cases as C
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    arrays, names, unstable = {}, [], []
    cases = C.all_cases()
    for c in cases:
        name = C.case_name(c)
        outs, ints = C.run_case(pkg, ctx, c)
        outs2, ints2 = C.run_case(pkg, ctx, c)
        if ints != ints2 or {k: v[0] for k, v in outs.items()} != {k: v[0] for k, v in outs2.items()}:
            unstable.append(name)
            print(f"NOT REPRODUCED, left out: {name}", flush=True)
            continue
        for k, (sha, sample) in outs.items():
            assert np.isfinite(sample).all(), name
            arrays[f"sha/{name}/{k}"] = np.array(sha)
            arrays[f"sample/{name}/{k}"] = sample
        for k, v in ints.items():
            arrays[f"int/{name}/{k}"] = np.array(v, dtype=np.int64)
        names.append(name)
        print(f"{name}: {ints} {' '.join(v[0][:12] for v in outs.values())}", flush=True)
    assert 10 * len(unstable) <= len(cases), unstable
    arrays["meta"] = np.array(json.dumps({
        "parent_commit": args.parent, "hipcc": hipcc_version(), "build_info": pkg.lib().sdxl_build_info().decode(), "library": os.path.basename(pkg.LIB_PATH),
        "recorded_by": "tools/record_weight_pack_fixture.py", "cases": names, "not_reproduced": unstable}))
    np.savez_compressed(args.out, **arrays)
    print(f"{len(names)} cases ({len(unstable)} left out) -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
