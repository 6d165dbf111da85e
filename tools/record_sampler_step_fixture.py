"""Writes tests/golden/sampler_step_bits.npz: every case of tests/sampler_step_cases.py through sdxl_sampler_step_replay, on the loaded library.

    timeout -k 10 120 python tools/record_sampler_step_fixture.py --parent <commit> [--out tests/golden/sampler_step_bits.npz]

The fixture was recorded ONCE, from a library whose per-step kernels were still the text of commit 456ca47 (ddim_kernel, dpmpp2m_kernel,
guided_step_kernel: `git diff 456ca47 -- csrc/elementwise.hip` was empty), and pins the bits of the one step_kernel that replaced them.  Do not
run this again to make tests/test_gpu_sampler_step.py pass: a failing case there means a rounding of the kernel changed.  It stays in the tree as
the record of how the file was made, and for a new case that an added option needs (record the new case alone, from a library whose kernel passes the
old ones, and merge it into the file).  `--parent` is written into the file's meta record as given; the hipcc line is read from `hipcc --version`.
Layout and the note on toolchains: tests/sampler_step_cases.py.
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
    ap.add_argument("--parent", required=True, help="hash of the commit whose step kernels the loaded library was compiled from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sampler_step_bits.npz"))
    args = ap.parse_args()

    import __graft_entry__ as ge
    import sampler_step_cases as C
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    alphas = pkg.default_alphas_cumprod()
    arrays = {"in/alphas": alphas}
    inputs = {}
    for shape in C.SHAPES:
        inputs[shape] = C.make_inputs(shape)
        for k, v in inputs[shape].items():
            arrays[f"in/{C.shape_key(shape)}/{k}"] = v
    cases = C.all_cases()
    for c in cases:
        packed, h_lat, h_ts = C.run_case(pkg, ctx, c, inputs[tuple(c["shape"])], alphas)
        again = C.run_case(pkg, ctx, c, inputs[tuple(c["shape"])], alphas)
        assert np.array_equal(packed.numpy().view(np.uint32), again[0].numpy().view(np.uint32)) and (h_lat, h_ts) == again[1:], C.case_name(c)
        assert np.isfinite(packed.numpy()).all(), C.case_name(c)
        arrays["out/" + C.case_name(c)] = packed.numpy()
        arrays["sha/" + C.case_name(c)] = np.array([h_lat, h_ts])
    arrays["meta"] = np.array(json.dumps({
        "parent_commit": args.parent, "hipcc": hipcc_version(), "build_info": pkg.lib().sdxl_build_info().decode(),
        "recorded_by": "tools/record_sampler_step_fixture.py", "cases": [C.case_name(c) for c in cases]}))
    np.savez_compressed(args.out, **arrays)
    print(f"{len(cases)} cases -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
