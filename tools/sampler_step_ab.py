"""A/B of the per-step kernel between two builds of the library (profiles/sampler_step_ab.txt): SDXL-base, f16, 1024 x 1024, n = 1, seeded DDIM
eta 0, 10 steps -- the workload of tools/guidance_step_cost.py, which every child process here runs with SDXL_LIB_PATH naming its library.

    timeout -k 10 1100 python tools/sampler_step_ab.py --a <parent library> --b <this library> [--repeats 3] > profiles/sampler_step_ab.txt

Per repeat and library, libraries alternating, one fresh process each:
  * a kernel trace (rocprofv3 --kernel-trace --stats, a run of its own): the durations of the update launches of the per-step kernel (whatever it is
    called in that library), split by the trajectory they belong to -- a trajectory is one initial launch and ten updates, and the tool runs the
    option sets in a fixed order -- and their median for default options and for scales = [7.5];
  * an untraced run: the p50 step time the tool reports for the same two option sets.  Reported, nothing is judged on it: machines and sessions
    differ by several per cent, and the kernel is on the order of 0.05 % of a step.
Verdict per option set: B's median over repeats must not exceed A's largest per-repeat median (B stays inside A's own repeat-to-repeat spread).
A child that fails or runs into its time limit ends the whole run at once.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "guidance_step_cost.py")
MODES = ("default", "scales", "rescale")      # the order tools/guidance_step_cost.py runs them in; two warm rounds first
STEP_KERNELS = ("step_kernel", "ddim_kernel", "dpmpp2m_kernel")       # guided_step_kernel ends in step_kernel
ITERS = 10


def child(cmd, lib, limit):
    env = dict(os.environ, SDXL_LIB_PATH=os.path.abspath(lib))
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, capture_output=True, text=True)      # the limit ends the child's own children too
    if r.returncode != 0:
        sys.exit(f"child failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def traced(lib):
    """-> {mode: [update-launch durations in us of the timed trajectory]}"""
    with tempfile.TemporaryDirectory() as td:
        child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "t", "--",
               sys.executable, TOOL, "--repeats", "1", "--steps", str(ITERS)], lib, 300)
        f = sorted(glob.glob(td + "/**/*kernel_trace.csv", recursive=True))[0]
        rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f)))
    rows = [(e - s) / 1e3 for s, e, n in rows if n.split("(")[0].split("<")[0].endswith(STEP_KERNELS)]
    per = ITERS + 1
    assert len(rows) == 3 * len(MODES) * per, f"{len(rows)} step-kernel rows, expected {3 * len(MODES) * per}"
    return {m: rows[(2 * len(MODES) + j) * per + 1:(2 * len(MODES) + j + 1) * per] for j, m in enumerate(MODES)}


def untraced(lib):
    out = child([sys.executable, TOOL, "--repeats", "2", "--steps", str(ITERS)], lib, 300)
    p50 = {}
    for ln in out.splitlines():
        if ln.startswith("{"):
            d = json.loads(ln)
            p50.setdefault(d["mode"], []).append(d["step_ms_p50"])
    return {m: statistics.median(v) for m, v in p50.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True, help="library A (the parent commit's build)")
    ap.add_argument("--b", required=True, help="library B (this tree's build)")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    libs = {"A": args.a, "B": args.b}
    print(f"# timeout -k 10 1100 python tools/sampler_step_ab.py --a {args.a} --b {args.b} --repeats {args.repeats} > profiles/sampler_step_ab.txt")
    print("# A = the parent commit's library (ddim_kernel / guided_step_kernel), B = this tree's (step_kernel).  kernel_us: update launches of the timed")
    print("# trajectory, from a kernel trace; step_ms_p50: the untraced tool's own figure.  One fresh process per row, libraries alternating.", flush=True)
    med, step = {}, {}
    for rep in range(args.repeats):
        for name, lib in libs.items():
            t = traced(lib)
            for m in ("default", "scales"):
                med.setdefault((name, m), []).append(statistics.median(t[m]))
                print(json.dumps({"lib": name, "repeat": rep, "mode": m, "kernel_us_median": round(statistics.median(t[m]), 3),
                                  "kernel_us_min": round(min(t[m]), 3), "kernel_us_max": round(max(t[m]), 3), "launches": len(t[m])}), flush=True)
        for name, lib in libs.items():
            u = untraced(lib)
            for m in ("default", "scales"):
                step.setdefault((name, m), []).append(u[m])
                print(json.dumps({"lib": name, "repeat": rep, "mode": m, "step_ms_p50": round(u[m], 4)}), flush=True)
    ok = True
    for m in ("default", "scales"):
        a, b = med[("A", m)], med[("B", m)]
        passed = statistics.median(b) <= max(a)
        ok &= passed
        print(f"# {m}: kernel median over repeats A {statistics.median(a):.3f} us (per repeat {min(a):.3f} .. {max(a):.3f}), B {statistics.median(b):.3f} us "
              f"(per repeat {min(b):.3f} .. {max(b):.3f}): {'inside' if passed else 'OUTSIDE'} A's spread;  step p50 A {statistics.median(step[('A', m)]):.4f} ms, "
              f"B {statistics.median(step[('B', m)]):.4f} ms (reported only)")
    sys.exit(0 if ok else 2)


if __name__ == "__main__":
    main()
