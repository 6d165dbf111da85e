"""Step time on noise-level schedules (profiles/levels_times.txt): DPM-Solver++(2M) and DPM++ 3M SDE on a 30-entry Karras sigma
list against 2M on the default schedule, on this library and on the parent commit's, and bench.py's line on both.

Config-2-shaped sampling (SDXL-base, 1024 x 1024, CFG 7.5, f16, synthetic weights, the seeded call at eta 0) through
sdxl_diffuser_step_times: p50 of the per-iteration event times of a trajectory.  One child process measures one library (SDXL_LIB_PATH names
the parent's build, which knows the default schedule only); the driver starts the children one after the other, the two libraries alternating,
and then bench.py the same way.

    python tools/levels_times.py --parent-lib <parent commit's libsdxl_mi355.so> [--rounds 2] [--bench-steps 3] [--bench-warmup 1]
    python tools/levels_times.py --worker [--levels]        (what the driver starts; --levels: also the sigma-list modes)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 30


def worker(levels, repeats):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    cfg = pkg.sdxl_base_config()
    g = torch.Generator().manual_seed(131)
    r = lambda *s: torch.randn(*s, generator=g)
    cond = pkg.Conditioning(context_full=r(1, 77, cfg.context_dim).cuda(), channel_context=r(1, cfg.adm_in_channels).cuda(),
                            unconditional_context_full=r(77, cfg.context_dim).cuda(),
                            unconditional_channel_context=r(cfg.adm_in_channels).cuda(), resolution=(1024, 1024))
    d = pkg.Diffuser(ctx, cfg, pkg.DTYPE_F16, seed=0)
    modes = [("2m default schedule", "dpmpp_2m", False)]
    if levels:
        modes += [("2m karras", "dpmpp_2m", True), ("3m karras", "dpmpp_3m", True)]
        karras = pkg.sigma_schedule("karras", N)

    def run(solver, on_sigmas):
        d.set_solver(solver)
        if levels:
            d.set_sigmas(karras if on_sigmas else None)
        return d.sample_latent(cond, 7.5, N, seeds=[1234], eta=0.0)

    d.enable_step_timing(True)
    for _, solver, on_sigmas in modes:          # plan, graph capture, every kernel the timed window uses
        run(solver, on_sigmas)
    torch.cuda.synchronize()
    lib = os.path.basename(os.path.dirname(os.path.dirname(os.environ["SDXL_LIB_PATH"]))) if os.environ.get("SDXL_LIB_PATH") else "this build"
    for rep in range(repeats):
        for label, solver, on_sigmas in modes:
            run(solver, on_sigmas)
            torch.cuda.synchronize()
            ms = d.step_times_ms()
            print(json.dumps({"lib": lib, "mode": label, "repeat": rep, "iterations": len(ms), "step_ms_p50": round(statistics.median(ms), 4),
                              "step_ms_min": round(min(ms), 4), "step_ms_max": round(max(ms), 4)}), flush=True)


def child(cmd, lib, limit):
    """one fresh process on one library; its stdout lines are passed through"""
    env = dict(os.environ)
    env.pop("SDXL_LIB_PATH", None)
    if lib:
        env["SDXL_LIB_PATH"] = lib
    p = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd)} on {lib or 'this build'} ended with status {p.returncode}: nothing more is started")
    return [l for l in p.stdout.splitlines() if l.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--levels", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=3)
    ap.add_argument("--bench-warmup", type=int, default=1)
    args = ap.parse_args()
    if args.worker:
        return worker(args.levels, args.repeats)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        ap.error("--parent-lib: the parent commit's libsdxl_mi355.so")
    parent = os.path.abspath(args.parent_lib)
    me = os.path.join("tools", "levels_times.py")
    for rnd in range(args.rounds):
        for lib in (parent, None):
            for line in child([me, "--worker", "--repeats", str(args.repeats)] + ([] if lib else ["--levels"]), lib, 600):
                print(json.dumps(dict(json.loads(line), round=rnd, lib="parent" if lib else "this")), flush=True)
    for rnd in range(args.rounds):
        for lib in (parent, None):
            for line in child(["bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)], lib, 900):
                b = json.loads(line)
                keep = {k: b[k] for k in b if not isinstance(b[k], (dict, list))}
                print(json.dumps(dict(keep, round=rnd, lib="parent" if lib else "this", tool="bench.py")), flush=True)


if __name__ == "__main__":
    main()
