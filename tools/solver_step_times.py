"""Step time of the DPM-Solver++(2M) trajectories against the DDIM ones (profiles/solver_step_times.txt).

Config-2-shaped sampling (SDXL-base, 1024 x 1024, 30 steps = 31 iterations, CFG 7.5, f16, synthetic weights) through
sdxl_diffuser_step_times: p50 of the per-iteration event times of each repeat, three repeats, the solvers alternating inside
every repeat.

    --solver NAME[:ETA]   repeatable; NAME ddim | dpmpp_2m.  Without ETA the explicit-noise call (noise0 as a tensor), with
                          ETA the seeded call.  Default: --solver ddim
    --prediction NAME     epsilon (default) | v: the handle's prediction type for every run of this process (DESIGN 3.7,
                          profiles/prediction_step_times.txt); "v" also hands the handle the zero-terminal-SNR table
    --e2e                 afterwards, whole sample_latent calls under a host clock (ends in a synchronise), step timing off:
                          DDIM at 30 steps, 2M at 20 and at 15 -- latents/s of the sampler alone, a step-count comparison
                          at unmeasured image quality

One process measures one library; SDXL_LIB_PATH names another build of it (e.g. the parent commit's, which knows `ddim`
only), so an A/B is

    SDXL_LIB_PATH=<parent .so> python tools/solver_step_times.py --solver ddim
    python tools/solver_step_times.py --solver ddim --solver dpmpp_2m:0 --solver dpmpp_2m:1 --e2e
    python tools/solver_step_times.py --prediction v --solver ddim --solver dpmpp_2m
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solver", action="append", default=None, metavar="NAME[:ETA]")
    ap.add_argument("--prediction", default="epsilon", choices=["epsilon", "v"])
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    modes = []
    for m in args.solver or ["ddim"]:
        name, _, eta = m.partition(":")
        if name not in ("ddim", "dpmpp_2m"):
            ap.error(f"unknown solver {name}")
        modes.append((m, name, float(eta) if eta else None))

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
    noise0 = r(1, 4, 128, 128).cuda()
    v_pred = args.prediction == "v"      # a library that knows epsilon only is never asked
    d = pkg.Diffuser(ctx, cfg, pkg.DTYPE_F16, seed=0,
                     alphas_cumprod=pkg.rescale_zero_terminal_snr(pkg.default_alphas_cumprod()) if v_pred else None)
    if v_pred:
        d.set_prediction("v")
    current = ["ddim"]

    def run(name, eta, n_steps):
        if name != current[0]:           # a library that knows DDIM only is never asked
            d.set_solver(name)
            current[0] = name
        if eta is None:
            return d.sample_latent(cond, 7.5, n_steps, noise0)
        return d.sample_latent(cond, 7.5, n_steps, seeds=[1234], eta=eta)

    d.enable_step_timing(True)
    run("ddim", None, 2)                 # plan + graph capture
    for _, name, eta in modes:           # warm every kernel the timed window uses
        run(name, eta, 30)
    torch.cuda.synchronize()
    lib = os.path.basename(os.environ.get("SDXL_LIB_PATH", "this build"))
    for rep in range(args.repeats):
        for label, name, eta in modes:
            run(name, eta, 30)
            torch.cuda.synchronize()
            ms = d.step_times_ms()
            print(json.dumps({"lib": lib, "prediction": args.prediction, "mode": label, "repeat": rep, "iterations": len(ms), "step_ms_p50": round(statistics.median(ms), 4),
                              "step_ms_min": round(min(ms), 4), "step_ms_max": round(max(ms), 4)}), flush=True)
    if args.e2e:
        d.enable_step_timing(False)
        jobs = [("ddim", 30), ("dpmpp_2m", 20), ("dpmpp_2m", 15)]
        for name, n_steps in jobs:
            run(name, 0.0, n_steps)
        torch.cuda.synchronize()
        for rep in range(args.repeats):
            for name, n_steps in jobs:
                t0 = time.perf_counter()
                run(name, 0.0, n_steps)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print(json.dumps({"lib": lib, "mode": f"e2e {name} eta 0", "n_steps": n_steps, "iterations": pkg.step_count(n_steps), "repeat": rep,
                                  "call_ms": round(dt * 1e3, 2), "latents_per_s": round(1.0 / dt, 4)}), flush=True)


if __name__ == "__main__":
    main()
