"""Few-step sampling against the default trajectory (profiles/fewstep_times.txt).

SDXL-base on synthetic weights, a 128 x 128 latent (1024 x 1024), f16, guidance off (SDXL_GUIDANCE_OFF: the conditional branch alone, as a
distilled checkpoint is run), n = 1 and n = 4, the VAE in the bench line's mode (f32_split).  One process, three repeats, the variants
alternating inside every repeat:

    images/s   whole sample_latent + latent_to_image calls under a host clock that ends in a synchronise: a 4-entry LCM list
               (timestep_schedule("lcm", 4), solver "lcm") against the default 31-iteration DDIM trajectory (n_steps 30)
    step p50   p50 of sdxl_diffuser_step_times for LCM against DDIM on the same 4-entry list (seeded, eta 0), and of the default
               31-iteration trajectory: this box's default-path step time, next to which the other numbers are read

Synthetic weights give no image to judge: the step counts are those the published checkpoints are run with, the quality is not measured."""
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    cfg = pkg.sdxl_base_config()
    d = pkg.Diffuser(ctx, cfg, pkg.DTYPE_F16, seed=0)
    d.set_guidance(mode="off")
    vae = pkg.LatentDecoder(ctx, None, pkg.DTYPE_F32_SPLIT, seed=0)
    lcm4 = pkg.timestep_schedule("lcm", 4)
    g = torch.Generator().manual_seed(131)
    r = lambda *s: torch.randn(*s, generator=g)

    def configure(solver, ts):
        d.set_solver(solver)
        d.set_timesteps(ts)

    variants = [("lcm, list %s" % lcm4, "lcm", lcm4, 4), ("ddim, list %s" % lcm4, "ddim", lcm4, 4), ("ddim, default 31 iterations", "ddim", None, 30)]
    for n in args.batches:
        cond = pkg.Conditioning(context_full=r(n, 77, cfg.context_dim).cuda(), channel_context=r(n, cfg.adm_in_channels).cuda(), resolution=(1024, 1024))
        seeds = list(range(1234, 1234 + n))

        def image(n_steps):
            return vae.latent_to_image(d.sample_latent(cond, 1.0, n_steps, seeds=seeds, eta=0.0))

        for _, solver, ts, n_steps in variants:         # plans, graph capture, every kernel of the timed window
            configure(solver, ts)
            image(n_steps)
        torch.cuda.synchronize()
        for rep in range(args.repeats):
            for label, solver, ts, n_steps in variants:
                configure(solver, ts)
                d.enable_step_timing(True)
                d.sample_latent(cond, 1.0, n_steps, seeds=seeds, eta=0.0)
                torch.cuda.synchronize()
                ms = d.step_times_ms()
                d.enable_step_timing(False)
                t0 = time.perf_counter()
                image(n_steps)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print(json.dumps({"n": n, "variant": label, "repeat": rep, "iterations": len(ms), "step_ms_p50": round(statistics.median(ms), 4),
                                  "step_ms_min": round(min(ms), 4), "step_ms_max": round(max(ms), 4), "call_ms": round(dt * 1e3, 2),
                                  "images_per_s": round(n / dt, 4)}), flush=True)
    configure("ddim", None)


if __name__ == "__main__":
    main()
