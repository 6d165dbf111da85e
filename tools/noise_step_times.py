"""Step time of the seeded trajectories against the explicit-noise ones (profiles/seeded_noise_step_times.txt).

Config-2-shaped sampling (SDXL-base, 1024 x 1024, 30 steps = 31 iterations, CFG 7.5, f16, synthetic weights) through
sdxl_diffuser_step_times: p50 of the per-iteration event times of each repeat.  Modes:

    explicit   noise0 as a tensor (works on any build of the library)
    eta0 eta1  the seeded call with eta = 0 / 1
    inpaint    one 100-step inpainting call end to end (host clock around work that ends in a synchronise): explicit,
               including the host's generation and upload of step_noise, and seeded

One process measures one library; SDXL_LIB_PATH names another build of it (e.g. the parent commit's), so an A/B is

    SDXL_LIB_PATH=<parent .so> python tools/noise_step_times.py explicit
    python tools/noise_step_times.py explicit eta0 eta1 inpaint
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    modes = sys.argv[1:] or ["explicit"]
    ctx = pkg.Context(0)
    cfg = pkg.sdxl_base_config()
    g = torch.Generator().manual_seed(131)
    r = lambda *s: torch.randn(*s, generator=g)
    cond = pkg.Conditioning(context_full=r(1, 77, cfg.context_dim).cuda(), channel_context=r(1, cfg.adm_in_channels).cuda(),
                            unconditional_context_full=r(77, cfg.context_dim).cuda(),
                            unconditional_channel_context=r(cfg.adm_in_channels).cuda(), resolution=(1024, 1024))
    noise0 = r(1, 4, 128, 128).cuda()
    d = pkg.Diffuser(ctx, cfg, pkg.DTYPE_F16, seed=0)
    d.enable_step_timing(True)
    runs = {"explicit": lambda: d.sample_latent(cond, 7.5, 30, noise0),
            "eta0": lambda: d.sample_latent(cond, 7.5, 30, seeds=[1234], eta=0.0),
            "eta1": lambda: d.sample_latent(cond, 7.5, 30, seeds=[1234], eta=1.0)}
    d.sample_latent(cond, 7.5, 2, noise0)                 # plan + graph capture
    d.sample_latent(cond, 7.5, 30, noise0)                # warm
    torch.cuda.synchronize()
    lib = os.path.basename(os.environ.get("SDXL_LIB_PATH", "this build"))
    for rep in range(3):                                  # the modes alternate inside every repeat
        for m in modes:
            if m not in runs:
                continue
            runs[m]()
            torch.cuda.synchronize()
            ms = d.step_times_ms()
            print(json.dumps({"lib": lib, "mode": m, "repeat": rep, "iterations": len(ms), "step_ms_p50": round(statistics.median(ms), 4),
                              "step_ms_min": round(min(ms), 4), "step_ms_max": round(max(ms), 4)}), flush=True)
    if "inpaint" in modes:
        d.enable_step_timing(False)
        iters = pkg.step_count(100)
        reference = r(1, 4, 128, 128).cuda()
        mask = torch.zeros(1, 4, 128, 128, dtype=torch.bool)
        mask[:, :, 32:96, 32:96] = True
        mask = mask.cuda()

        def explicit():
            hg = torch.Generator().manual_seed(7)
            n0 = torch.randn(1, 4, 128, 128, generator=hg).cuda()
            sn = torch.randn(iters, 1, 4, 128, 128, generator=hg).cuda()
            return d.sample_latent_with_inpainting(cond, 7.5, 100, reference, mask, n0, sn)

        def seeded_call():
            return d.sample_latent_with_inpainting(cond, 7.5, 100, reference, mask, seeds=[7])

        for rep in range(2):
            for name, fn in (("inpaint_explicit", explicit), ("inpaint_seeded", seeded_call)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                print(json.dumps({"lib": lib, "mode": name, "repeat": rep, "iterations": iters,
                                  "call_ms": round((time.perf_counter() - t0) * 1e3, 2)}), flush=True)


if __name__ == "__main__":
    main()
