"""Step time of config-2-shaped f16 trajectories over a long context (profiles/long_context_xattn_ab.txt).

SDXL-base, 1024 x 1024, 30 steps = 31 iterations, CFG 7.5, f16, synthetic weights, a context of --n-ctx tokens (77 per prompt
chunk) through sdxl_diffuser_step_times: p50 of the per-iteration event times of each repeat, three repeats.  Above 96 tokens
every context length is run with the knob "xattn_long" at 0 (projection + attention kernel, as before the long form existed)
and at 1 (the cross-attention inside the query projection's launch), the two alternating A / B / A / B inside one process; the
knob is read when the trajectory sets its context.

    --n-ctx N [N ...]     context lengths (default 154 231 308); up to 96 tokens the knob has no effect and one mode is run
    --profile N           instead: 3 trajectories of 4 steps at n_ctx = N with the knob at 1, then 3 with it at 0 -- the
                          program to put behind `rocprofv3 --kernel-trace --stats --` for the per-launch times of the long
                          fused launch and of the projection + attention pair

One process measures one library; SDXL_LIB_PATH names another build of it (e.g. the parent commit's: it has no knob and runs
every context above 96 tokens un-fused), so the check that the default path has not moved is

    SDXL_LIB_PATH=<parent .so> python tools/long_context_step_times.py --n-ctx 77
    python tools/long_context_step_times.py --n-ctx 77
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ctx", type=int, nargs="+", default=[154, 231, 308])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile", type=int, default=0, metavar="N_CTX")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    cfg = pkg.sdxl_base_config()
    g = torch.Generator().manual_seed(131)
    r = lambda *s: torch.randn(*s, generator=g)
    y, uy, noise0 = r(1, cfg.adm_in_channels).cuda(), r(cfg.adm_in_channels).cuda(), r(1, 4, 128, 128).cuda()
    d = pkg.Diffuser(ctx, cfg, pkg.DTYPE_F16, seed=0)
    lib = os.path.basename(os.path.dirname(os.environ["SDXL_LIB_PATH"])) if os.environ.get("SDXL_LIB_PATH") else "this build"
    has_knob = True
    try:
        pkg.debug_set("xattn_long", 1)
    except pkg.EngineError:
        has_knob = False      # an older build: every context above 96 tokens is un-fused there

    def cond(n_ctx):
        return pkg.Conditioning(context_full=r(1, n_ctx, cfg.context_dim).cuda(), channel_context=y,
                                unconditional_context_full=r(n_ctx, cfg.context_dim).cuda(), unconditional_channel_context=uy, resolution=(1024, 1024))

    def run(c, knob, n_steps):
        if has_knob:
            pkg.debug_set("xattn_long", knob)
        return d.sample_latent(c, 7.5, n_steps, noise0)

    if args.profile:
        c = cond(args.profile)
        for knob in (1, 0):
            for _ in range(3):
                run(c, knob, 4)
            torch.cuda.synchronize()
        return

    d.enable_step_timing(True)
    for n_ctx in args.n_ctx:
        c = cond(n_ctx)
        knobs = (0, 1) if n_ctx > 96 and has_knob else (1,)
        run(c, knobs[0], 2)                  # plan + graph capture
        for knob in knobs:                   # warm every kernel the timed window uses
            run(c, knob, 30)
        torch.cuda.synchronize()
        for rep in range(args.repeats):
            for knob in knobs:
                run(c, knob, 30)
                torch.cuda.synchronize()
                ms = d.step_times_ms()
                print(json.dumps({"lib": lib, "n_ctx": n_ctx, "xattn_long": knob if n_ctx > 96 and has_knob else None, "repeat": rep, "iterations": len(ms),
                                  "step_ms_p50": round(statistics.median(ms), 4), "step_ms_min": round(min(ms), 4), "step_ms_max": round(max(ms), 4)}), flush=True)
    if has_knob:
        pkg.debug_set("xattn_long", 1)


if __name__ == "__main__":
    main()
