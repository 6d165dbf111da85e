"""Step time of a trajectory with CFG rescale against the same trajectory without (profiles/guidance_step_cost.txt).

SDXL-base, 1024 x 1024 (64 moment blocks per entry), n = 1, f16, synthetic weights, seeded DDIM at eta 0, 10 steps, through
sdxl_diffuser_step_times: p50 of the per-iteration event times of each repeat, the two option sets alternating on ONE handle in one
process.  "scales" is the step kernel with guidance options but no rescale (no extra launch); "rescale" adds the moments and factor
launches in front of it on every iteration.

    timeout -k 10 240 python tools/guidance_step_cost.py [--repeats 5] > profiles/guidance_step_cost.txt

(about 40 s on an MI355X; the limit ends a run that hangs.)  The output starts with that command and what the rows are.
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()

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
    modes = [("default", dict()), ("scales", dict(scales=[7.5])), ("rescale", dict(rescale=0.7))]

    def run(options):
        d.set_guidance(**options)
        return d.sample_latent(cond, 7.5, args.steps, seeds=[1234], eta=0.0)

    print("# timeout -k 10 240 python tools/guidance_step_cost.py --repeats %d --steps %d > profiles/guidance_step_cost.txt" % (args.repeats, args.steps))
    print("# SDXL-base, synthetic weights, f16, 1024 x 1024, n = 1, seeded DDIM eta 0, CFG 7.5; one handle, one process, modes alternating.")
    print("# default: default options.  scales: guided step kernel, no rescale (no extra launch).  rescale: phi = 0.7, moments + factor launches")
    print("# in front of the step kernel on every iteration.  step_ms_*: per-iteration event times of one trajectory.  No bar: box noise is several per cent.")
    d.enable_step_timing(True)
    for _, options in modes * 2:          # plan + graph capture, then every kernel of the timed window once more
        run(options)
    torch.cuda.synchronize()
    p50 = {}
    for rep in range(args.repeats):
        for label, options in modes:
            run(options)
            torch.cuda.synchronize()
            ms = d.step_times_ms()
            print(json.dumps({"mode": label, "repeat": rep, "iterations": len(ms), "step_ms_p50": round(statistics.median(ms), 4),
                              "step_ms_min": round(min(ms), 4), "step_ms_max": round(max(ms), 4)}), flush=True)
            p50.setdefault(label, []).append(statistics.median(ms))
    print("# median of the repeats' p50: " + ", ".join(f"{k} {statistics.median(v):.4f} ms" for k, v in p50.items()))


if __name__ == "__main__":
    main()
