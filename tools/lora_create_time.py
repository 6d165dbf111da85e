"""Creation cost of create-time adapters (profiles/lora_create_time.txt).

SDXL-base UNet, f16, synthetic weights of one seed: sdxl_unet_create_synthetic against sdxl_unet_create_lora with a rank-16 adapter on every
attention Linear (query / key / value / out of attn1 and attn2 of all 70 transformer blocks, 560 entries, host arrays).  One process, each variant
twice, alternating; wall clock around the create call, which ends synchronised (the builder waits for its stream).

    python tools/lora_create_time.py [--rank 16] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    cfg = pkg.sdxl_base_config()
    specs = pkg.unet_param_specs(cfg)
    rng = np.random.default_rng(5)
    entries, floats = [], 0
    for i, p in enumerate(specs):
        if p.kind == 0 and (".attn1." in p.name or ".attn2." in p.name):
            d_in, d_out = p.shape
            down = (rng.standard_normal((args.rank, d_in)) / np.sqrt(d_in)).astype(np.float32)
            up = (rng.standard_normal((d_out, args.rank)) * 0.05).astype(np.float32)
            entries.append(pkg.lora_entry(i, down, up))
            floats += down.size + up.size
    lines = [f"SDXL-base UNet, DTYPE_F16, synthetic seed 0; adapter: rank {args.rank} on {len(entries)} attention Linears ({floats * 4 / 1e6:.1f} MB of host arrays)"]

    def create(lora):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u = pkg.UNet(ctx, cfg, pkg.DTYPE_F16, seed=0, lora=lora)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del u
        return dt

    times = {"plain": [], "lora": []}
    for rep in range(2):
        for name, lora in (("plain", None), ("lora", entries)):
            times[name].append(create(lora))
            lines.append(f"repeat {rep} {name:5s} create {times[name][-1] * 1e3:9.1f} ms")
    best = {k: min(v) for k, v in times.items()}
    lines.append(f"best of two: plain {best['plain'] * 1e3:.1f} ms, lora {best['lora'] * 1e3:.1f} ms, difference {(best['lora'] - best['plain']) * 1e3:+.1f} ms "
                 f"({(best['lora'] - best['plain']) / len(entries) * 1e3:.3f} ms per adapted tensor)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
