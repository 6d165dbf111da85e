"""The per-step add of several control nets on its own (profiles/controlnet_trajectory_times.txt), at the base model's shapes on a
128 x 128 latent, B = 2, f16:

    --add N      N launches each of the per-step add with one and with two sources (sdxl_skip_residual_add_steps_multi) and of the one-source
                 entry (sdxl_skip_residual_add_steps) over the ten segments a UNet's table has there.  Run it under
                 rocprofv3 --kernel-trace --stats and read the rows of skip_add_kernel<_Float16, 1, true> (2 N launches: both one-source entries
                 run it) and skip_add_kernel<_Float16, 2, true>: the entries themselves allocate and synchronise.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--add", type=int, default=0)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    cfg = pkg.sdxl_base_config()
    if args.add:
        shapes = pkg.unet_skip_shapes(cfg, 128, 128)
        B = 2
        concat = [640, 640, 960, 960, 1280, 1920, 1920, 2560, 2560, 2560]      # (tools/controlnet_op_times.py: the concat widths in skip_shapes order)
        segs1, segs2 = [], []
        for (c, h, w), ld in zip(shapes, concat):
            buf = torch.randn(B * h * w, ld, device="cuda").half()
            s1, s2 = (torch.randn(B * h * w, c, device="cuda").half() for _ in range(2))
            dst = buf[:, :c] if len(segs1) == len(shapes) - 1 else buf[:, ld - c:]
            segs1.append((dst, [s1]))
            segs2.append((dst, [s1, s2]))
        one = torch.full((2, 1, 8), 0.5, device="cuda")
        two = torch.full((2, 2, 8), 0.5, device="cuda")
        for _ in range(args.add):
            pkg.skip_residual_add_steps(ctx, [(dst, s[0]) for dst, s in segs1], B, one.view(2, 8), 0)
            pkg.skip_residual_add_steps_multi(ctx, segs1, B, one, 0)
            pkg.skip_residual_add_steps_multi(ctx, segs2, B, two, 0)
        torch.cuda.synchronize()
        print(json.dumps({"add_launches_each": args.add, "segments": len(segs1)}), flush=True)


if __name__ == "__main__":
    main()
