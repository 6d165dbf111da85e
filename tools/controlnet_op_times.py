"""The two per-step additions of a controlled SDXL step on their own (profiles/controlnet_op_times.txt), at the shapes of the base model on a
128 x 128 latent with B = 2 in f16:

    --add N      N launches of the one-launch skip-residual add (sdxl_skip_residual_add) over the ten segments a UNet's table has there: the skip
                 halves of the concat buffers (column slices, row pitch = the concat width) and the middle block's output.  Run it under
                 rocprofv3 --kernel-trace --stats and read the row of skip_add_kernel<_Float16, 1, false>: the entry itself allocates and synchronises.
    --convs      the ten 1x1 convolutions of a control net, shape by shape through sdxl_bench_igemm (event-timed mean of 20 launches each, in
                 isolation: no graph, no neighbours in the cache -- not the cost inside a step)
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
    ap.add_argument("--convs", action="store_true")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    cfg = pkg.sdxl_base_config()
    shapes = pkg.unet_skip_shapes(cfg, 128, 128)
    B = 2
    if args.add:
        # a skip tensor of C channels is the upper part of a concat buffer whose lower part is the decoder's running tensor: widths of the
        # base model's output entries, in skip_shapes order (the middle block's output is the lower 1280 of the first concat buffer)
        concat = [640, 640, 960, 960, 1280, 1920, 1920, 2560, 2560, 2560]
        segs, nbytes = [], 0
        for (c, h, w), ld in zip(shapes, concat):
            buf = torch.randn(B * h * w, ld, device="cuda").half()
            src = torch.randn(B * h * w, c, device="cuda").half()
            last = len(segs) == len(shapes) - 1
            segs.append((buf[:, :c] if last else buf[:, ld - c:], src))
            nbytes += 3 * src.numel() * 2
        scale = torch.tensor([0.5], device="cuda")
        for _ in range(args.add):
            pkg.skip_residual_add(ctx, segs, scale)
        torch.cuda.synchronize()
        print(json.dumps({"add_launches": args.add, "segments": len(segs), "bytes_moved_per_launch": nbytes}), flush=True)
    if args.convs:
        total = 0.0
        for c, h, w in shapes:
            ms = pkg.bench_igemm(ctx, B, h, w, c, c, 1)
            total += ms
            print(json.dumps({"conv1x1": [B, h, w, c, c], "ms": round(ms, 4)}), flush=True)
        print(json.dumps({"conv1x1_total_ms_isolated": round(total, 4)}), flush=True)


if __name__ == "__main__":
    main()
