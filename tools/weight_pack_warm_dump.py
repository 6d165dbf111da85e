"""The weight-warming schedule of the SDXL base UNet as text, and the time a full-size Diffuser takes to create: what a change of the weight
arena's allocation order would move (run_conv extends a launch's cold region over the arena neighbours of its weight, csrc/weights.cpp).

    [SDXL_LIB_PATH=<other build>] timeout -k 10 300 python tools/weight_pack_warm_dump.py --out profiles/<name>.txt

A fresh child process (SDXL_WARM_DUMP=1, stderr captured) creates the f16 base Diffuser on synthetic seed 0 and runs one eager forward, B = 2,
128 x 128 latent, 77 context tokens; the `[warm]` lines of its stderr go to --out, the create time is printed.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child():
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    cfg = pkg.sdxl_base_config()
    t0 = time.perf_counter()
    d = pkg.Diffuser(ctx, cfg, pkg.DTYPE_F16, seed=0)
    ctx.synchronize()
    print(f"create_s {time.perf_counter() - t0:.3f} weight_bytes {d.diffusion.weight_arena()[1]}")
    u = d.diffusion
    u.set_graph(False)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 128, 128, generator=g).cuda()
    out = u.forward(x, torch.tensor([999, 500], dtype=torch.int32).cuda(), torch.randn(2, 77, cfg.context_dim, generator=g).cuda(),
                    torch.randn(2, cfg.adm_in_channels, generator=g).cuda())
    assert torch.isfinite(out).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--out", "-"], env=dict(os.environ, SDXL_WARM_DUMP="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=280)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        sys.exit(r.returncode)
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[warm]")]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(r.stdout.strip(), f"-> {len(lines)} [warm] lines in {args.out}")


if __name__ == "__main__":
    main()
