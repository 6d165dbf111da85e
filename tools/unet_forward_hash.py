"""sha256 of one seeded SDXL-base UNet forward (CFG pair, 128x128 latent, synthetic weights) per dtype name: two builds agree bit for bit iff the lines agree
    [SDXL_LIB_PATH=<other build>] python tools/unet_forward_hash.py F16 F32_SPLIT"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as ge
pkg = ge.load_package()
ctx = pkg.Context(0)
cfg = pkg.sdxl_base_config()
rnd = lambda seed, *shape: torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()
x, c, y = rnd(50, 2, 4, 128, 128), rnd(51, 2, 77, cfg.context_dim), rnd(52, 2, cfg.adm_in_channels)
t = torch.tensor([999, 333], dtype=torch.int32).cuda()
for name in sys.argv[1:]:
    u = pkg.UNet(ctx, cfg, getattr(pkg, "DTYPE_" + name), seed=0)
    out = u.forward(x, t, c, y).cpu()
    print(f"unet forward {name}: sha256 {hashlib.sha256(out.numpy().tobytes()).hexdigest()} finite={bool(torch.isfinite(out).all())}", flush=True)
    del u
