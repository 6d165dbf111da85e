"""two 4-step CFG trajectories of the f16 base UNet at 1024^2 (graph replay) for a kernel trace"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as ge
pkg = ge.load_package(); ctx = pkg.Context(0)
d = pkg.Diffuser(ctx, pkg.sdxl_base_config(), pkg.DTYPE_F16, seed=0)
g = torch.Generator(device="cuda").manual_seed(0)
r = lambda *s: torch.randn(*s, device="cuda", generator=g)
cond = pkg.Conditioning(context_full=r(1, 77, 2048), channel_context=r(1, 2816), unconditional_context_full=r(77, 2048),
                        unconditional_channel_context=r(2816), resolution=(1024, 1024))
noise = r(1, 4, 128, 128)
for it in range(2):
    lat = d.sample_latent(cond, 7.5, 4, noise)
torch.cuda.synchronize()
print("ok", bool(torch.isfinite(lat).all()))
