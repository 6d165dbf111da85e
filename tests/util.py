"""shared helpers of the parity tests"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import config as OC, model as OM


def rel_err(out: torch.Tensor, ref: torch.Tensor) -> float:
    out, ref = out.detach().float().cpu(), ref.detach().float().cpu()
    return ((out - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def max_abs(out, ref) -> float:
    return (out.detach().float().cpu() - ref.detach().float().cpu()).abs().max().item()


def seeded(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def to_pkg_cfg(pkg, ocfg):
    return pkg.UNetConfig(ocfg.adm_in_channels, ocfg.model_channels, list(ocfg.channel_mults), ocfg.n_head_channels,
                          list(ocfg.transformer_depths), ocfg.context_dim, ocfg.in_channels, ocfg.out_channels,
                          ocfg.is_refiner)


def to_pkg_vcfg(pkg, v):
    return pkg.VAEConfig(list(v.enc_channels), list(v.dec_channels), v.n_group, v.enc_out_channels, v.scale_factor)


def unet_weights(ocfg, seed=0):
    return OM.to_torch(OC.synth_weights(OC.unet_param_specs(ocfg), seed))


def f16v(x):
    return x.half().float()


def ulp16(v):
    """spacing of the f16 numbers at |v| (subnormals: 2^-24)"""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))) - 10.0)


def rounding_slack(x, d):
    """(f16(x) as fp64, per element: one f16 spacing where x lies within d of a rounding midpoint -- the kernel rounds an fp32 value that
    may sit on the other side -- else 0)"""
    h = x.half().double()
    gap = (x - h).abs()
    u1, u2 = ulp16(x), ulp16(h)
    near = ((gap - u1 / 2).abs() <= d) | ((gap - u2 / 2).abs() <= d)
    return h, torch.where(near, torch.maximum(u1, u2), torch.zeros_like(x))


def geglu(y, dy=None):
    """GEGLU (unet/mod.rs:942-956: value half * gelu(gate half)) in fp64; with dy: + the propagated per-element bound"""
    n = y.shape[1] // 2
    v, g = y[:, :n], y[:, n:]
    out = v * F.gelu(g)
    if dy is None:
        return out, None
    dv, dg = dy[:, :n], dy[:, n:]
    return out, F.gelu(g).abs() * dv + (v.abs() + dv) * 1.13 * dg
