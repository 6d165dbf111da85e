"""Nearest-2x upsample + 3x3 convolution on the folded phase weights (csrc/upsample_fold.h, IgemmParams::ph_rows) against fp64.

What the folded launch computes: out = sum_k x_k P(Wf_k) in fp32, Wf = the fp32 phase sums of the 3x3 taps (tests/upsample_fold_ref.py, bit for bit
the library's: test_cpu_upsample_fold.py), P = the engine's packing -- one f16 rounding in the f16 engine, a (hi, lo) f16 pair (22 bits) in the
split-operand one.

Bars
  * f16 engine against fp64 phase convolutions of the SAME rounded weights f16(Wf), exact-f16 inputs: U max|ref|, U = 1e-5 -- the bar of
    test_gpu_f16_kernels.py for fp32-stored GEMM outputs on exact f16 operands.
  * split-operand engine against fp64 of the fp32 Wf: 2e-6 max|ref|, the bar and the input recipe of test_gpu_ops.py::test_conv2d_split_operand.
  * folded against fp64 of the ORIGINAL 3x3 weights (what the model computes): the extra term is the weight rounding delta_k = f16(Wf_k) - Wf_k,
    |delta_k| <= u |Wf_k|, u = 2^-11:  |sum_k x_k delta_k| <= min(u sum_k |x_k Wf_k|, 8 u sqrt(sum_k x_k^2 Wf_k^2))  -- the worst case, and
    Hoeffding's bound for zero-mean roundings in [-u |Wf_k|, u |Wf_k|] (P <= 2 e^-32 per element, as the attention bars of test_gpu_f16_kernels.py)
    -- plus U max|ref| for the fp32 accumulation.  K = 4 Cin terms per element, evaluated per element from the data.
"""
import math

import numpy as np
import pytest
import torch

import upsample_fold_ref as UF
from oracle import config as OC, model as OM, pipeline as OP
from util import f16v, rel_err, seeded, to_pkg_cfg, to_pkg_vcfg, unet_weights

pytestmark = pytest.mark.gpu

U = 1e-5                 # test_gpu_f16_kernels.py: fp32-stored GEMM output on exact f16 operands, relative to max|ref|
UH = 2.0 ** -11          # f16 unit roundoff
SPLIT = 2e-6             # test_gpu_ops.py::test_conv2d_split_operand
F16, HL = 1, 3           # SDXL_DTYPE_F16, SDXL_DTYPE_F32_SPLIT

SHAPES = [  # B, Cin, H, W, Cout, folded
    (2, 64, 8, 16, 128, True),       # one 256-row tile per phase
    (1, 128, 16, 48, 160, True),     # three tiles per phase, H != W, the 160-wide tiles
    (1, 128, 16, 48, 320, True),
    (1, 64, 9, 9, 128, False),       # 81 rows per phase: no tile multiple -> gather form on the 3x3 weights
]


def operands(dtype, B, Cin, H, W, Cout):
    if dtype == F16:      # exact f16 inputs and parameters (test_gpu_f16_kernels.py conv_case)
        x = f16v(seeded(B, Cin, H, W, seed=20))
        w = f16v(seeded(Cout, Cin, 3, 3, seed=21) / math.sqrt(Cin * 9))
        b = 0.1 * seeded(Cout, seed=22)
    else:                 # inputs over five decades, small fp32 weights (test_gpu_ops.py test_conv2d_split_operand)
        g = torch.Generator().manual_seed(16)
        x = seeded(B, Cin, H, W, seed=13) * torch.pow(10.0, torch.rand(B, Cin, 1, 1, generator=g) * 5.0 - 4.0)
        w = 0.02 * seeded(Cout, Cin, 3, 3, seed=14) / math.sqrt(Cin * 9)
        b = 0.01 * seeded(Cout, seed=15)
    return x, w, b


def packed_fold(dtype, w):
    """the folded weights as the engine multiplies them, fp64: f16(fp32 sums) in the f16 engine, the fp32 sums (carried as 22-bit pairs) in the split one"""
    wf = UF.fold(w.numpy(), np.float32)
    return (wf.astype(np.float16) if dtype == F16 else wf).astype(np.float64)


def run(pkg, ctx, dtype, x, w, b):
    out, folded = pkg.conv2d_upsample_folded(ctx, x.cuda(), w.cuda(), b.cuda(), dtype)
    return out.cpu().double().numpy(), folded


@pytest.mark.parametrize("dtype", [F16, HL])
@pytest.mark.parametrize("B,Cin,H,W,Cout,folded", SHAPES)
def test_folded_conv_against_fp64_phase_convs(pkg, ctx, dtype, B, Cin, H, W, Cout, folded):
    x, w, b = operands(dtype, B, Cin, H, W, Cout)
    out, took = run(pkg, ctx, dtype, x, w, b)
    assert took == folded
    ref = UF.conv_phases(x.numpy(), packed_fold(dtype, w), b.numpy()) if folded else UF.conv_upsampled(x.numpy(), w.numpy(), b.numpy())
    assert out.shape == ref.shape == (B, Cout, 2 * H, 2 * W)
    e = np.abs(out - ref).max() / np.abs(ref).max()
    bar = U if dtype == F16 else SPLIT
    print(f"upsample fold dtype={dtype} {(B, Cin, H, W, Cout)} folded={took}: max err {e:.3e} max|ref| (bar {bar:.0e})")
    assert np.isfinite(out).all() and e <= bar


@pytest.mark.parametrize("dtype", [F16, HL])
def test_entry_alone_equals_entry_in_the_pair(pkg, ctx, dtype):
    """B = 2 (one 256-row tile per phase) against each entry alone (128 rows per phase): the same bits"""
    B, Cin, H, W, Cout, _ = SHAPES[0]
    x, w, b = operands(dtype, B, Cin, H, W, Cout)
    pair, took = pkg.conv2d_upsample_folded(ctx, x.cuda(), w.cuda(), b.cuda(), dtype)
    assert took
    for e in range(B):
        alone, took1 = pkg.conv2d_upsample_folded(ctx, x[e:e + 1].cuda(), w.cuda(), b.cuda(), dtype)
        assert took1 and torch.equal(alone[0], pair[e]), e


@pytest.mark.parametrize("dtype", [F16, HL])
def test_knob_on_and_off_against_the_original_weights(pkg, ctx, dtype):
    """the same layer folded and unfolded, both against fp64 of the 3x3 weights; the folded error inside the weight-rounding bar (module docstring)"""
    B, Cin, H, W, Cout, _ = SHAPES[1]
    x, w, b = operands(dtype, B, Cin, H, W, Cout)
    on, took_on = run(pkg, ctx, dtype, x, w, b)
    pkg.debug_set("upsample_fold", 0)
    try:
        off, took_off = run(pkg, ctx, dtype, x, w, b)
    finally:
        pkg.debug_set("upsample_fold", 1)
    assert took_on and not took_off
    ref = UF.conv_upsampled(x.numpy(), w.numpy(), b.numpy())
    mref = np.abs(ref).max()
    e_on, e_off = np.abs(on - ref), np.abs(off - ref)
    if dtype == F16:
        wf = UF.fold(w.numpy(), np.float64)
        worst = UH * UF.conv_phases(np.abs(x.numpy()), np.abs(wf))
        likely = 8 * UH * np.sqrt(UF.conv_phases(x.numpy().astype(np.float64) ** 2, wf ** 2))
        bar_on = np.minimum(worst, likely) + U * mref
        bar_off = np.full_like(ref, U * mref)
    else:
        bar_on = bar_off = np.full_like(ref, SPLIT * mref)
    print(f"upsample fold knob dtype={dtype} K={4 * Cin}: folded {e_on.max() / mref:.3e}, unfolded {e_off.max() / mref:.3e} max|ref| "
          f"(ratio {e_on.max() / max(e_off.max(), 1e-300):.1f}); folded worst element {(e_on / bar_on).max():.3f} x its bar, bar median {np.median(bar_on) / mref:.2e} max|ref|")
    assert (e_off <= bar_off).all()
    assert (e_on <= bar_on).all()


def test_decoder_folded_and_unfolded_against_the_oracle(pkg, ctx):
    """split-operand tiny decoder on a 16x16 latent: every upsampler (256, 1024, 4096 source pixels) runs folded; bound of test_gpu_models.py"""
    v = OC.tiny_vae_config()
    Wd = OM.to_torch(OC.synth_weights(OC.vae_decoder_param_specs(v)))
    latent = seeded(1, 4, 16, 16, seed=50) * 0.5
    ref = OP.LatentDecoder(v, Wd).decode_latent(latent)
    ld = pkg.LatentDecoder(ctx, to_pkg_vcfg(pkg, v), HL, seed=0)
    on = ld.decode_latent(latent.cuda()).cpu()
    pkg.debug_set("upsample_fold", 0)
    try:
        off = ld.decode_latent(latent.cuda()).cpu()
    finally:
        pkg.debug_set("upsample_fold", 1)
    e_on, e_off = rel_err(on, ref), rel_err(off, ref)
    print(f"vae decode 16x16 split-operand: folded {e_on:.3e}, unfolded {e_off:.3e}")
    assert not torch.equal(on, off), "the knob changed nothing: the folded form did not run"
    assert e_on < 5e-6 and e_off < 5e-6


def test_unet_folded_and_unfolded_against_the_oracle(pkg, ctx):
    """f16 tiny UNet on a 64x64 latent: both upsample levels (256 and 1024 source pixels per entry) run folded; bound of test_gpu_models.py"""
    ocfg = OC.tiny_config()
    W = unet_weights(ocfg)
    B, H = 2, 64
    x = torch.from_numpy(OC.arb_tensor(B, 4, H, H))
    context = torch.from_numpy(OC.arb_tensor(B, 5, ocfg.context_dim))
    y = torch.from_numpy(OC.arb_tensor(B, ocfg.adm_in_channels))
    t = torch.tensor([999, 1], dtype=torch.int32)
    ref = OM.unet_forward(ocfg, W, x, t.long(), context, y)
    outs = {}
    for knob in (1, 0):
        pkg.debug_set("upsample_fold", knob)
        try:
            u = pkg.UNet(ctx, to_pkg_cfg(pkg, ocfg), F16, seed=0)
            runs = [u.forward(x.cuda(), t.cuda(), context.cuda(), y.cuda()).cpu() for _ in range(3)]      # eager, capture, replay
        finally:
            pkg.debug_set("upsample_fold", 1)
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[1], runs[2]), "hipGraph replay differs from the eager run"
        outs[knob] = runs[0]
    e_on, e_off = rel_err(outs[1], ref), rel_err(outs[0], ref)
    print(f"unet forward 64x64 f16: folded {e_on:.3e}, unfolded {e_off:.3e}")
    assert not torch.equal(outs[1], outs[0]), "the knob changed nothing: the folded form did not run"
    assert e_on < 4.5e-3 and e_off < 4.5e-3
