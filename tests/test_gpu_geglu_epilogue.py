"""The 256x320 GEGLU kernel (tile 26, igemm_wide_kernel) at the smallest shapes where its tail can go wrong: its LDS-staged instantiation, and
the direct one (column vectors parked in LDS at kernel entry, registers -> 16-byte stores) against it.

Two routes reach the kernel:
  * the op entries pkg.linear / pkg.layer_norm_linear with geglu=True (tile 26 forced through the igemm_variant hook).  They store fp32, so these
    launches run the STAGED instantiation whatever the knob says; what they cover of this kernel is the prologue, the k-loop below / at / above
    the ring depth and the staged tail on whole and ragged row tiles, each against fp64 within the bar of test_gpu_f16_kernels.gemm_bar
    (U = 1e-5 max|ref| through util.geglu, plus gelu_erf2's own error -- no new tolerance), and bit for bit against igemm_epilogue_staged = 1.
  * one transformer entry of a UNet's block plan in f16 mode (UNet.run_block): there the GEGLU projection stores f16 without residual, which is the
    case launch_wide gives the direct instantiation.  M = 512 is two whole row tiles; M = 320 leaves the second one ragged: its rows past M are
    computed on zero-page operands and must not be stored.  The block's output must be bit for bit the one with igemm_epilogue_staged = 1 (the
    staged instantiation): the direct epilogue applies the staged one's operations in its order.
"""
import math

import pytest
import torch

from oracle import config as OC
from test_gpu_f16_kernels import fold_ref, gemm_bar, rnd
from util import f16v, geglu, to_pkg_cfg

pytestmark = pytest.mark.gpu

U = 1e-5
TILE = 26


def forced(pkg, staged, fn):
    """fn() with tile 26 forced and the epilogue knob set; both restored"""
    pkg.debug_set("igemm_variant", TILE)
    pkg.debug_set("igemm_epilogue_staged", 1 if staged else 0)
    try:
        return fn()
    finally:
        pkg.debug_set("igemm_epilogue_staged", 0)
        pkg.debug_set("igemm_variant", 0)


def within(tag, out, ref, tol):
    err = (out.double() - ref).abs()
    ratio = (err / tol).max().item()
    print(f"{tag}: max err {err.max().item():.3e}, worst element {ratio:.3f} x its bar")
    assert torch.isfinite(out).all(), f"{tag}: non-finite output"
    assert ratio <= 1.0, f"{tag}: worst element {ratio:.3f} x its bar"


def linear_operands(M, K, N, bias, seed=10):
    # linear_case's operands with the weights at 1.5 / sqrt(K): gate pre-activations ~ N(0, 1.5^2) reach |g| ~ 6 over a tile, both signs
    x = f16v(rnd(M, K, seed=seed))
    w = f16v(rnd(K, N, seed=seed + 1, scale=1.5 / math.sqrt(K)))
    b = 0.1 * rnd(N, seed=seed + 2) if bias else None
    return x, w, b


def linear_both(pkg, ctx, M, K, N, bias, seed=10):
    x, w, b = linear_operands(M, K, N, bias, seed)
    y = x.double() @ w.double() + (b.double() if bias else 0.0)
    ref, tol = gemm_bar(y, True)
    out = forced(pkg, False, lambda: pkg.linear(ctx, x, w, b, True, 1))
    staged = forced(pkg, True, lambda: pkg.linear(ctx, x, w, b, True, 1))
    return out, staged, ref, tol, y[:, N // 2:].abs().max().item()


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("K", [64, 96, 160])         # 2, 3 and 5 k-tiles: below, at and above the ring depth
@pytest.mark.parametrize("N", [640, 960])            # two and three column tiles
@pytest.mark.parametrize("M", [256, 512, 320])       # one tile, two tiles, a ragged second tile
def test_geglu_linear(pkg, ctx, M, N, K, bias):
    out, staged, ref, tol, gmax = linear_both(pkg, ctx, M, K, N, bias)
    tag = f"geglu tile 26 linear M={M} N={N} K={K} bias={bias} (max|g| {gmax:.2f})"
    within(tag, out, ref, tol)
    assert torch.equal(out, staged), f"{tag}: differs from the staged epilogue by {(out - staged).abs().max().item():.3e}"


@pytest.mark.parametrize("large_mean", [False, True])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("K", [64, 192])             # the folded LayerNorm takes K % 64 == 0: 2 and 6 k-tiles, 1 and 3 statistics slots
@pytest.mark.parametrize("N", [640, 960])
@pytest.mark.parametrize("M", [256, 512, 320])
def test_geglu_layer_norm_linear(pkg, ctx, M, N, K, bias, large_mean):
    eps = 1e-5
    x = rnd(M, K, seed=30, scale=2.0, shift=0.3)
    if large_mean:       # the row set of test_layer_norm_linear_folded: every 4th row |mu| = 20 sigma, row 1 at 100 sigma
        x[::4] = rnd(M, K, seed=31, scale=0.5)[::4] + 10.0 * torch.sign(rnd(M, 1, seed=32)[::4])
        x[1] = rnd(K, seed=33, scale=0.05) - 5.0
    x16 = f16v(x)
    gamma, beta = 1 + 0.1 * rnd(K, seed=34), 0.1 * rnd(K, seed=35)
    w = rnd(K, N, seed=36, scale=1.5 / math.sqrt(K))
    b = 0.1 * rnd(N, seed=37) if bias else None
    run = lambda: pkg.layer_norm_linear(ctx, x16, gamma, beta, w, b, eps, True, 1)      # noqa: E731
    out, staged = forced(pkg, False, run), forced(pkg, True, run)
    y, canc = fold_ref(x16, gamma, beta, w, b, eps)
    ref, slack = geglu(y, U * y.abs().max() + canc)
    n = N // 2
    tol = U * ref.abs().max() + slack + y[:, :n].abs() * (0.75e-7 * y[:, n:].abs() + 2e-6 * torch.nn.functional.gelu(y[:, n:]).abs())
    tag = f"geglu tile 26 layer_norm_linear M={M} N={N} K={K} bias={bias} large_mean={large_mean} (max|g| {y[:, n:].abs().max().item():.2f})"
    within(tag, out, ref, tol)
    assert torch.equal(out, staged), f"{tag}: differs from the staged epilogue by {(out - staged).abs().max().item():.3e}"


def test_geglu_back_to_back_widths(pkg, ctx):
    # two launches of different N (and bias / no bias) back to back, then the first again: a column vector left in LDS by the previous
    # launch, or by the previous workgroup on the same CU, would show
    first = linear_both(pkg, ctx, 512, 160, 960, True, seed=50)
    second = linear_both(pkg, ctx, 512, 160, 640, False, seed=60)
    again = linear_both(pkg, ctx, 512, 160, 960, True, seed=50)
    for tag, (out, staged, ref, tol, _) in (("N=960 bias", first), ("N=640 no bias", second), ("N=960 bias again", again)):
        within(f"geglu tile 26 back to back {tag}", out, ref, tol)
        assert torch.equal(out, staged), tag
    assert torch.equal(first[0], again[0])


# ---- the f16-stored GEGLU of a UNet transformer entry: the direct epilogue

BLOCK_CFG = OC.UNetConfig(128, 320, [1, 2, 4], 64, [0, 1, 1], 128)      # level 1: C = 640, 10 heads, GEGLU N = 5120 (16 column tiles), K = 640
BLOCK = ("input", 4)                                               # 320 -> 640 ResBlock + one transformer block


@pytest.fixture(scope="module")
def block_unet(pkg, ctx):
    return pkg.UNet(ctx, to_pkg_cfg(pkg, BLOCK_CFG), pkg.DTYPE_F16, seed=0)


@pytest.mark.parametrize("B,h,w", [(2, 16, 16), (1, 16, 20)])     # M = 512: two whole row tiles; M = 320: the second one ragged
def test_geglu_direct_matches_staged_in_a_unet_block(pkg, ctx, block_unet, B, h, w):
    x = rnd(B, 320, h, w, seed=70)
    emb = 0.5 * rnd(B, 4 * BLOCK_CFG.model_channels, seed=71)
    context = rnd(B, 77, BLOCK_CFG.context_dim, seed=72)
    run = lambda: block_unet.run_block(BLOCK[0], BLOCK[1], x, emb, context)      # noqa: E731
    direct, staged = forced(pkg, False, run), forced(pkg, True, run)
    assert torch.isfinite(direct).all() and direct.abs().max().item() > 0
    assert torch.equal(direct, staged), f"B={B} {h}x{w}: direct and staged GEGLU epilogues differ by {(direct - staged).abs().max().item():.3e}"
    # the next level's entry in between (C = 1280: GEGLU N = 10240, K = 1280, M = 128 / 80 -- one ragged row tile, other bias and ln_cs vectors):
    # a vector corner left over from another launch would show in either
    x2 = rnd(B, 640, h // 2, w // 2, seed=73)
    run2 = lambda: block_unet.run_block("input", 7, x2, emb, context)      # noqa: E731
    direct2, staged2 = forced(pkg, False, run2), forced(pkg, True, run2)
    assert torch.isfinite(direct2).all() and torch.equal(direct2, staged2), f"B={B} {h // 2}x{w // 2}: the 1280-wide entry differs"
    assert torch.equal(direct, forced(pkg, False, run)), "the replay differs"
