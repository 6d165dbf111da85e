"""Record-only cases for tools/ops_ab_record.py that the op tests do not call on every path: null bias in f16 and F32_SPLIT, GEGLU in both, the four fused values, the generic f16 attention kernel"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.Context(0)


def arb(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
@pytest.mark.parametrize("geglu", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M,K,N", [(256, 320, 1280), (77, 128, 192), (300, 640, 5120)])
def test_linear_forms(pkg, ctx, dtype, geglu, bias, M, K, N):
    x, w = arb(1, M, K), arb(2, K, N) / K ** 0.5
    b = arb(3, N).cuda() if bias else None
    try:
        pkg.linear(ctx, x.cuda(), w.cuda(), b, geglu, dtype)
    except Exception:      # recorded by the plugin: both libraries must refuse alike
        pass


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("B,Cin,H,W,Cout,k,stride,pad,up", [(2, 64, 16, 16, 128, 3, 1, 1, False), (1, 320, 8, 8, 640, 1, 1, 0, False),
                                                            (1, 32, 8, 8, 64, 3, 2, 1, False), (1, 64, 8, 8, 64, 3, 1, 1, True)])
def test_conv_forms(pkg, ctx, dtype, bias, B, Cin, H, W, Cout, k, stride, pad, up):
    x, w = arb(4, B, Cin, H, W), arb(5, Cout, Cin, k, k) / (Cin * k * k) ** 0.5
    b = arb(6, Cout).cuda() if bias else None
    try:
        pkg.conv2d(ctx, x.cuda(), w.cuda(), b, stride, pad, up, dtype)
    except Exception:      # recorded by the plugin: both libraries must refuse alike
        pass


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1, 2, 3])
@pytest.mark.parametrize("B,Nq,Nk,C", [(2, 1024, 77, 1280), (1, 128, 96, 64), (2, 256, 33, 640)])
def test_ln_query_fused_values(pkg, ctx, fused, B, Nq, Nk, C):
    x, g, bt = arb(7, B, Nq, C), 1 + 0.1 * arb(8, C), 0.1 * arb(9, C)
    wq, k, v = arb(10, C, C) / C ** 0.5, arb(11, B, Nk, C), arb(12, B, Nk, C)
    try:
        pkg.ln_query_cross_attention(ctx, x.cuda(), g.cuda(), bt.cuda(), wq.cuda(), k.cuda(), v.cuda(), 1e-5, fused)
    except Exception:      # recorded by the plugin: both libraries must refuse alike
        pass


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nq,Nk,heads", [(2, 300, 77, 10), (1, 320, 320, 1)])
def test_attention_generic_f16(pkg, ctx, B, Nq, Nk, heads):
    # attn_variant -1 in f16: attn_d64_kernel<_Float16>, which no op test forces
    q, k, v = arb(19, B, Nq, 64 * heads), arb(20, B, Nk, 64 * heads), arb(21, B, Nk, 64 * heads)
    pkg.debug_set("attn_variant", -1)
    try:
        pkg.qkv_attention(ctx, q.cuda(), k.cuda(), v.cuda(), None, heads, 1)
    finally:
        pkg.debug_set("attn_variant", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("fused", [False, True])
def test_conv_group_norm_forms(pkg, ctx, res, fused):
    B, Cin, H, W, Cout = 2, 320, 16, 16, 640
    x, w, b = arb(13, B, Cin, H, W), arb(14, Cout, Cin, 3, 3) / (Cin * 9) ** 0.5, arb(15, Cout)
    g, bt = 1 + 0.1 * arb(16, Cout), 0.1 * arb(17, Cout)
    r = arb(18, B, Cout, H, W).cuda() if res else None
    try:
        pkg.conv2d_group_norm(ctx, x.cuda(), w.cuda(), b.cuda(), g.cuda(), bt.cuda(), 1e-5, 32, True, r, fused)
    except Exception:      # recorded by the plugin: both libraries must refuse alike
        pass
