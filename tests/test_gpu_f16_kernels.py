"""The f16 kernels (SDXL_DTYPE_F16 and the generic kernel of SDXL_DTYPE_F16_F32RES) against fp64, op by op, at SDXL's own shapes.

Every case drives an op entry (linear, conv2d, layer_norm_linear, conv2d_group_norm, group_norm, layer_norm, qkv_attention,
ln_query_cross_attention).  The reference is plain torch fp64 on the operands the kernel sees: inputs the entry rounds to f16 are
rounded on the host first (x.half()), so that conversion is exact; the conversions themselves are tested bit for bit.  Every further
rounding the kernels perform is emulated or bounded per element (DESIGN 5.1 lists them with the measured errors):

  * f16 operands on entry: copy_rows / nchw_to_nhwc (csrc/elementwise.hip:20-25 st_f) at dtype 1; the generic kernel's A load
    (csrc/igemm.hip:53-65 load_chunk, :161 the gather) at dtype 2; the packed weights (elementwise.hip:636-649 pack_linear_kernel,
    pack_conv_kernel).  All are round-to-nearest-even: test_*_conversion_* check them bit for bit.
  * WeightBuilder::pack, LN_FOLD (csrc/weights.cpp): W' = f16(fp32(gamma_k W_kn)) (pack_linear_kernel with kscale), cs_n = sum_k W'_kn in fp32
    over the packed values (colsum_packed_kernel), b'_n = sum_k beta_k W_kn + b_n in fp32 from the unrounded W (beta_dot_kernel); the
    epilogue forms rstd (x W') - rstd mu cs + b' (igemm_common.h:211-219) with (mu, rstd) of the f16 rows (the identity GEMM's stat_out).
    Emulated exactly in fp64 (W' bit-exact on the host).
  * GELU: gelu_erf2 (igemm_common.h:65-74), A&S 7.1.26, |d erf| <= 1.5e-7 -> |d gelu(g)| <= 0.75e-7 |g|.
  * f16-stored outputs: the norm outputs (norm.hip), the conv output h of conv2d_group_norm (capi_ops.hip sdxl_conv2d_group_norm: Act h, igemm_common.h:510-520),
    attention O (attention.hip:674, :1186, :1608), the projected q of the unfused cross-attention (capi_ops.hip sdxl_ln_query_cross_attention: qd).
  * the GroupNorm statistics of conv2d_group_norm: the fused path takes them from the STORED f16 values (igemm_common.h:506-509, rr =
    (float)(half_t)v), the statistics pass reads the stored f16 h: both describe the same data, so both paths share one bar.
  * Q pre-scale: (half_t)((float)q * sc), sc = fp32(scale * log2 e) (attention.hip:506-517 and its siblings): emulated BIT-EXACTLY on the
    host (one fp32 multiply, one RNE conversion).  Fused cross-attention: f16(q_fp32 * sc) straight from the projection's accumulators
    (igemm_common.h:1011): rounding_slack around the fp64 q.
  * P = exp2(S - m) rounded to f16 before the PV MFMA (attention.hip:641-643, igemm_common.h:1038-1040), l summed from the UNROUNDED
    fp32 P, under a deferred running max m <= max S (P <= 2^THR): not emulable (m is the kernel's), bounded per element, below.
  * key-split / key-half merges (attention.hip:1151-1176, attn_xhalf_merge): fp32, inside the fp32-class term.

Bars (derivations; each test prints its worst element as a multiple of its bar and the old op test's bar over the new one):
  * fp32-stored GEMM outputs on exact f16 operands: U = 1e-5 max|ref| (fp32 accumulation, room for K up to 17 280).  GEGLU: the fp32
    bar on both halves propagated through v gelu(g) (util.geglu, |gelu'| <= 1.13) + |v| (0.75e-7 |g| + 2e-6 |gelu g|) for gelu_erf2.
  * folded LayerNorm: the same, plus the fold's cancellation: rstd (x W') and rstd mu cs are both ~ rstd |mu| |cs| and cancel.  Each is
    an fp32 sum of K terms whose roundings (<= 2^-24 of a partial sum ~ |mu| sqrt(k) rms(W')) add as a random walk: sigma ~
    0.58 * 2^-24 * K |mu| rms_k(W'_kn) per sum, 0.82 for the two; 4 sigma with partial sums up to twice their rms -> 8 * 2^-24 * K *
    rstd |mu| rms_k(W'_kn).  Measured: 0.1-0.2 of it on the 100-sigma row.
  * norms (f16 output): U max|ref| + 8 * 2^-24 (|mu| + sigma) rstd |gamma| (the fp32 mean carries a few ulp of |mu| into x - mu) +
    half an f16 spacing at the reference.  conv -> GroupNorm additionally: h = f16(conv) is rounding_slack-emulated (one spacing where
    the exact value sits within U of a midpoint), propagated through (h - mu) rstd gamma and SiLU (|silu'| <= 1.1).
  * attention (f16 O): with p_j = exp2(S_j - max S), l = sum p_j, u = 2^-11:
        |O - O_ref| <= min(u sum_j p_j |v_j|, 8 u sqrt(sum_j p_j^2 v_j^2)) / l + 2^-25 sum_{p_j < 2^-14} |v_j| / l
            (P's rounding, relative <= u on normal P -- the deferred max only scales P up by 2^(max S - m) >= 1, so P is normal wherever
             p_j >= 2^-14 -- absolute <= 2^-25 on subnormal P.  The first bound is the worst case; the second is Hoeffding's for
             independent zero-mean roundings delta_j in [-u, u]: P(|sum delta_j p_j v_j| >= 8 u sqrt(sum p_j^2 v_j^2)) <= 2 e^-32 = 2.5e-14
             per element, < 1e-5 over every element this module checks.  l is summed from the unrounded P, so only the numerator moves)
                      + ln 2 * 1.1 * sum_j p_j E_j (|v_j| + |O|) / l    (E_j = sum_d slack(q'_d) |k_jd|: q' rounding ambiguity)
                      + U max|ref| + half an f16 spacing at the reference.

The old bars (test_gpu_ops.py: 4e-3 GEMM/norm, 8e-3 GEGLU, 6e-3 attention, relative to max|ref|, with unrounded inputs and an fp32
oracle) sit 10x-400x above these.

Out of scope: the f16-store epilogues no op entry reaches (the f16 output of a plain linear / conv2d with a residual as the UNet runs
them, the QKV projection's transposed V^T store); the UNet-level tests cover them, and tests/test_gpu_clip_layer.py holds both to an fp64
reference at the CLIP encoders' real widths: the V^T store at 77 rows per entry (every row tile straddles batch entries) and the in-place residual
epilogue on an f16 and on an fp32 stream.

Dispatch (launch_attention_d64, attention.hip): base 64^2 (10 heads, 4096 queries) runs attn_d64_mix_kernel level 0 (4/5 of the heads in
128-query blocks, the rest key-split); base 32^2 (20 heads, 1024) level 2 (the last fifth as key halves merged across workgroups);
the refiner's 12 / 24 heads are not divisible by 5: 4096 queries run variant 2 (128-query blocks), 1024 and 256 queries the key-split body.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import model as OM
from util import f16v, geglu, rounding_slack, ulp16

pytestmark = pytest.mark.gpu

U = 1e-5                         # fp32-class bar, relative to max|ref|
UH = 2.0 ** -11                  # f16 unit roundoff
LOG2E = 1.4426950408889634
DEV = "cuda"


def rnd(*shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale + shift


def check(tag, out, ref, tol, old):
    """out within its per-element bar tol of the fp64 ref; prints error, bar and the old bar's factor over it"""
    out, ref = out.double(), ref.double()
    tol = torch.as_tensor(tol, dtype=torch.float64, device=ref.device).expand_as(ref)
    err = (out - ref).abs()
    mref = ref.abs().max().item()
    ratio = (err / tol).max().item()
    tmed, tmax = tol.median().item(), tol.max().item()
    print(f"{tag}: max err {err.max().item() / mref:.2e} max|ref|, worst element {ratio:.3f} x its bar; bar median {tmed / mref:.2e}, "
          f"max {tmax / mref:.2e} max|ref| (old bar {old:.0e}: {old * mref / tmed:.0f}x above the median bar, {old * mref / tmax:.0f}x above the max)")
    assert torch.isfinite(out).all(), f"{tag}: non-finite output"
    assert ratio <= 1.0, f"{tag}: worst element {ratio:.3f} x its bar"


def gemm_bar(y, geglu_=False):
    """(ref, per-element bar) of an fp32-stored GEMM output y (fp64, bias included) -- module docstring"""
    if not geglu_:
        return y, U * y.abs().max()
    ref, slack = geglu(y, torch.full_like(y, U * y.abs().max().item()))
    n = y.shape[1] // 2
    v, g = y[:, :n], y[:, n:]
    return ref, U * ref.abs().max() + slack + v.abs() * (0.75e-7 * g.abs() + 2e-6 * F.gelu(g).abs())


def with_variant(pkg, key, v, fn):
    pkg.debug_set(key, v)
    try:
        return fn()
    finally:
        pkg.debug_set(key, 1 if key == "attn_xsplit" else 0)


# ----------------------------------------------------------------------------------------------------------------- 1. conversions

def conversion_values():
    """fp32 values that probe RNE to f16: ties, near-ties, subnormals, the smallest normal, 65504 and the overflow threshold"""
    s = [1 + 2 ** -11, 1 + 3 * 2 ** -11, 1 + 2 ** -11 + 2 ** -23, 1 + 2 ** -11 - 2 ** -23, 2048 + 1, 2048 + 3, 0.1, 1 / 3, -1 - 2 ** -11,
         2 ** -24, 2 ** -25, 3 * 2 ** -25, 2 ** -25 + 2 ** -40, 1.5 * 2 ** -24, 5 * 2 ** -26, 2 ** -26, -3 * 2 ** -25, 2 ** -30,
         2 ** -14, 2 ** -14 - 2 ** -25, 2 ** -14 + 2 ** -25, 2 ** -14 - 2 ** -26, 65504.0, 65519.0, 65519.996, -65519.0, 65505.0,
         0.0, -0.0, 1.0, -2.5, 1000.3]
    return torch.tensor(s, dtype=torch.float32)


def conversion_matrix(rows, n, seed):
    v = conversion_values()
    x = rnd(rows, n, seed=seed).cpu() * torch.exp2(torch.randint(-20, 12, (rows, n), generator=torch.Generator().manual_seed(seed))).float()
    x.view(-1)[: v.numel()] = v
    x.view(-1)[v.numel(): 2 * v.numel()] = -v
    return x


def assert_f16_exact(tag, out, x):
    want = f16v(x)
    fin = torch.isfinite(want)
    assert torch.equal(out[fin], want[fin]), f"{tag}: {(out[fin] != want[fin]).sum().item()} elements are not RNE f16(x)"


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("M", [160, 2048])
def test_linear_conversion_activation_side_is_rne(pkg, ctx, dtype, M):
    # x @ I (fp32 output) = f16(x) bit for bit: dtype 1 converts in copy_rows, dtype 2 in the generic kernel's A load
    K = 128
    x = conversion_matrix(M, K, seed=1)
    out = pkg.linear(ctx, x.cuda(), torch.eye(K).cuda(), None, False, dtype).cpu()
    assert_f16_exact(f"linear x@I dtype={dtype} M={M}", out, x)
    print(f"linear x@I dtype={dtype} M={M}: bit-exact f16(x) on {x.numel()} values incl. ties, subnormals, 2^-14, 65504, 65519.996")


@pytest.mark.parametrize("dtype", [1, 2])
def test_linear_conversion_weight_side_is_rne(pkg, ctx, dtype):
    K, N = 128, 256
    w = conversion_matrix(K, N, seed=2)
    out = pkg.linear(ctx, torch.eye(K).cuda(), w.cuda(), None, False, dtype).cpu()
    assert_f16_exact(f"linear I@w dtype={dtype}", out, w)


@pytest.mark.parametrize("dtype", [1, 2])
def test_linear_conversion_overflow_and_non_finite(pkg, ctx, dtype):
    # an input that is not finite in f16 (65520 and above round to inf; inf; NaN) converts to f16(x) = +-inf / NaN: in x @ I its own
    # column comes out +-inf (inf x 1 plus finite x 0 terms; NaN stays NaN) and every other column of its row NaN (inf x 0).  The weight
    # side (I @ w) the same along the column.  Every other row / column stays bit-exact.
    K = 128
    x = conversion_matrix(64, K, seed=3)
    w = conversion_matrix(K, 64, seed=4)
    bad = {5: 65520.0, 9: -65520.0, 17: float("inf"), 23: float("-inf"), 31: float("nan"), 40: 1e6}
    for r, val in bad.items():
        x[r, (7 * r) % K] = val
        w[(7 * r) % K, r] = val
    out = pkg.linear(ctx, x.cuda(), torch.eye(K).cuda(), None, False, dtype).cpu()
    outw = pkg.linear(ctx, torch.eye(K).cuda(), w.cuda(), None, False, dtype).cpu()
    for o, lines in ((out, out), (outw, outw.t())):
        for r, val in bad.items():
            c = (7 * r) % K
            want = torch.tensor(val).half().float()
            assert torch.equal(lines[r, c], want) or (torch.isnan(want) and torch.isnan(lines[r, c])), f"{val}: {lines[r, c]}"
            assert torch.isnan(torch.cat([lines[r, :c], lines[r, c + 1:]])).all()
    keep = torch.ones(64, dtype=torch.bool)
    keep[torch.tensor(sorted(bad))] = False
    assert torch.equal(out[keep], f16v(x[keep])) and torch.equal(outw[:, keep], f16v(w[:, keep]))


@pytest.mark.parametrize("variant", [0, 6, 7, 8])
def test_attention_single_key_returns_f16_v(pkg, ctx, variant):
    # Nk = 1: P = 1, O = v exactly -- the V^T transpose / padding path and O's store, bit for bit
    B, Nq, C, heads = 2, 320, 640, 10
    q, k = rnd(B, Nq, C, seed=4), rnd(B, 1, C, seed=5)
    v = conversion_matrix(B, C, seed=6).clamp(-60000, 60000).reshape(B, 1, C)
    out = with_variant(pkg, "attn_variant", variant, lambda: pkg.qkv_attention(ctx, q, k, v.cuda(), None, heads, 1))
    want = f16v(v).expand(B, Nq, C).cuda()
    assert torch.equal(out, want)


# ----------------------------------------------------------------------------------------------------------------- 2. GEMMs

def linear_case(pkg, ctx, M, K, N, geglu_, dtype, seed=10):
    x = f16v(rnd(M, K, seed=seed))
    w = f16v(rnd(K, N, seed=seed + 1, scale=1 / math.sqrt(K)))
    b = 0.1 * rnd(N, seed=seed + 2)
    out = pkg.linear(ctx, x, w, b, geglu_, dtype)
    y = x.double() @ w.double() + b.double()
    ref, tol = gemm_bar(y, geglu_)
    return out, ref, tol


LINEARS = [  # M, K, N, geglu: the transformer projections (QKV, out, GEGLU N = 8C, FF-out K = 4C) + split-K + ragged M
    (8192, 640, 1920, False), (8192, 640, 640, False), (8192, 640, 5120, True), (8192, 2560, 640, False),      # base 64^2, B = 2
    (2048, 1280, 3840, False), (2048, 1280, 1280, False), (2048, 1280, 10240, True), (2048, 5120, 1280, False),  # base 32^2, B = 2
    (4096, 640, 1920, False), (4096, 2560, 640, False), (1024, 1280, 10240, True), (1024, 5120, 1280, False),   # B = 1
    (8192, 768, 2304, False), (8192, 768, 6144, True), (8192, 3072, 768, False),                                 # refiner 64^2
    (2048, 1536, 4608, False), (2048, 1536, 12288, True), (2048, 6144, 1536, False), (512, 6144, 1536, False),   # refiner 32^2 / 16^2
    (1024, 10240, 1280, False), (512, 12288, 1536, False),                                                       # split-K (K >= 10240)
    (154, 2048, 1280, False), (154, 1280, 768, False), (1000, 1280, 1280, False), (4000, 640, 5120, True), (77, 640, 640, False),  # ragged M
]


@pytest.mark.parametrize("M,K,N,geglu_", LINEARS)
def test_linear_f16(pkg, ctx, M, K, N, geglu_):
    out, ref, tol = linear_case(pkg, ctx, M, K, N, geglu_, 1)
    check(f"linear dtype=1 M={M} K={K} N={N} geglu={geglu_}", out, ref, tol, 8e-3 if geglu_ else 4e-3)


@pytest.mark.parametrize("M,K,N,geglu_", [(8192, 640, 640, False), (2048, 1280, 10240, True), (2048, 5120, 1280, False),
                                           (154, 2048, 1280, False), (1024, 10240, 1280, False), (1000, 1280, 1280, False)])
def test_linear_generic_kernel(pkg, ctx, M, K, N, geglu_):
    out, ref, tol = linear_case(pkg, ctx, M, K, N, geglu_, 2)
    check(f"linear dtype=2 M={M} K={K} N={N} geglu={geglu_}", out, ref, tol, 8e-3 if geglu_ else 4e-3)


@pytest.mark.parametrize("variant", [60, 62])
@pytest.mark.parametrize("M,K,N", [(8192, 640, 640), (2048, 1280, 1280), (1000, 5120, 1280), (154, 2048, 1280)])
def test_linear_wreg_tile_heights(pkg, ctx, variant, M, K, N):
    out, ref, tol = with_variant(pkg, "igemm_variant", variant, lambda: linear_case(pkg, ctx, M, K, N, False, 1))
    check(f"linear wreg variant={variant} M={M} K={K} N={N}", out, ref, tol, 4e-3)


def conv_ref(x, w, b, stride, pad, up):
    """fp64 convolution as a sum of per-tap GEMMs (NHWC), x [B,Cin,H,W], w [Cout,Cin,k,k]"""
    x = x.double().permute(0, 2, 3, 1)
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, H, W, Cin = x.shape
    Cout, _, k, _ = w.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    out = torch.zeros(B * Ho * Wo, Cout, dtype=torch.float64, device=x.device)
    wd = w.double()
    for dy in range(k):
        for dx in range(k):
            xs = xp[:, dy: dy + stride * (Ho - 1) + 1: stride, dx: dx + stride * (Wo - 1) + 1: stride, :]
            out += xs.reshape(-1, Cin) @ wd[:, :, dy, dx].t()
    if b is not None:
        out += b.double()
    return out.reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2)


CONVS = [  # B, Cin, H, W, Cout, k, stride, pad, upsample
    (2, 320, 128, 128, 320, 3, 1, 1, False), (2, 640, 64, 64, 640, 3, 1, 1, False), (2, 1280, 32, 32, 1280, 3, 1, 1, False),
    (1, 640, 64, 64, 640, 3, 1, 1, False), (1, 1280, 32, 32, 1280, 3, 1, 1, False),
    (2, 320, 64, 64, 640, 3, 1, 1, False), (2, 640, 32, 32, 1280, 3, 1, 1, False),                 # channel-doubling ResBlock conv1
    (2, 1920, 64, 64, 640, 3, 1, 1, False), (2, 960, 128, 128, 320, 3, 1, 1, False),               # decoder ResBlocks (K = 17280 / 8640)
    (2, 2560, 32, 32, 1280, 3, 1, 1, False),
    (2, 320, 64, 64, 640, 1, 1, 0, False), (2, 1920, 64, 64, 640, 1, 1, 0, False), (2, 960, 128, 128, 320, 1, 1, 0, False),  # 1x1 skips
    (2, 320, 128, 128, 320, 3, 2, 1, False), (2, 640, 64, 64, 640, 3, 2, 1, False),                 # Downsample
    (2, 1280, 32, 32, 1280, 3, 1, 1, True), (2, 640, 64, 64, 640, 3, 1, 1, True),                   # Upsample (fused nearest 2x)
    (2, 4, 128, 128, 320, 3, 1, 1, False), (2, 320, 128, 128, 4, 3, 1, 1, False),                   # conv_in / conv_out
    (2, 384, 128, 128, 384, 3, 1, 1, False), (2, 1536, 32, 32, 1536, 3, 1, 1, False), (2, 1536, 16, 16, 1536, 3, 1, 1, False),  # refiner
    (2, 768, 64, 64, 768, 3, 1, 1, False), (2, 3072, 16, 16, 1536, 3, 1, 1, False),
]


def conv_case(pkg, ctx, B, Cin, H, W, Cout, k, stride, pad, up, dtype, seed=20):
    x = f16v(rnd(B, Cin, H, W, seed=seed))
    w = f16v(rnd(Cout, Cin, k, k, seed=seed + 1, scale=1 / math.sqrt(Cin * k * k)))
    b = 0.1 * rnd(Cout, seed=seed + 2)
    out = pkg.conv2d(ctx, x, w, b, stride, pad, up, dtype)
    ref = conv_ref(x, w, b, stride, pad, up)
    return out, ref, U * ref.abs().max()


@pytest.mark.parametrize("B,Cin,H,W,Cout,k,stride,pad,up", CONVS)
def test_conv2d_f16(pkg, ctx, B, Cin, H, W, Cout, k, stride, pad, up):
    out, ref, tol = conv_case(pkg, ctx, B, Cin, H, W, Cout, k, stride, pad, up, 1)
    check(f"conv2d dtype=1 {(B, Cin, H, W, Cout, k, stride, pad, up)}", out, ref, tol, 4e-3)


@pytest.mark.parametrize("B,Cin,H,W,Cout,k,stride,pad,up", [CONVS[1], CONVS[2], CONVS[7], CONVS[13], CONVS[15], CONVS[17]])
def test_conv2d_generic_kernel(pkg, ctx, B, Cin, H, W, Cout, k, stride, pad, up):
    out, ref, tol = conv_case(pkg, ctx, B, Cin, H, W, Cout, k, stride, pad, up, 2)
    check(f"conv2d dtype=2 {(B, Cin, H, W, Cout, k, stride, pad, up)}", out, ref, tol, 4e-3)


# ----------------------------------------------------------------------------------------------------------------- 3. folded LayerNorm

def ln_stats(x, eps):
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    return mu, var, 1.0 / torch.sqrt(var + eps)


def fold_ref(x16, gamma, beta, w, b, eps):
    """fp64 emulation of the folded LayerNorm -> linear (module docstring): (y, per-element cancellation bar)"""
    K = w.shape[0]
    wf = (w * gamma[:, None]).half().double()                  # pack_linear_kernel: f16(fp32(w gamma))
    cs = wf.sum(0)
    bf = beta.double() @ w.double() + (b.double() if b is not None else 0.0)
    mu, _, rstd = ln_stats(x16, eps)
    y = rstd * (x16.double() @ wf) - rstd * mu * cs + bf
    canc = 8 * 2.0 ** -24 * K * (rstd * mu.abs()) * wf.pow(2).mean(0).sqrt()
    return y, canc


@pytest.mark.parametrize("M,K,N,geglu_", [(8192, 640, 1920, False), (8192, 640, 5120, True), (2048, 1280, 3840, False),
                                           (2048, 1280, 10240, True), (4096, 768, 2304, False), (1000, 1536, 12288, True),
                                           (300, 1536, 1536, False)])
@pytest.mark.parametrize("large_mean", [False, True])
def test_layer_norm_linear_folded(pkg, ctx, M, K, N, geglu_, large_mean):
    eps = 1e-5
    x = rnd(M, K, seed=30, scale=2.0, shift=0.3)
    if large_mean:       # every 4th row: |mu| = 20 sigma (outlier channels of a real residual stream), row 1 at |mu| = 100 sigma
        x[::4] = rnd(M, K, seed=31, scale=0.5)[::4] + 10.0 * torch.sign(rnd(M, 1, seed=32)[::4])
        x[1] = rnd(K, seed=33, scale=0.05) - 5.0
    x16 = f16v(x)
    gamma, beta = 1 + 0.1 * rnd(K, seed=34), 0.1 * rnd(K, seed=35)
    w = rnd(K, N, seed=36, scale=1 / math.sqrt(K))
    b = 0.1 * rnd(N, seed=37)
    out = pkg.layer_norm_linear(ctx, x16, gamma, beta, w, b, eps, geglu_, 1)
    y, canc = fold_ref(x16, gamma, beta, w, b, eps)
    if geglu_:
        ref, slack = geglu(y, U * y.abs().max() + canc)
        n = N // 2
        tol = U * ref.abs().max() + slack + y[:, :n].abs() * (0.75e-7 * y[:, n:].abs() + 2e-6 * F.gelu(y[:, n:]).abs())
    else:
        ref, tol = y, U * y.abs().max() + canc
    check(f"layer_norm_linear folded M={M} K={K} N={N} geglu={geglu_} large_mean={large_mean}", out, ref, tol,
          8e-3 if geglu_ else 4e-3)


# ----------------------------------------------------------------------------------------------------------------- 4. norms

def norm_bar(ref, mu, sigma, rstd, gamma_abs):
    t = U * ref.abs().max() + 8 * 2.0 ** -24 * (mu.abs() + sigma) * rstd * gamma_abs
    return t + ulp16(ref.abs() + t) / 2


def gn_ref(h, gamma, beta, G, eps, silu):
    """fp64 GroupNorm(+SiLU) of h [B,C,H,W] -> (out, mu, sigma, rstd) broadcast to h's shape"""
    B, C = h.shape[:2]
    hg = h.double().reshape(B, G, -1)
    mu = hg.mean(-1, keepdim=True)
    var = ((hg - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = ((hg - mu) * rstd).reshape(h.shape)
    y = xh * gamma.double()[None, :, None, None] + beta.double()[None, :, None, None]
    exp = lambda t: t.expand(B, G, hg.shape[-1]).reshape(h.shape)
    return (F.silu(y) if silu else y), exp(mu), exp(var.sqrt()), exp(rstd)


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("B,C,H,W,silu,mean", [(2, 320, 128, 128, True, 0.3), (2, 640, 64, 64, True, 0.0), (2, 1280, 32, 32, False, 0.0),
                                               (1, 2560, 32, 32, True, 0.0), (2, 960, 64, 64, True, 0.0), (1, 640, 64, 64, False, 40.0),
                                               (2, 512, 128, 128, True, -25.0)])
def test_group_norm_f16(pkg, ctx, dtype, B, C, H, W, silu, mean):
    x = rnd(B, C, H, W, seed=40, scale=0.05 if abs(mean) > 1 else 3.0, shift=mean)
    if dtype == 1:
        x = f16v(x)          # dtype 1 stores the input as f16; dtype 2 keeps it fp32
    gamma, beta = 1 + 0.1 * rnd(C, seed=41), 0.1 * rnd(C, seed=42)
    out = pkg.group_norm(ctx, x, gamma, beta, 32, 1e-5, silu, dtype)
    ref, mu, sg, rstd = gn_ref(x, gamma, beta, 32, 1e-5, silu)
    tol = norm_bar(ref, mu, sg, rstd, 1.1 * gamma.double().abs()[None, :, None, None])
    check(f"group_norm dtype={dtype} {(B, C, H, W)} silu={silu} mean={mean}", out, ref, tol, 6e-3 if abs(mean) > 1 else 4e-3)


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("rows,C,mean", [(8192, 640, 0.3), (2048, 1280, 0.3), (4096, 768, 0.0), (154, 2048, 0.0), (1000, 1536, 30.0),
                                         (300, 640, -200.0)])
def test_layer_norm_f16(pkg, ctx, dtype, rows, C, mean):
    x = rnd(rows, C, seed=43, scale=0.05 if abs(mean) > 1 else 2.0, shift=mean)
    if dtype == 1:
        x = f16v(x)
    gamma, beta = 1 + 0.1 * rnd(C, seed=44), 0.1 * rnd(C, seed=45)
    out = pkg.layer_norm(ctx, x, gamma, beta, 1e-5, dtype)
    mu, var, rstd = ln_stats(x, 1e-5)
    ref = (x.double() - mu) * rstd * gamma.double() + beta.double()
    tol = norm_bar(ref, mu, var.sqrt(), rstd, gamma.double().abs())
    check(f"layer_norm dtype={dtype} rows={rows} C={C} mean={mean}", out, ref, tol, 4e-3)


@pytest.mark.parametrize("B,Cin,H,W,Cout,res", [(2, 640, 64, 64, 640, False), (2, 1280, 32, 32, 1280, True), (2, 320, 64, 64, 640, True),
                                                (2, 1920, 64, 64, 640, False), (1, 64, 16, 16, 128, False), (2, 320, 128, 128, 320, False),
                                                (2, 128, 24, 24, 128, True)])
def test_conv2d_group_norm_f16(pkg, ctx, B, Cin, H, W, Cout, res):
    # the shapes of test_conv2d_group_norm_statistics_from_producer; both paths against one emulation: h = f16(conv + b + r) (the
    # kernel rounds an fp32 value: rounding_slack), GroupNorm + SiLU of h in fp64, f16 output
    x = f16v(rnd(B, Cin, H, W, seed=50, scale=1.2, shift=0.3))
    w = f16v(rnd(Cout, Cin, 3, 3, seed=51, scale=1 / math.sqrt(9 * Cin)))
    b = 0.5 * rnd(Cout, seed=52) + 2.0
    r = f16v(rnd(B, Cout, H, W, seed=53)) if res else None
    gamma, beta = 1 + 0.1 * rnd(Cout, seed=54), 0.1 * rnd(Cout, seed=55)
    hx = conv_ref(x, w, b, 1, 1, False) + (r.double() if res else 0.0)
    h, sp = rounding_slack(hx, U * hx.abs().max().item())
    ref, mu, sg, rstd = gn_ref(h, gamma, beta, 32, 1e-5, True)
    G = 32
    sp_mean = sp.reshape(B, G, -1).mean(-1, keepdim=True).expand(B, G, H * W * Cout // G).reshape(h.shape)
    ga = gamma.double().abs()[None, :, None, None]
    tol = norm_bar(ref, mu, sg, rstd, 1.1 * ga) + 1.1 * ga * rstd * (sp + sp_mean * (1 + ((h - mu) * rstd).abs()))
    for fused in (True, False):
        out, took = pkg.conv2d_group_norm(ctx, x, w, b, gamma, beta, 1e-5, 32, True, r, fused=fused)
        check(f"conv->GN {(B, Cin, H, W, Cout)} res={res} fused={fused} (statistics from the producer: {took})", out, ref, tol, 4e-3)


# ----------------------------------------------------------------------------------------------------------------- 5./6. attention

def prescale(q16, scale):
    """the kernels' Q pre-scale, bit-exact: f16(fp32(q) * fp32(scale * log2 e))"""
    sc = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    return (q16.float() * sc.to(q16.device)).half().double()


def attn_ref(q2, k, v, heads, mask=None, sq=None, chunk=1024):
    """fp64 attention in the exp2 domain on the pre-scaled q2 [B,Nq,C] and f16 k, v -> (O, per-element bar without the output term)"""
    B, Nq, C = q2.shape
    d = C // heads
    O = torch.empty(B, Nq, C, dtype=torch.float64, device=DEV)
    bar = torch.empty_like(O)
    kd, vd = k.double(), v.double()
    for b in range(B):
        for h in range(heads):
            cs = slice(h * d, (h + 1) * d)
            kh, vh = kd[b, :, cs], vd[b, :, cs]
            for q0 in range(0, Nq, chunk):
                qs = slice(q0, min(Nq, q0 + chunk))
                s = q2[b, qs, cs] @ kh.t()
                if mask is not None:
                    s = s + mask[qs].double() * LOG2E
                p = torch.exp2(s - s.max(-1, keepdim=True).values)
                l = p.sum(-1, keepdim=True)
                o = (p @ vh) / l
                # P's rounding: min(worst case, Hoeffding at 8 sigma) on normal P, 2^-25 per subnormal P (module docstring)
                e = torch.minimum(UH * p @ vh.abs(), 8 * UH * torch.sqrt((p * p) @ (vh * vh))) / l
                e = e + (2.0 ** -25 * ((p > 0) & (p < 2.0 ** -14)).double()) @ vh.abs() / l
                if sq is not None:
                    pe = p * (sq[b, qs, cs] @ kh.abs().t())
                    e = e + math.log(2) * 1.1 * (pe @ vh.abs() + o.abs() * pe.sum(-1, keepdim=True)) / l
                O[b, qs, cs] = o
                bar[b, qs, cs] = e
    return O, bar


def attn_check(tag, out, O, bar):
    tol = bar + U * O.abs().max()
    check(tag, out, O, tol + ulp16(O.abs() + tol) / 2, 6e-3)


def self_attn(pkg, ctx, B, N, heads, seed, variant=0, spikes=False, Nk=None):
    C = 64 * heads
    Nk = Nk or N
    q, k, v = f16v(rnd(B, N, C, seed=seed)), f16v(rnd(B, Nk, C, seed=seed + 1)), f16v(rnd(B, Nk, C, seed=seed + 2))
    if spikes:     # late running-max jumps (test_qkv_attention_online_softmax_rescale), in every head of entry 0
        k[0, 3000] = q[0, 3] * 6.0
        k[0, 4000] = q[0, 77] * 2.5
        k[0, 10] = q[0, 130] * 9.0
        k[0, 2049] = q[0, 2048] * 4.0
        k = f16v(k)
    out = with_variant(pkg, "attn_variant", variant, lambda: pkg.qkv_attention(ctx, q, k, v, None, heads, 1))
    O, bar = attn_ref(prescale(q, 0.125), k, v, heads)
    return out, O, bar


@pytest.mark.parametrize("B,N,heads,body", [(2, 4096, 10, "mix level 0"), (2, 1024, 20, "mix level 2"), (2, 4096, 12, "variant 2"),
                                             (2, 1024, 24, "key split"), (2, 256, 24, "key split"), (1, 4096, 10, "mix level 0"),
                                             (1, 1024, 20, "mix level 2"), (1, 4096, 12, "variant 2"), (1, 1024, 24, "key split"),
                                             (1, 256, 24, "key split")])
def test_self_attention_d64(pkg, ctx, B, N, heads, body):
    out, O, bar = self_attn(pkg, ctx, B, N, heads, seed=60)
    attn_check(f"self-attention B={B} N={N} heads={heads} ({body})", out, O, bar)


@pytest.mark.parametrize("variant,B,N,heads", [(6, 2, 1024, 20), (7, 2, 4096, 10), (8, 2, 1024, 20), (6, 1, 4096, 12)])
def test_self_attention_d64_forced_variants(pkg, ctx, variant, B, N, heads):
    out, O, bar = self_attn(pkg, ctx, B, N, heads, seed=61, variant=variant)
    attn_check(f"self-attention variant={variant} B={B} N={N} heads={heads}", out, O, bar)


@pytest.mark.parametrize("variant", [0, 2, 6])
def test_self_attention_d64_late_max_jumps(pkg, ctx, variant):
    out, O, bar = self_attn(pkg, ctx, 1, 4096, 10, seed=62, variant=variant, spikes=True)
    attn_check(f"self-attention 4096 keys with late max jumps, variant={variant}", out, O, bar)


@pytest.mark.parametrize("B,Nq,C", [(2, 1024, 1280), (2, 4096, 640), (2, 4096, 768), (2, 1024, 1536)])
def test_cross_attention_77_keys(pkg, ctx, B, Nq, C):
    out, O, bar = self_attn(pkg, ctx, B, Nq, C // 64, seed=63, Nk=77)
    attn_check(f"qkv_attention Nk=77 B={B} Nq={Nq} C={C}", out, O, bar)


def test_masked_attention_clip_causal(pkg, ctx):
    B, N, C, heads = 2, 77, 768, 12
    q, k, v = f16v(rnd(B, N, C, seed=64)), f16v(rnd(B, N, C, seed=65)), f16v(rnd(B, N, C, seed=66))
    mask = OM.attn_decoder_mask(N).to(DEV)
    out = pkg.qkv_attention(ctx, q, k, v, mask, heads, 1)
    O, bar = attn_ref(prescale(q, 0.125), k, v, heads, mask=mask)
    attn_check("masked attention (CLIP causal 77x77)", out, O, bar)


@pytest.mark.parametrize("N", [16384, 1000])
def test_wide_head_attention_vae_mid(pkg, ctx, N):
    # attn_hd_kernel<512>: the VAE mid-block's single head at 128^2 latent tokens, and a ragged count
    C = 512
    q, k, v = f16v(rnd(1, N, C, seed=67)), f16v(rnd(1, N, C, seed=68)), f16v(rnd(1, N, C, seed=69))
    out = pkg.qkv_attention(ctx, q, k, v, None, 1, 1)
    O, bar = attn_ref(prescale(q, float(torch.tensor(1 / math.sqrt(512), dtype=torch.float32))), k, v, 1, chunk=2048)
    attn_check(f"wide-head attention N={N}", out, O, bar)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B,Nq,C,ctx_dim", [(2, 1024, 1280, 2048), (2, 4096, 640, 2048), (2, 4096, 768, 1280)])
def test_ln_query_cross_attention_f16(pkg, ctx, fused, B, Nq, C, ctx_dim):
    # LN -> folded query projection -> 77-key attention; the context (width 2048, the refiner's 1280) projected to K / V upstream
    eps, Nk = 1e-5, 77
    x16 = f16v(rnd(B, Nq, C, seed=70, scale=1.5, shift=0.2))
    gamma, beta = 1 + 0.1 * rnd(C, seed=71), 0.1 * rnd(C, seed=72)
    wq = rnd(C, C, seed=73, scale=1 / math.sqrt(C))
    cx = rnd(B, Nk, ctx_dim, seed=74)
    k = f16v(cx @ rnd(ctx_dim, C, seed=75, scale=1 / math.sqrt(ctx_dim)))
    v = f16v(cx @ rnd(ctx_dim, C, seed=76, scale=1 / math.sqrt(ctx_dim)))
    out = pkg.ln_query_cross_attention(ctx, x16, gamma, beta, wq, k, v, eps, fused)
    q, canc = fold_ref(x16.reshape(-1, C), gamma, beta, wq, None, eps)
    q = q.reshape(B, Nq, C)
    dq = U * q.abs().max() + canc.reshape(B, Nq, C)
    sc = float(torch.tensor(0.125, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    if fused:      # f16(q_fp32 * sc) in the epilogue
        q2, sq = rounding_slack(q * sc, dq * sc)
    else:          # q stored as f16, then the attention kernel's pre-scale
        q1, s1 = rounding_slack(q, dq)
        q2 = prescale(q1.float(), 0.125)
        sq = s1 * sc + ulp16(q2) * (s1 > 0)
    O, bar = attn_ref(q2, k, v, C // 64, sq=sq)
    attn_check(f"ln_query_cross_attention fused={fused} B={B} Nq={Nq} C={C} context {ctx_dim}", out, O, bar)
