"""fp64 references, CPU emulations of each mode's documented arithmetic, plantable defects, case tables and input builders for the two blocks of the
autoencoder that run as single-op entries (sdxl_vae_attn_block / sdxl_vae_res_block -> vae_attn_block / vae_res_block of csrc/vae.cpp).  torch / numpy on
the CPU; no GPU, no engine.  tests/test_gpu_vae_blocks.py sends the operands built here to the GPU; tests/test_cpu_vae_block_ref.py shows on the same
operands that each planted defect leaves the bounds.

References (fp64, following oracle/model.py::vae_attn_block / vae_resnet_block): GroupNorm with biased variance and eps inside the sqrt, softmax of
q k^T C^-1/2, one head of C channels.

Emulations (fp32 on the CPU; `mode` is the name of the dtype):
  "f32"    everything in fp32.
  "f16"    the stream is f16 (a VAE of that dtype keeps it so: the input is rounded on entry, the output on exit); GEMM operands and every stored
           activation are rounded to f16, products accumulate in fp32.  GroupNorm and softmax compute in fp32 from what was stored.
  "split"  fp32 stream; every GEMM operand is a pair hi = f16(x), lo = f16(x - hi) (f16 subnormals honoured: torch's conversion keeps them), a product is
           a_h w_h + a_l w_h + a_h w_l in fp32.  Weights are split after the power of two that brings max|w| into [2^13, 2^14) (undone exactly).  The
           attention's P is stored times 2^12 before the split and the P V product divided by it.  The nin_shortcut reads x times, per batch entry, the
           power of two that brings that entry's max|x| into [2^13, 2^14), and its GEMM multiplies the inverse back.

Bounds: nothing is fixed in advance and nothing comes from a GPU.  bound(case, mode) = MARGIN[mode] x (error of that mode's emulation against fp64 on
that case's operands).  MARGIN is 4 for f32 / split (another summation order, the dropped lo x lo products of 2^-22 each, MFMA-internal rounding) and 2
for f16 (the project's "<= 2 x measured" convention: operand rounding, which the emulation reproduces, dominates there).

Error metrics: attention block max|out - ref| / max|ref - x| (the branch, not the residual passing through); res block max|out - ref| / max|ref| per
batch entry (the magnitude case's entries differ by 2^22)."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

MODES = {0: "f32", 1: "f16", 3: "split"}      # SDXL_DTYPE_F32, _F16, _F32_SPLIT
MARGIN = {"f32": 4.0, "f16": 2.0, "split": 4.0}
N_GROUP = 32
EPS = 1e-6
QT = 8192          # query rows per pass of the un-fused chain (vae_attn_block)
P_SCALE = 4096.0   # split mode: P is stored times 2^12

# (name, B, C, H, W)
ATTN_CASES = (
    ("base_8x8", 2, 512, 8, 8),
    ("ragged_9x9", 1, 512, 9, 9),            # split mode: fp32 V^T fallback (HW % 8 != 0); ragged flash tiles in f16
    ("wide_24x40", 2, 512, 24, 40),          # H != W
    ("c128_12x20", 2, 128, 12, 20),          # the un-fused chain in f16 too
    ("two_pass_90x92", 1, 512, 90, 92),      # 8192 + 88 query rows, keys padded to 8288
    ("flat_90x92", 1, 512, 90, 92),          # the same shape with a flat softmax over zero-mean values: every P ~ 1.2e-4 (f32 and split only, see attn_inputs)
)
# modes a case runs in (default: all three)
ATTN_CASE_MODES = {"flat_90x92": ("f32", "split")}
# (name, B, Cin, Cout, H, W, magnitude)
RES_CASES = (
    ("nin_16x24", 2, 128, 64, 16, 24, False),      # shortcut; 12 row splits of the statistics pass
    ("plain_5x5", 1, 64, 64, 5, 5, False),         # no shortcut; one split
    ("cap_64x80", 2, 256, 128, 64, 80, False),     # the 128-split cap
    ("magnitude_16x24", 2, 128, 64, 16, 24, True),  # entry 0 times 2^15, entry 1 times 2^-7; f32 and split only
)

ATTN_DEFECTS = ("scale_quarter", "norm_256", "pass_offset", "pv_tail", "batch_keys", "p_lo_dropped", "p_noscale")
RES_DEFECTS = ("one_scale", "no_a_scale", "absmax_no_last_row")


def attn_case(name):
    return next(c for c in ATTN_CASES if c[0] == name)


def res_case(name):
    return next(c for c in RES_CASES if c[0] == name)


def attn_modes(name):
    return ATTN_CASE_MODES.get(name, tuple(MODES.values()))


def attn_defect_applies(defect, name, mode):
    """where a defect is held to the 5 x factor: the shapes and modes at which it changes what the block computes.  p_noscale (P stored without its 2^12)
    costs precision only where the probabilities that carry the output are small enough for the lo halves of P to fall under the f16 subnormal quantum
    2^-24: on the peaked rows of the other cases (row maxima ~0.15) the large probabilities carry the output and keep 22 bits without the scale -- measured
    0.3 ... 0.5 x the bound there, recorded in test_cpu_vae_block_ref.py -- so it is held to the factor on the flat case, which was built for it."""
    _, B, C, H, W = attn_case(name)
    HW = H * W
    if mode not in attn_modes(name) or (defect in ("p_lo_dropped", "p_noscale") and mode != "split"):
        return False
    return {"scale_quarter": True, "norm_256": HW > 256, "pass_offset": HW > QT, "pv_tail": HW % 32 != 0, "batch_keys": B > 1,
            "p_lo_dropped": True, "p_noscale": name.startswith("flat")}[defect]


def res_defect_applies(defect, name, mode):
    """the shortcut's per-entry scaling exists in the split mode only; its defects are planted on the magnitude case, whose inputs are built for them"""
    return mode == "split" and res_case(name)[6]


def subset_rows(HW):
    """query rows that are compared: all of them, or for the two-pass case rows 0-63, the last 152 (both sides of the pass boundary at 8192) and 64 spread between"""
    if HW <= QT:
        return np.arange(HW)
    mid = np.linspace(64, HW - 153, 64).astype(np.int64)
    return np.unique(np.concatenate([np.arange(64), mid, np.arange(HW - 152, HW)]))


# ------------------------------------------------------------------------------------------------------------------ inputs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


_inputs = {}


def attn_inputs(name):
    """fp32 operands of an attention case (built once, never modified).  wq / wk ~ N(0,1) 1.5 / sqrt(C) and wv / wo ~ N(0,1) / sqrt(C) give scores of
    std ~2.3 and peaked rows of P (a near-uniform softmax would hide every defect of the chain); x ~ unit variance with a per-channel offset.
    The flat case is the exception, built for one defect the peaked cases cannot see (P stored without its 2^12, split mode): q and k a tenth as large
    (scores of std ~0.02: P ~ 1 / 8280 everywhere, its lo halves under the f16 subnormal quantum unless scaled) and zero-mean values (no channel offset, no
    beta, bv, bo), so the output is the small random sum a lost lo half shows in, not a mean that hides it."""
    if name not in _inputs:
        _, B, C, H, W = attn_case(name)
        g = _gen(name)
        r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        d = {"x": r(B, C, H, W) + 0.5 * r(1, C, 1, 1), "gamma": 1.0 + 0.2 * r(C), "beta": 0.1 * r(C)}
        for k, sc in (("q", 1.5), ("k", 1.5), ("v", 1.0), ("o", 1.0)):
            d["w" + k] = r(C, C) * (sc / math.sqrt(C))
            d["b" + k] = 0.1 * r(C)
        if name.startswith("flat"):
            d["x"] = r(B, C, H, W)
            for k in ("wq", "wk", "bq", "bk"):
                d[k] = d[k] * 0.1
            for k in ("beta", "bv", "bo"):
                d[k] = torch.zeros(C)
        _inputs[name] = {k: v.contiguous() for k, v in d.items()}
    return _inputs[name]


def res_inputs(name):
    """fp32 operands of a res-block case.  The magnitude case: entry 0 times 2^15, entry 1 times 2^-7 (powers of two: the reference stays exact), each
    entry's largest element, 8 x the rest, at its last pixel of its last channel; conv2 and its bias times 2^-12 there, so that the shortcut -- the path
    the case is about -- carries each entry's output and an error of it is not hidden under the branch."""
    if name not in _inputs:
        _, B, Cin, Cout, H, W, mag = res_case(name)
        g = _gen(name)
        r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        x = r(B, Cin, H, W) + 0.5 * r(1, Cin, 1, 1)
        d = {"gamma1": 1.0 + 0.2 * r(Cin), "beta1": 0.1 * r(Cin), "w1": r(Cout, Cin, 3, 3) / math.sqrt(9 * Cin), "b1": 0.1 * r(Cout),
             "gamma2": 1.0 + 0.2 * r(Cout), "beta2": 0.1 * r(Cout), "w2": r(Cout, Cout, 3, 3) / math.sqrt(9 * Cout), "b2": 0.1 * r(Cout),
             "w_nin": None, "b_nin": None}
        if Cin != Cout:
            d["w_nin"], d["b_nin"] = r(Cout, Cin, 1, 1) / math.sqrt(Cin), 0.1 * r(Cout)
        if mag:
            for b, e in ((0, 15), (1, -7)):
                x[b, -1, -1, -1] = 8.0 * x[b].abs().max()
                x[b] *= 2.0 ** e
            d["w2"], d["b2"] = d["w2"] * 2.0 ** -12, d["b2"] * 2.0 ** -12
            d["b_nin"] = d["b_nin"] * 2.0 ** -7      # (within entry 1's shortcut range, so that entry's output is the GEMM's, not the bias's)
        d["x"] = x
        _inputs[name] = {k: (None if v is None else v.contiguous()) for k, v in d.items()}
    return _inputs[name]


# ------------------------------------------------------------------------------------------------------------------ fp64 references
def _gn64(x, gamma, beta, silu):
    B, C = x.shape[:2]
    y = x.reshape(B, N_GROUP, -1)
    y = (y - y.mean(-1, keepdim=True)) / torch.sqrt(y.var(-1, unbiased=False, keepdim=True) + EPS)
    y = y.reshape(x.shape) * gamma.reshape(1, C, 1, 1) + beta.reshape(1, C, 1, 1)
    return y * torch.sigmoid(y) if silu else y


def _rows(t):
    """[B,C,H,W] -> [B,HW,C]"""
    B, C = t.shape[:2]
    return t.reshape(B, C, -1).transpose(1, 2).contiguous()


_refs = {}


def attn_ref(name):
    """(out rows [B,R,C], x rows [B,R,C]) in fp64 at subset_rows of the case: computed once, shared, never modified"""
    if ("a", name) not in _refs:
        d = {k: v.double() for k, v in attn_inputs(name).items()}
        C = d["x"].shape[1]
        rows = torch.from_numpy(subset_rows(d["x"].shape[2] * d["x"].shape[3]))
        hn, xr = _rows(_gn64(d["x"], d["gamma"], d["beta"], False)), _rows(d["x"])
        w = lambda k: d["w" + k].reshape(C, C).T      # noqa: E731
        q, k, v = hn[:, rows] @ w("q") + d["bq"], hn @ w("k") + d["bk"], hn @ w("v") + d["bv"]
        p = torch.softmax(q @ k.transpose(1, 2) * C ** -0.5, -1)
        _refs[("a", name)] = (xr[:, rows] + (p @ v) @ w("o") + d["bo"], xr[:, rows])
    return _refs[("a", name)]


def res_ref(name):
    """out [B,Cout,H,W] in fp64"""
    if ("r", name) not in _refs:
        d = {k: (None if v is None else v.double()) for k, v in res_inputs(name).items()}
        h = F.conv2d(_gn64(d["x"], d["gamma1"], d["beta1"], True), d["w1"], d["b1"], padding=1)
        h = F.conv2d(_gn64(h, d["gamma2"], d["beta2"], True), d["w2"], d["b2"], padding=1)
        _refs[("r", name)] = (F.conv2d(d["x"], d["w_nin"], d["b_nin"]) if d["w_nin"] is not None else d["x"]) + h
    return _refs[("r", name)]


# ------------------------------------------------------------------------------------------------------------------ emulations
def f16(x):
    return x.half().float()


def _pow2_scale(absmax):
    """hl_stream_scale / WeightBuilder::hl_scale: the power of two that brings absmax into [2^13, 2^14)"""
    if not (absmax > 0.0 and math.isfinite(absmax)):
        return 1.0
    return 2.0 ** (14 - math.frexp(absmax)[1])


def _operand(mode, x):
    """an activation as its mode stores it / hands it to a GEMM: tuple of fp32 parts"""
    if mode == "f32":
        return (x,)
    h = f16(x)
    return (h,) if mode == "f16" else (h, f16(x - h))


def _weight(mode, w):
    if mode != "split":
        return _operand(mode, w)
    sc = _pow2_scale(float(w.abs().max()))
    h, l = _operand(mode, w * sc)
    return (h / sc, l / sc)


def _mm(a, w):
    """a [..,M,K] parts x w [..,N,K] parts -> [..,M,N] fp32: a_h w_h (+ a_l w_h + a_h w_l)"""
    wt = [p.transpose(-1, -2) for p in w]
    out = a[0] @ wt[0]
    if len(a) > 1:
        out = out + a[1] @ wt[0]
    if len(wt) > 1:
        out = out + a[0] @ wt[1]
    return out


def _conv3(a, w):
    out = F.conv2d(a[0], w[0], padding=1)
    if len(a) > 1:
        out = out + F.conv2d(a[1], w[0], padding=1)
    if len(w) > 1:
        out = out + F.conv2d(a[0], w[1], padding=1)
    return out


def _gn32(x, gamma, beta, silu):
    B, C = x.shape[:2]
    y = x.reshape(B, N_GROUP, -1)
    y = (y - y.mean(-1, keepdim=True)) * torch.rsqrt(y.var(-1, unbiased=False, keepdim=True) + np.float32(EPS))
    y = y.reshape(x.shape) * gamma.reshape(1, C, 1, 1) + beta.reshape(1, C, 1, 1)
    return y / (1.0 + torch.exp(-y)) if silu else y


def _stream(mode, x):
    return f16(x) if mode == "f16" else x


def attn_emulate(name, mode, defect=None, stages=None):
    """out rows [B,R,C] (fp32) of the attention block in `mode` at subset_rows(HW); stages: a dict that receives the intermediate tensors
    (scores, P, P V, out) for locating a disagreement"""
    d = attn_inputs(name)
    B, C, H, W = d["x"].shape
    HW = H * W
    rows = torch.from_numpy(subset_rows(HW))
    x = _stream(mode, d["x"])
    xr = _rows(x)
    hn = _operand(mode, _rows(_gn32(x, d["gamma"], d["beta"], False)))
    w = {k: _weight(mode, d["w" + k].reshape(C, C)) for k in "qkvo"}
    q, k, v = (_operand(mode, _mm(hn, w[n]) + d["b" + n]) for n in "qkv")      # stored in the compute dtype, [B,HW,C]
    src = torch.where(rows >= QT, rows - QT, rows) if defect == "pass_offset" else rows
    scale = np.float32(C ** -0.25 if defect == "scale_quarter" else C ** -0.5)
    ps = P_SCALE if mode == "split" and defect != "p_noscale" else 1.0
    nk = HW - HW % 32 if defect == "pv_tail" else HW
    outs = []
    for b in range(B):
        kb = 0 if defect == "batch_keys" and b == 1 else b
        S = _mm([p[b, src] for p in q], [p[kb] for p in k])
        z = S * scale
        e = torch.exp(z - z.max(-1, keepdim=True).values)
        den = (e[:, :256] if defect == "norm_256" else e).sum(-1, keepdim=True)
        P = _operand(mode, e * (np.float32(ps) / den))
        if defect == "p_lo_dropped":
            P = (P[0], torch.zeros_like(P[0]))
        o = _mm([p[:, :nk] for p in P], [p[b, :nk].T for p in v]) * np.float32(1.0 / ps)
        y = _mm(_operand(mode, o), w["o"]) + d["bo"] + xr[b, rows]
        outs.append(_stream(mode, y))
        if stages is not None:
            stages.setdefault("scores", []).append(S); stages.setdefault("P", []).append(P[0] / ps)
            stages.setdefault("PV", []).append(o); stages.setdefault("out", []).append(outs[-1])
    return torch.stack(outs)


def res_emulate(name, mode, defect=None):
    """out [B,Cout,H,W] (fp32) of the res block in `mode`"""
    d = res_inputs(name)
    x = _stream(mode, d["x"])
    B, Cin = x.shape[:2]
    h = _stream(mode, _conv3(_operand(mode, _gn32(x, d["gamma1"], d["beta1"], True)), _weight(mode, d["w1"])) + d["b1"].reshape(1, -1, 1, 1))
    h = _conv3(_operand(mode, _gn32(h, d["gamma2"], d["beta2"], True)), _weight(mode, d["w2"])) + d["b2"].reshape(1, -1, 1, 1)
    if d["w_nin"] is None:
        return _stream(mode, h + x)
    wn = _weight(mode, d["w_nin"].reshape(-1, Cin))
    xr = _rows(x)
    short = []
    for b in range(B):
        sc = 1.0
        if mode == "split":      # hl_operand: one power of two per batch entry from the maxima norm1's statistics pass left
            src = x if defect == "one_scale" else x[b, :, :-1] if defect == "absmax_no_last_row" else x[b]
            sc = _pow2_scale(float(src.abs().max()))
        r = _mm(_operand(mode, xr[b] * np.float32(sc)), wn)
        if defect != "no_a_scale":
            r = r * np.float32(1.0 / sc)
        short.append(r + d["b_nin"])
    short = _stream(mode, torch.stack(short).transpose(1, 2).reshape(h.shape))
    return _stream(mode, h + short)


# ------------------------------------------------------------------------------------------------------------------ metrics and bounds
def attn_error(out_rows, name):
    """max|out - ref| / max|ref - x| over the compared rows (inf where out is not finite)"""
    ref, xr = attn_ref(name)
    o = out_rows.double()
    if not bool(torch.isfinite(o).all()):
        return math.inf
    return float((o - ref).abs().max() / (ref - xr).abs().max())


def res_errors(out, name):
    """per batch entry max|out - ref| / max|ref|"""
    ref = res_ref(name)
    o = out.double()
    return [float((o[b] - ref[b]).abs().max() / ref[b].abs().max()) if bool(torch.isfinite(o[b]).all()) else math.inf for b in range(ref.shape[0])]


_emu = {}


def attn_bound(name, mode):
    """(bound, emulation's own error): bound = MARGIN[mode] x error of the mode's emulation on this case's operands"""
    if ("a", name, mode) not in _emu:
        e = attn_error(attn_emulate(name, mode), name)
        _emu[("a", name, mode)] = (MARGIN[mode] * e, e)
    return _emu[("a", name, mode)]


def res_bounds(name, mode):
    """([bound per entry], [emulation's error per entry])"""
    if ("r", name, mode) not in _emu:
        e = res_errors(res_emulate(name, mode), name)
        _emu[("r", name, mode)] = ([MARGIN[mode] * v for v in e], e)
    return _emu[("r", name, mode)]
