"""Cases, fp64 references, per-mode CPU emulations and plantable defects for the entries of the UNet's block plan that run on their own through
sdxl_unet_block (UNet::run_block -> run_entry, res_block, spatial_transformer of csrc/unet.cpp: the code UNet::forward runs).  torch / numpy on the CPU;
no GPU, no engine.  tests/test_gpu_unet_blocks.py sends the operands built here to the GPU; tests/test_cpu_unet_block_ref.py shows on the same operands
that each planted defect leaves the bounds.

Models (CONFIGS; every case names its own through CONFIG_OF): "base", the base configuration with the deepest level's transformer depth cut from 10 to
2, and "refiner", the refiner configuration with every transformer depth cut from 4 to 2 (widths 384 / 768 / 1536 / 1536 on four levels, a 1280-wide
context, 6 / 12 / 24 heads, the deepest level without a transformer, ResU entries in the decoder).  Either way every entry has its model's widths,
embedding width and emb_off order.  The engine holds seeded synthetic weights; this module generates only the entry's own tensors
(oracle.config.synth_values is keyed by tensor name) and every *.lin_embed tensor of the case's model.

Reference: oracle.model._unet_block / res_block / spatial_transformer on float64 tensors, NUM in its default mode (nothing in those functions casts).

Emulations (fp32 on the CPU, roundings where the engine stores rounded values -- read from res_block / spatial_transformer of csrc/unet.cpp):
  dtype 1  f16: both operands of every GEMM and q, k, v, P of both attentions rounded to f16 (the oracle's `operands` emulation with every class on), the
           conv_in output h (stored in the compute dtype) and every write of the residual stream rounded to f16; x, emb-bias and statistics fp32.
           A ResBlock with a 1x1 skip writes the stream twice: the skip convolution stores skip(x) into the destination and conv_out adds it back as
           its residual operand (UNet::res_block of csrc/unet.cpp: run_conv(w.skip, ..., out, es); e2.R = out), two f16 roundings where a ResBlock
           without a skip has one.  The emulation first rounded x + h once in either kind; the refiner's rf_out_3072 (a ResBlock with a skip and
           nothing behind it, 64 rows) then sat at 1.10 of its bound on one entry, and the base's out_960_res, the same kind of entry, had been
           the file's worst line at 0.81.  No kernel at fault: the second rounding went into the emulation, for every case of both models.
  dtype 2  the same with an fp32 stream (h is still stored f16: Act h of res_block carries the compute dtype).
  dtype 0, 3, 7  fp32 arithmetic.  The GEMMs (convolutions as the implicit GEMM over C k k) accumulate as the MFMA k-loop does: one fp32 accumulator per
           output, rounded after every step of the chain, k ascending -- dtype 0: steps of 2 (v_mfma_f32_32x32x2_f32: PipeElem<float>::mma of
           csrc/igemm_common.h, "an fp32 fma chain per output"); split modes: steps of 16 (v_mfma_f32_32x32x16_f16), three per step, over the
           (hi, lo) f16 halves of both operands (a_h w_h + a_l w_h + a_h w_l; the weights split after the power of two that brings max|w| into
           [2^13, 2^14)).  A CPU matrix product sums K = 2880 ... 23040 terms in blocked vector lanes and leaves an eighth of that chain's
           rounding (measured here on the CPU: 4e-7 against 3.4e-6 at K = 11520), so without the chain the emulation is not the engine's
           arithmetic.  In the split modes the 1x1 skip convolution reads x times, per batch entry, the power of two that brings that entry's
           max|x| into [2^13, 2^14) (hl_operand from the maxima the norm_in statistics pass leaves) and multiplies the inverse back.
           Attention and the GEMV of the embedding bias stay the CPU's fp32.
  dtype 5  the classes mix_classes() reports on f16 operands (self-attention, QKV, both out-projections, GEGLU, FF-out, the operands of the
           cross-attention query projection); everything else fp32-class as in dtype 3.
Modes 5 and 7 run on f16-valued weights on both sides.

Error: per batch entry, max|out - ref64| over all elements / max|ref64| of that entry.
Bound: MARGIN x the emulation's error on the same case and entry; MARGIN is vae_block_ref's: 2 where operand rounding (which the emulation reproduces)
dominates (dtypes 1, 2, 5), 4 for the fp32-class modes (another summation order, the dropped lo x lo products, MFMA-internal rounding).  No chain got a
margin of its own: tests/test_cpu_unet_block_ref.py holds the emulation's error on two further input seeds of every case to the bound that seed 0 gives.
Nothing comes from a GPU result.

What the bounds are not.  (a) Fixed numbers: inside one accumulation step the order is the host BLAS's, so the emulation's error, and with it the
bound, moves by some 20 % from one test machine to another (res_320 in dtype 0: 1.66e-6 / 1.61e-6 on one, 1.41e-6 / 1.71e-6 on another).  (b) Tight in
the split modes on long K: the chain is emulated over the whole K, where the engine's in-launch split-K (K = 11520 / 23040) sums shorter chains; the
emulation over-estimates the engine's rounding there and the 1280-wide cases sit at 0.15 ... 0.25 of their bound in dtypes 3 and 7.  The planted defects
are three to six orders of magnitude outside those bounds (tests/test_cpu_unet_block_ref.py).

What the refiner cases (RF_CASES) reach that no base case does -- tests/test_cpu_unet_block_ref.py asserts it on the selection (csrc/select.cpp) itself:
self-attention with 12 / 24 heads (never the mixed-block kernel: the key-split kernel at 256 / 1024 queries, the 128-query kernel at 252 / 1008);
eight-slice split-K (igemm_splitk_slices: one entry has at most 256 rows) on whole tiles with the statistics from the epilogue (rf_rest_1536), on a
ragged 252-row tile (rf_res_1536_deep_bucket, rf_middle_1536_bucket) and on 64 rows (rf_out_3072, rf_down_1536), three slices at N = 1536 on whole and
ragged rows; ResU entries with the folded (16 x 16) and the gather (18 x 14: phase_shape_ok refuses it) upsample; K = 3456 ... 27648, N = 384 / 768 / 1536."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import config as OC, model as OM

CFG = OC.UNetConfig(2816, 320, [1, 2, 4], 64, [0, 2, 2], 2048)
RF_CFG = OC.UNetConfig(2560, 384, [1, 2, 4, 4], 64, [0, 2, 2, 2], 1280, is_refiner=True)
CONFIGS = {"base": CFG, "refiner": RF_CFG}
N_CTX = 77
B = 2
F16W_CLASSES = 1 | 2 | 4 | 8 | 16 | 32 | 128 | 256 | 512      # what a SDXL_DTYPE_F32_SPLIT_MIX_F16W model reports (tests/test_gpu_models.py)
MIX_EXPECTED = {5: F16W_CLASSES, 7: 4096 | 512 | 256}           # sdxl_unet_mix_classes per dtype (0 for the others): a silent fallback does not pass for the mode
ALL_CLASSES = frozenset(("conv_res", "conv_skip", "conv_io", "conv_updown", "conv_proj", "qkv", "attn", "out1", "out2", "q2", "xkv", "xattn", "geglu", "ff"))
_MIX_BITS = ((1, "attn"), (2, "geglu"), (4, "qkv"), (4, "attn"), (8, "ff"), (16, "out1"), (32, "out2"), (128, "q2"))


class Mode:
    def __init__(self, name, classes=frozenset(), stream16=False, h16=False, split=False, f16w=False, margin=4.0, kc=0):
        self.name, self.classes, self.stream16, self.h16, self.split, self.f16w, self.margin = name, frozenset(classes), stream16, h16, split, f16w, margin
        self.kc = kc      # depth of one accumulation step of the fp32-class GEMMs (0: the CPU's own summation)


def mode_of(dtype, mix=None):
    """the arithmetic of an engine dtype; dtype 5 takes the classes from the MixClass bits (default: the mode's own)"""
    if dtype == 5:
        bits = F16W_CLASSES if mix is None else mix
        return Mode("mix5", {c for b, c in _MIX_BITS if bits & b}, split=True, f16w=True, margin=2.0, kc=16)
    return {0: Mode("f32", kc=2), 1: Mode("f16", ALL_CLASSES, stream16=True, h16=True, margin=2.0), 2: Mode("f16_f32res", ALL_CLASSES, h16=True, margin=2.0),
            3: Mode("split", split=True, kc=16), 7: Mode("split_f16w", split=True, f16w=True, kc=16)}[dtype]


# (name, section, index, h, w, magnitude)
CASES = (
    ("res_320", "input", 1, 16, 16, False),            # HW % 256 == 0: conv_in leaves norm_out's statistics in f16
    ("res_320_ragged", "input", 1, 8, 24, False),      # HW = 192: the statistics pass runs
    ("down_320", "input", 3, 16, 16, False),           # stride-2 convolution into a concat slice
    ("rest_640_skip", "input", 4, 16, 16, False),      # 320 -> 640 with the 1x1 skip, transformer depth 2, 10 heads
    ("rest_640_skip_mag", "input", 4, 16, 16, True),   # entry 1's inputs 2^10 times entry 0's (not in dtype 1: an f16 stream cannot hold it)
    ("rest_1280", "input", 8, 32, 32, False),          # the base model's level-2 shape for a CFG pair: K = 11520, M = 2048
    ("rest_1280_bucket", "input", 8, 36, 28, False),   # HW = 1008 (the 1152 x 896 bucket): padded V^T, zero fill, un-fused cross-attention
    ("middle_1280", "middle", 0, 16, 16, False),
    ("out_2560", "output", 0, 16, 16, False),          # concat-width input, K = 23040
    ("out_1920_up", "output", 2, 16, 16, False),       # + the folded upsample convolution
    ("out_960_res", "output", 6, 16, 16, False),       # widest skip ratio, no transformer
    ("head", "head", 0, 16, 16, False),                # N = 4
)
# the refiner configuration's cases (rows of one entry decide split-K: <= 256 rows eight slices, <= 1024 three; statistics from the epilogue on whole 256-row tiles)
RF_CASES = (
    ("rf_res_384", "input", 1, 16, 16, False),               # N = 384: 12 channels per GroupNorm group, K = 3456
    ("rf_rest_768_skip", "input", 4, 16, 16, False),         # 384 -> 768 with the 1x1 skip, 12 heads
    ("rf_rest_768_skip_mag", "input", 4, 16, 16, True),      # entry 1 at 2^10 x (not in dtype 1, as in the base)
    ("rf_rest_1536_skip", "input", 7, 32, 32, False),        # 768 -> 1536, 24 heads at 1024 queries, three-slice split-K + producer statistics at N = 1536
    ("rf_rest_1536", "input", 8, 16, 16, False),             # eight slices + producer statistics, 24 heads at 256 queries
    ("rf_rest_1536_bucket", "input", 8, 36, 28, False),      # HW = 1008: padded V^T, three slices on ragged rows, the statistics pass
    ("rf_down_1536", "input", 9, 16, 16, False),             # stride-2 convolution, K = 13824, M = 128
    ("rf_res_1536_deep", "input", 10, 16, 16, False),        # level 3 (no transformer) at its 1024^2 size
    ("rf_res_1536_deep_bucket", "input", 11, 18, 14, False),  # 252 rows: eight slices on one ragged tile that spans both entries
    ("rf_middle_1536_bucket", "middle", 0, 18, 14, False),   # 252 queries / keys, 24 heads, both ResBlocks ragged
    ("rf_out_3072", "output", 0, 8, 8, False),               # K = 27648, 64 rows per entry (statistics-buffer quotient h w / 256 = 0)
    ("rf_out_3072_up", "output", 2, 16, 16, False),          # ResU: the folded phase upsample
    ("rf_out_3072_up_bucket", "output", 2, 18, 14, False),   # ResU: the gather upsample (Hin Win % 128 != 0)
    ("rf_out_2304", "output", 6, 16, 16, False),             # 2304 -> 768 + transformer, K = 20736
    ("rf_out_1152_res", "output", 9, 16, 16, False),         # 1152 -> 384
    ("rf_head", "head", 0, 16, 16, False),                   # K = 3456, N = 4
)
CONFIG_OF = {**{c[0]: "base" for c in CASES}, **{c[0]: "refiner" for c in RF_CASES}}      # case name -> key of CONFIGS
ALL_DTYPES = (0, 1, 3)
TRANSFORMER_DTYPES = (2, 5, 7)

# defect -> (case, dtype) it is planted on
DEFECTS = {
    "emb_slice_neighbour": ("res_320", 0),          # the next ResBlock's emb_off slice
    "emb_other_entry": ("res_320", 0),
    "skip_dropped": ("out_960_res", 0),             # x (its first C_out channels) added where skip(x) belongs
    "one_scale": ("rest_640_skip_mag", 3),          # entry 0's operand scale for both entries
    "norm_out_stats_in": ("res_320", 1),            # norm_out normalised with norm_in's statistics
    "stale_ln_stats": ("rest_640_skip", 1),         # block 1's norm1 with the statistics of the stream before block 0's FF-out
    "ctx_other_entry": ("rest_640_skip", 0),
    "ctx_pad_live": ("rest_640_skip", 0),           # keys 77..95 of the padded context (zero rows) take part in the softmax
    "vt_pad_nonzero": ("rest_1280_bucket", 1),      # V^T padding behind key 1008 not zero (P = 0 there: 0 x inf)
    "geglu_swapped": ("rest_640_skip", 0),
    "proj_out_no_residual": ("rest_640_skip", 0),
    "dst_col0": ("down_320", 0),                    # written at column 0 of the concat buffer: the slice that is read back was never written
    # the refiner plan: the layout defects where four levels move the offsets ("rf/": the same defect, planted on a refiner case) ...
    "rf/emb_slice_neighbour": ("rf_res_1536_deep", 0),
    "rf/stale_ln_stats": ("rf_rest_1536", 1),
    "rf/ctx_pad_live": ("rf_rest_768_skip", 0),
    "rf/vt_pad_nonzero": ("rf_middle_1536_bucket", 1),      # 252 keys: 4 padded columns
    "rf/skip_dropped": ("rf_out_1152_res", 0),
    "rf/dst_col0": ("rf_down_1536", 0),
    "rf/one_scale": ("rf_rest_768_skip_mag", 3),
    # ... and three that only its shapes can show (dtype 1: the widest bounds of the case)
    "rf/splitk_slice_lost": ("rf_res_1536_deep_bucket", 1),  # the last of eight K slices missing from conv_out
    "rf/splitk_tail_rows": ("rf_res_1536_deep_bucket", 1),   # rows 248 ... 251 of each entry (the ragged end of its tile) get slice 0 of conv_out only
    "rf/head_width_128": ("rf_rest_1536", 1),                # self-attention over 1536 channels as 12 heads of 128
}


def case(name):
    return next(c for c in CASES + RF_CASES if c[0] == name)


def config(name):
    """the UNetConfig of the case's model"""
    return CONFIGS[CONFIG_OF[name]]


def has_transformer(name):
    return block_of(name)["kind"] in ("ResT", "ResTU", "ResTRes")


def case_dtypes(name):
    dts = ALL_DTYPES + (TRANSFORMER_DTYPES if has_transformer(name) else ())
    return tuple(d for d in sorted(dts) if not (case(name)[5] and d == 1))


_plan = {k: OC.unet_block_plan(c) for k, c in CONFIGS.items()}


def block_of(name):
    _, section, index, _, _, _ = case(name)
    cfg, plan = config(name), _plan[CONFIG_OF[name]]
    if section == "head":
        return dict(kind="Head", c_in=cfg.model_channels, c_out=cfg.out_channels)
    if section == "middle":
        m = plan[1]
        return dict(m, c_in=m["c"], c_out=m["c"])
    b = plan[0 if section == "input" else 2][index]
    return dict(b, c_in=b.get("c_in", b.get("c")), c_out=b.get("c_out", b.get("c")))


def prefix(name):
    _, section, index, _, _, _ = case(name)
    return {"input": f"input_blocks.{index}", "middle": "middle_block", "output": f"output_blocks.{index}", "head": ""}[section]


# ------------------------------------------------------------------------------------------------------------------ operands
_specs = {k: OC.unet_param_specs(c) for k, c in CONFIGS.items()}
_weights = {}


def _own(spec_name, p):
    return spec_name.startswith(p + ".") if p else (spec_name.startswith("norm_out.") or spec_name.startswith("conv_out."))


def _tensors(cfg_key, f16w, pick):
    W = {}
    for s in _specs[cfg_key]:
        if pick(s.name):
            v = torch.from_numpy(OC.synth_values(s.name, s.numel, s.scale, s.mean, 0).reshape(s.shape))
            W[s.name] = v.half().float() if f16w and not s.name.endswith(".eps") else v
    return W


def weights(name, f16w=False):
    """fp32 tensors of the case's own parameters + every lin_embed of its model, the latter in emb_off order and shared between the model's cases (seed
    0; f16w: rounded to f16 values, what SEED_F16_WEIGHTS gives the engine)"""
    k, p = CONFIG_OF[name], prefix(name)
    if (k, None, f16w) not in _weights:
        _weights[(k, None, f16w)] = _tensors(k, f16w, lambda n: ".lin_embed." in n)
    if (k, p, f16w) not in _weights:
        own = _tensors(k, f16w, lambda n: _own(n, p) and ".lin_embed." not in n)
        _weights[(k, p, f16w)] = {**own, **_weights[(k, None, f16w)]}
    return _weights[(k, p, f16w)]


_inputs = {}


def inputs(name, seed=0):
    """(x [B,c_in,h,w], emb [B,4 mc], context [B,77,ctx]) fp32, built once per (case, seed) and never modified.  x ~ unit variance with a per-channel
    offset; emb ~ 0.5 N(0,1).  The magnitude variant: entry 1's x, emb-independent, times 2^10 (a power of two: the reference stays exact)."""
    if (name, seed) not in _inputs:
        _, _, _, h, w, mag = case(name)
        g = torch.Generator().manual_seed(zlib.crc32(f"{name.replace('_mag', '')}/{seed}".encode()))
        r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        c_in = block_of(name)["c_in"]
        x = r(B, c_in, h, w) + 0.5 * r(1, c_in, 1, 1)
        emb, ctx = 0.5 * r(B, 4 * config(name).model_channels), r(B, N_CTX, config(name).context_dim)
        if mag:
            x[1] *= 2.0 ** 10
        _inputs[(name, seed)] = (x.contiguous(), emb.contiguous(), ctx.contiguous())
    return _inputs[(name, seed)]


# ------------------------------------------------------------------------------------------------------------------ references
def _oracle(name, x, emb, ctx, W):
    _, section, _, _, _, _ = case(name)
    b, p = block_of(name), prefix(name)
    if section == "head":
        return OM.conv2d(OM.silu(OM.gn(x, W, "norm_out")), W, "conv_out", padding=1, cls="conv_io")
    if section == "middle":
        x = OM.res_block(x, emb, W, p + ".res1")
        x = OM.spatial_transformer(x, ctx, W, p + ".transformer", b["n_head"], b["depth"])
        return OM.res_block(x, emb, W, p + ".res2")
    return OM._unet_block(x, emb, ctx, W, p, b)


_refs = {}


def ref64(name, seed=0, f16w=False):
    """the entry's output in fp64 (cached, never modified)"""
    if (name, seed, f16w) not in _refs:
        assert OM.NUM.mode is None
        x, emb, ctx = (t.double() for t in inputs(name, seed))
        out = _oracle(name, x, emb, ctx, {k: v.double() for k, v in weights(name, f16w).items()})
        assert out.dtype == torch.float64
        _refs[(name, seed, f16w)] = out
    return _refs[(name, seed, f16w)]


def oracle32(name):
    """the fp32 oracle on the same operands"""
    assert OM.NUM.mode is None
    return _oracle(name, *inputs(name), weights(name))


# ------------------------------------------------------------------------------------------------------------------ emulation
def f16(x):
    return x.half().float()


def _pow2_scale(absmax):
    """hl_stream_scale: the power of two that brings absmax into [2^13, 2^14)"""
    if not (absmax > 0.0 and math.isfinite(absmax)):
        return 1.0
    return 2.0 ** (14 - math.frexp(absmax)[1])


def _seq_mm(passes, kc):
    """sum over the passes (a [M,K], w [K,N]) of a @ w with the accumulator rounded to fp32 after every kc-deep step of every pass, k ascending: the
    accumulation chain of an MFMA k-loop (row blocks keep the accumulator in cache; the order within a step is the CPU's)"""
    (M, K), N = passes[0][0].shape, passes[0][1].shape[1]
    rb = max(64, (1 << 21) // N)
    out = torch.empty(M, N)
    for r0 in range(0, M, rb):
        acc = torch.zeros(min(rb, M - r0), N)
        for k0 in range(0, K, kc):
            for a, w in passes:
                acc.addmm_(a[r0:r0 + rb, k0:k0 + kc], w[k0:k0 + kc])
        out[r0:r0 + rb] = acc
    return out


def _gemm(m, a, w, cls):
    """a [M,K] @ w [K,N] as the mode's GEMM of class cls computes it"""
    if cls in m.classes:
        return f16(a) @ f16(w)
    if not m.kc:
        return a @ w
    if not m.split:
        return _seq_mm(((a, w),), m.kc)
    # (hi, lo) f16 halves, the weights after the power of two that brings max|w| into [2^13, 2^14) (WeightBuilder::hl_scale); a_l w_l is dropped
    sc = np.float32(_pow2_scale(float(w.abs().max())))
    ah, wh = f16(a), f16(w * sc)
    return _seq_mm(((ah, wh), (f16(a - ah), wh), (ah, f16(w * sc - wh))), m.kc) / sc


def _lin(m, x, W, name, cls):
    w = W[name + ".weight"]
    y = _gemm(m, x.reshape(-1, x.shape[-1]), w, cls).reshape(*x.shape[:-1], w.shape[1])
    return y + W[name + ".bias"] if name + ".bias" in W else y


def _conv(m, x, W, name, cls, stride=1, padding=0, a_scale=None):
    """a_scale [B,1,1,1] (split modes): the GEMM reads x times it and multiplies the inverse back per entry (IgemmParams::a_scale)"""
    w, b = W[name + ".weight"], W[name + ".bias"]
    if cls in m.classes or not m.kc:
        if cls in m.classes:
            x, w = f16(x), f16(w)
        return F.conv2d(x, w, b, stride=stride, padding=padding)
    Bn, _, H, Wd = x.shape
    k = w.shape[2]
    ho, wo = (H + 2 * padding - k) // stride + 1, (Wd + 2 * padding - k) // stride + 1
    cols = F.unfold(x if a_scale is None else x * a_scale, k, padding=padding, stride=stride).transpose(1, 2).reshape(Bn * ho * wo, -1)      # the implicit GEMM's A: [B h w, C k k]
    y = _gemm(m, cols, w.reshape(w.shape[0], -1).T.contiguous(), cls).reshape(Bn, ho * wo, -1)
    if a_scale is not None:
        y = y / a_scale.reshape(Bn, 1, 1)
    return (y + b).transpose(1, 2).reshape(Bn, -1, ho, wo)


def _stats(y):
    """(mean, biased variance) of the last dimension: what a statistics buffer carries"""
    mu = y.mean(-1, keepdim=True)
    return mu, ((y - mu) ** 2).mean(-1, keepdim=True)


def _norm(y, st, eps):
    return (y - st[0]) / torch.sqrt(st[1] + eps)


def _gn(x, W, p, silu, stats=None):
    Bn, C = x.shape[:2]
    y = x.reshape(Bn, 32, -1)
    y = _norm(y, stats or _stats(y), OM._eps(W, p)).reshape(x.shape) * W[p + ".gamma"].reshape(1, C, 1, 1) + W[p + ".beta"].reshape(1, C, 1, 1)
    return y * torch.sigmoid(y) if silu else y


def _ln(x, W, p, stats=None):
    return _norm(x, stats or _stats(x), OM._eps(W, p)) * W[p + ".gamma"] + W[p + ".beta"]


def _stream(m, x):
    return f16(x) if m.stream16 else x


def _attention(m, q, k, v, n_head, cls, defect=None, pad_keys=0):
    """oracle.model.qkv_attention; class on: q, k, v and the un-normalised P = exp(s - max) <= 1 rounded to f16.  pad_keys: that many further keys
    with zero K and V rows (a zero context row projects to zero: no bias) take part in the softmax."""
    if cls in m.classes:
        q, k, v = f16(q), f16(k), f16(v)
    Bn, nq, C = q.shape
    if pad_keys:
        k, v = (torch.cat([t, torch.zeros(Bn, pad_keys, C)], 1) for t in (k, v))
    nk, d = k.shape[1], C // n_head
    heads = lambda t, n: t.reshape(Bn, n, n_head, d).transpose(1, 2)      # noqa: E731
    s = (heads(q, nq) * d ** -0.25) @ (heads(k, nk) * d ** -0.25).transpose(-1, -2)
    p = torch.softmax(s, dim=3)
    vh = heads(v, nk)
    if cls in m.classes:
        mx = p.amax(dim=3, keepdim=True)
        o = f16(p / mx) @ vh * mx
    else:
        o = p @ vh
    if defect == "vt_pad_nonzero" and nk % 64:      # the tile behind the last key: P is 0 there, V^T is whatever the buffer held
        npad = 64 - nk % 64
        o = o + torch.zeros(Bn, n_head, nq, npad) @ torch.full((Bn, n_head, npad, d), math.inf)
    return o.transpose(1, 2).flatten(2, 3)


def _res_block(m, x, emb, W, p, defect=None):
    """ResBlock (unet/mod.rs:1082-1106) as UNet::res_block stores it"""
    Bn = x.shape[0]
    le = p + ".lin_embed"
    if defect == "emb_slice_neighbour":      # the slice of the ResBlock that follows in emb_off order with the same width
        names = [n[:-len(".weight")] for n in W if n.endswith(".lin_embed.weight")]      # (weights(): every lin_embed of the model, in emb_off order)
        c_out = W[le + ".weight"].shape[1]
        le = next(n for n in names[names.index(le) + 1:] + names[:names.index(le)] if W[n + ".weight"].shape[1] == c_out)
    e = F.silu(emb.flip(0) if defect == "emb_other_entry" else emb) @ W[le + ".weight"] + W[le + ".bias"]      # the fp32 GEMV over all ResBlocks
    st_in = _stats(x.reshape(Bn, 32, -1))
    h = _conv(m, _gn(x, W, p + ".norm_in", True, st_in), W, p + ".conv_in", "conv_res", padding=1) + e[:, :, None, None]
    if m.h16:
        h = f16(h)
    g = _gn(h, W, p + ".norm_out", True, st_in if defect == "norm_out_stats_in" else None)
    h = _conv(m, g, W, p + ".conv_out", "conv_res", padding=1)
    if defect in ("splitk_slice_lost", "splitk_tail_rows"):      # conv_out in eight K slices (K ordered C k k: a slice is an eighth of the channels)
        w, c8 = W[p + ".conv_out.weight"], h.shape[1] // 8
        part = lambda lo, hi: _conv(m, g[:, lo:hi], {"w.weight": w[:, lo:hi].contiguous(), "w.bias": W[p + ".conv_out.bias"]}, "w", "conv_res", padding=1)      # noqa: E731
        if defect == "splitk_slice_lost":
            h = part(0, 7 * c8)
        else:      # the last rows of each entry's (ragged) tile: only slice 0 arrived
            rows = h.flatten(2).clone()
            rows[:, :, -4:] = part(0, c8).flatten(2)[:, :, -4:]
            h = rows.reshape(h.shape)
    if p + ".skip_connection.weight" not in W:
        return _stream(m, x + h)
    if defect == "skip_dropped":
        c_out = h.shape[1]
        return _stream(m, (x[:, :c_out] if x.shape[1] >= c_out else F.pad(x, (0, 0, 0, 0, 0, c_out - x.shape[1]))) + h)
    sc = None
    if m.split:      # hl_operand: the (hi, lo) halves are those of x times one power of two per batch entry
        sc = [_pow2_scale(float(x[0 if defect == "one_scale" else b].abs().max())) for b in range(Bn)]
        sc = torch.tensor(sc, dtype=torch.float32).reshape(Bn, 1, 1, 1)
    # (the skip convolution writes the destination, conv_out reads it back as its residual operand -- UNet::res_block: run_conv(w.skip, ..., out, es);
    #  e2.R = out -- so an f16 stream rounds skip(x) on its own before the sum is rounded)
    return _stream(m, _stream(m, _conv(m, x, W, p + ".skip_connection", "conv_skip", a_scale=sc)) + h)


def _transformer(m, x, ctx, W, p, n_head, depth, defect=None):
    """SpatialTransformer (unet/mod.rs:820-845, 885-891) as UNet::spatial_transformer stores it: in place on the stream tensor x"""
    Bn, C, H, Wd = x.shape
    if defect == "ctx_other_entry":
        ctx = ctx.flip(0)
    t = _gn(x, W, p + ".norm", False).reshape(Bn, C, H * Wd).transpose(1, 2)
    t = _stream(m, _lin(m, t, W, p + ".proj_in", "conv_proj"))
    stale = None
    for j in range(depth):
        q = f"{p}.blocks.{j}"
        a = _ln(t, W, q + ".norm1", stale if defect == "stale_ln_stats" and j == 1 else None)
        a = _attention(m, *(_lin(m, a, W, f"{q}.attn1.{n}", "qkv") for n in ("query", "key", "value")), n_head // 2 if defect == "head_width_128" else n_head, "attn", defect)
        t = _stream(m, t + _lin(m, a, W, q + ".attn1.out", "out1"))
        a = _attention(m, _lin(m, _ln(t, W, q + ".norm2"), W, q + ".attn2.query", "q2"), _lin(m, ctx, W, q + ".attn2.key", "xkv"),
                       _lin(m, ctx, W, q + ".attn2.value", "xkv"), n_head, "xattn", pad_keys=96 - N_CTX if defect == "ctx_pad_live" else 0)
        t = _stream(m, t + _lin(m, a, W, q + ".attn2.out", "out2"))
        pr = _lin(m, _ln(t, W, q + ".norm3"), W, q + ".mlp.geglu.proj", "geglu")
        n = pr.shape[-1] // 2
        val, gate = (pr[..., n:], pr[..., :n]) if defect == "geglu_swapped" else (pr[..., :n], pr[..., n:])
        stale = _stats(t)      # the buffer a producer before FF-out filled: what block j + 1 reads if the ping-pong index is not flipped
        t = _stream(m, t + _lin(m, val * F.gelu(gate), W, q + ".mlp.lin", "ff"))
    t = _lin(m, t, W, p + ".proj_out", "conv_proj").transpose(1, 2).reshape(Bn, C, H, Wd)
    return _stream(m, t if defect == "proj_out_no_residual" else x + t)


def emulate(name, dtype, defect=None, seed=0, mix=None):
    """the entry's output [B,c_out,h_out,w_out] (fp32) in the arithmetic of `dtype`; defect: a key of DEFECTS ("rf/x" plants x)"""
    defect = defect and defect.rpartition("/")[2]
    m = mode_of(dtype, mix)
    _, section, _, _, _, _ = case(name)
    b, p, W = block_of(name), prefix(name), weights(name, m.f16w)
    x, emb, ctx = inputs(name, seed)
    k = b["kind"]
    if k == "Head":      # (the head's GroupNorm reads the stream; conv_out writes fp32)
        return _conv(m, _gn(_stream(m, x), W, "norm_out", True), W, "conv_out", "conv_io", padding=1)
    x = _stream(m, x)
    if k in ("Conv", "Down"):
        out = _stream(m, _conv(m, x, W, p, "conv_io" if k == "Conv" else "conv_updown", stride=2 if k == "Down" else 1, padding=1))
        return torch.zeros_like(out) if defect == "dst_col0" else out
    if k == "ResTRes":
        x = _res_block(m, x, emb, W, p + ".res1", defect)
        x = _transformer(m, x, ctx, W, p + ".transformer", b["n_head"], b["depth"], defect)
        return _res_block(m, x, emb, W, p + ".res2", defect)
    if k == "Res":
        return _res_block(m, x, emb, W, p, defect)
    x = _res_block(m, x, emb, W, p + ".res", defect)
    if k in ("ResT", "ResTU"):
        x = _transformer(m, x, ctx, W, p + ".transformer", b["n_head"], b["depth"], defect)
    if k in ("ResTU", "ResU"):
        x = _stream(m, _conv(m, OM.upsample_nearest2x(x), W, p + ".upsample.conv", "conv_updown", padding=1))
    return x


# ------------------------------------------------------------------------------------------------------------------ metric and bounds
def errors(out, name, seed=0, f16w=False):
    """per batch entry max|out - ref64| / max|ref64| (inf where out is not finite)"""
    ref = ref64(name, seed, f16w)
    o = out.double()
    return [float((o[b] - ref[b]).abs().max() / ref[b].abs().max()) if bool(torch.isfinite(o[b]).all()) else math.inf for b in range(ref.shape[0])]


_emu = {}


def emulation_errors(name, dtype, seed=0):
    if (name, dtype, seed) not in _emu:
        _emu[(name, dtype, seed)] = errors(emulate(name, dtype, seed=seed), name, seed, mode_of(dtype).f16w)
    return _emu[(name, dtype, seed)]


def bounds(name, dtype):
    """([bound per entry], [the emulation's own error per entry]): bound = margin of the mode x the emulation's error on this case"""
    e = emulation_errors(name, dtype)
    return [mode_of(dtype).margin * v for v in e], e
