"""Helpers of the adapter (LoRA) tests: a seeded adapter set in the usual PyTorch form (down.weight [r, in...], up.weight [out, r]), its
fp64 merge into oracle weights, and the per-element bound of the merge op's fixed fp32 arithmetic."""
import numpy as np
import torch

# (parameter-name suffix, which match, rank, strength): the first tensor whose name ends in the suffix unless `which` says otherwise.
#   attn1.query + attn1.value: two of the three tensors of the fused QKV matrix; attn2.key: the hoisted context K / V; mlp.geglu.proj: the GEGLU
#   interleave (and its (hi | lo) forms); mlp.lin: FF-out; conv_in: a ResBlock 3x3 convolution; skip_connection: a 1x1 convolution; proj_in: the
#   spatial transformer's 1x1 projection (an nn::Linear in the reference); lin2_time_embed: the time-embedding MLP on the GEMV path; lin_embed:
#   a ResBlock's slice of the fused embedding projection; the last two rows adapt attn1.query a SECOND time and reach the deepest level.
ADAPTERS = (
    (".attn1.query.weight", 0, 4, 1.0),
    (".attn1.value.weight", 0, 3, 1.0),
    (".attn2.key.weight", 0, 4, 1.0),
    (".mlp.geglu.proj.weight", 0, 5, 1.0),
    (".mlp.lin.weight", 0, 4, 1.0),
    (".conv_in.weight", 1, 4, 1.0),
    (".skip_connection.weight", 0, 3, 1.0),
    (".transformer.proj_in.weight", 0, 2, 1.0),
    ("lin2_time_embed.weight", 0, 2, 1.0),
    (".lin_embed.weight", 2, 2, 1.0),
    (".attn1.query.weight", 0, 2, -0.6),
    (".attn2.value.weight", -1, 3, 1.0),
)


def find(specs, suffix, which=0):
    """index of the `which`-th parameter whose name ends in `suffix`"""
    hits = [i for i, p in enumerate(specs) if p.name.endswith(suffix)]
    return hits[which]


def adapter_set(specs, magnitude, seed=7, rows=ADAPTERS):
    """[(param index, down [r, in...], up [out, r], alpha, strength)] as fp32 numpy arrays.  With unit-variance inputs, strength 1 and alpha = 2 r
    the adapter's branch up(down(x)) * alpha / r has standard deviation `magnitude` per output (the synthetic base layers have ~1)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for suffix, which, rank, strength in rows:
        i = find(specs, suffix, which)
        shape = tuple(specs[i].shape)
        if specs[i].kind == 1:      # SDXL_PARAM_CONV_W [Cout, Cin, kh, kw]
            d_out, fan_in, down_shape = shape[0], int(np.prod(shape[1:])), (rank,) + shape[1:]
        else:                       # SDXL_PARAM_LINEAR_W [d_in, d_out]
            d_out, fan_in, down_shape = shape[1], shape[0], (rank, shape[0])
        down = torch.randn(down_shape, generator=g) / np.sqrt(fan_in)
        up = torch.randn(d_out, rank, generator=g) * (magnitude / (2.0 * np.sqrt(rank)))
        out.append((i, down.numpy(), up.numpy(), 2.0 * rank, strength))
    return out


def left_right(spec, down, up):
    """(left [rows, r], right [r, cols]) of the parameter's matrix view (rows = shape[0]) -- the layout rule of include/sdxl_mi355.h"""
    down, up = np.asarray(down), np.asarray(up)
    r = down.shape[0]
    if spec.kind == 1:
        return up.reshape(up.shape[0], r), down.reshape(r, -1)
    return down.reshape(r, -1).T, up.reshape(up.shape[0], r).T


def merged_fp64(specs, W, adapters, round_f16=False):
    """oracle weights (name -> torch tensor) with the adapters merged in fp64 and cast to fp32 (optionally through f16)"""
    W = dict(W)
    acc = {}
    for i, down, up, alpha, strength in adapters:
        p = specs[i]
        left, right = left_right(p, down, up)
        scale = np.float32(strength * alpha / down.shape[0])
        cur = acc.get(i, W[p.name].double().reshape(left.shape[0], -1))
        acc[i] = cur + float(scale) * torch.from_numpy(left.astype(np.float64)) @ torch.from_numpy(right.astype(np.float64))
    for i, v in acc.items():
        v = v.float()
        W[specs[i].name] = (v.half().float() if round_f16 else v).reshape(tuple(specs[i].shape))
    return W


def merge_bound(w, left, right, scale):
    """fp64 reference and per-element bound of  acc = fma chain over j ascending; w' = fma(scale, acc, w)  in fp32:
    |err| <= (rank + 2) 2^-24 (|w| + |scale| sum_j |left||right|) + one fp32 ulp of the result"""
    w, left, right = w.double(), left.double(), right.double()
    rank = left.shape[1]
    ref = w + scale * (left @ right)
    mag = w.abs() + abs(scale) * (left.abs() @ right.abs())
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 23.0)
    return ref, (rank + 2) * 2.0 ** -24 * mag + ulp
