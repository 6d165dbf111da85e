"""The fused cross-attention over a long context (csrc/igemm_common.h xattn_unit_long) as numpy arithmetic, and the inputs the CPU and GPU tests share.

`inputs` builds what pkg.ln_query_cross_attention takes; `emulate` restates the kernel's tail per head: q (with the softmax scale and log2 e
folded in), K, V, P and the stored output rounded to f16, fp32 accumulation, 96-key blocks, keys >= n_ctx masked by the block's key offset, the
running maximum / row sum / output rescaled by exp2(m - m') in fp32, one multiply by 1 / l at the end.  `defect` plants one of the bugs the blocked form
invites, so that the CPU test can show the chosen inputs expose each of them far outside the GPU test's bound:
    "skip_rescale"   the running output and row sum are not rescaled when the maximum rises
    "mask_no_offset" the key mask compares the key's index INSIDE its block with n_ctx (the short form's mask, copied)
    "drop_last"      the last block is never visited
    "l_not_rescaled" the output is rescaled, the row sum is not
"""
import math

import numpy as np
import torch

from util import seeded

TOL_F16 = 4e-3          # TOL[1] of tests/test_gpu_ops.py: one f16 rounding of the operands plus the f16 rounding of the stored result
BLOCK = 96
DEFECTS = ("skip_rescale", "mask_no_offset", "drop_last", "l_not_rescaled")

# (B, Nq, Nk, C, variant): the shapes of tests/test_gpu_xattn_long.py.  variant = forced tile height ("igemm_variant": 60 = 96 rows, 62 = 64 rows, 0 = auto)
SHAPES = [
    (2, 64, 97, 128, 60), (2, 64, 97, 128, 62),        # second block holds one key; the 96-row tile straddles two entries
    (2, 64, 154, 128, 60), (2, 64, 154, 128, 62),      # two chunks
    (1, 128, 192, 128, 60),                            # two full blocks, nothing masked
    (1, 64, 193, 128, 62),                             # third block holds one key
    (3, 64, 231, 256, 60),                             # three entries, three chunks
    (1, 64, 384, 128, 62),                             # the maximum key count
    (2, 256, 308, 1280, 0),                            # production width, four chunks
    (2, 1024, 154, 1280, 0), (1, 4096, 154, 640, 0),   # the step's own launches at the 32^2 / 64^2 levels
]
UNDERFLOW = (2, 64, 231, 128, 60)                      # + a last-block key scaled x 8: the earlier blocks' weights underflow towards 0


def boosted_key(Nk, kind):
    """index of the key an entry scales: in the first block, the last live key, or inside a middle block"""
    nb = (Nk + BLOCK - 1) // BLOCK
    return {"first": 0, "last": Nk - 1, "middle": min(BLOCK * (nb // 2) + 5, Nk - 1)}[kind]


def boost_kinds(B, rot):
    """one kind per entry, rotated from case to case: a maximum that rises late (forces the rescale) and one that never rises"""
    return [("last", "first", "middle")[(b + rot) % 3] for b in range(B)]


def inputs(B, Nq, Nk, C, seed=21, rot=0, factor=3.0, kinds=None):
    """(x, gamma, beta, wq, k, v) fp32 CPU tensors; x holds f16 values (the engine's stream)"""
    x = (seeded(B, Nq, C, seed=seed) * 1.5 + 0.2).half().float()
    gamma, beta = 1 + 0.1 * seeded(C, seed=5), 0.1 * seeded(C, seed=6)
    wq = seeded(C, C, seed=seed + 1) / math.sqrt(C)
    k, v = seeded(B, Nk, C, seed=seed + 2), seeded(B, Nk, C, seed=seed + 3)
    for b, kind in enumerate(kinds or boost_kinds(B, rot)):
        k[b, boosted_key(Nk, kind)] *= factor
    return x, gamma, beta, wq, k, v


def query_fp64(x, gamma, beta, wq, eps=1e-5):
    x = x.double()
    mu, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    return (((x - mu) / torch.sqrt(var + eps)) * gamma.double() + beta.double()) @ wq.double()


def attention_fp64(q, k, v):
    """softmax(q k^T / 8) v per 64-channel head; q [B, Nq, C], k / v [B, Nk, C] fp64 -> [B, Nq, C] fp64"""
    B, Nq, C = q.shape
    H = C // 64
    qh, kh, vh = (t.double().reshape(B, -1, H, 64).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * 0.125, dim=-1)
    return (p @ vh).transpose(1, 2).reshape(B, Nq, C)


def _f16(a):
    return a.astype(np.float16).astype(np.float32)


def emulate(q, k, v, defect=None):
    """the blocked arithmetic on fp64 q [B, Nq, C] (un-scaled), k / v [B, Nk, C] -> [B, Nq, C] fp32 holding f16 values"""
    B, Nq, C = q.shape
    Nk, H = k.shape[1], C // 64
    nb = (Nk + BLOCK - 1) // BLOCK
    sc = np.float32(0.125) * np.float32(1.44269504088896340736)
    qs = _f16((q.numpy() * np.float64(sc)).astype(np.float32)).reshape(B, Nq, H, 64).transpose(0, 2, 1, 3)          # [B, H, Nq, 64]
    pad = nb * BLOCK - Nk
    kp = np.pad(_f16(k.numpy().astype(np.float32)), ((0, 0), (0, pad), (0, 0))).reshape(B, nb * BLOCK, H, 64).transpose(0, 2, 1, 3)
    vp = np.pad(_f16(v.numpy().astype(np.float32)), ((0, 0), (0, pad), (0, 0))).reshape(B, nb * BLOCK, H, 64).transpose(0, 2, 1, 3)
    m = np.zeros((B, H, Nq, 1), np.float32)
    l = np.zeros((B, H, Nq, 1), np.float32)
    o = np.zeros((B, H, Nq, 64), np.float32)
    for b in range(nb - 1 if defect == "drop_last" else nb):
        kb, vb = kp[:, :, b * BLOCK:(b + 1) * BLOCK], vp[:, :, b * BLOCK:(b + 1) * BLOCK]
        s = np.matmul(qs, kb.transpose(0, 1, 3, 2), dtype=np.float32)                                              # [B, H, Nq, 96]
        key = np.arange(BLOCK) + (0 if defect == "mask_no_offset" else b * BLOCK)
        s = np.where(key >= Nk, np.float32(-np.inf), s)
        mb = s.max(-1, keepdims=True)
        if b == 0:
            m = mb
        else:
            mn = np.maximum(m, mb)
            alpha = np.exp2(m - mn).astype(np.float32)
            if defect != "skip_rescale":
                o = o * alpha
                if defect != "l_not_rescaled":
                    l = l * alpha
            m = mn
        p = np.exp2(s - m).astype(np.float32)
        l = l + p.sum(-1, keepdims=True, dtype=np.float32)
        o = o + np.matmul(_f16(p), vb, dtype=np.float32)
    out = _f16(o * (np.float32(1.0) / l))
    return torch.from_numpy(out.transpose(0, 2, 1, 3).reshape(B, Nq, C).copy())
