"""fp64 references, CPU emulations of each dtype's documented arithmetic, plantable defects, case tables and input builders for one CLIP encoder layer
(ResidualDecoderAttentionBlock) and the pooled head, as csrc/clip.cpp runs them (ClipText::block / ClipText::run).  torch / numpy on the CPU; no GPU, no
engine.  tests/test_gpu_clip_layer.py builds one-layer CLIP models from the operands made here (the token table holds the case's input rows, the ids
index them) and holds the GPU to the bounds; tests/test_cpu_clip_layer_ref.py shows on the same operands that each planted defect leaves them.

References (fp64, following oracle/clip.py::_block / forward_hidden_pooled): pre-LN block, heads of 64 channels, scores times 1/8, additive causal
mask, GELU(erf) or x sigmoid(1.702 x); head = first index of the maximal id, LayerNorm of that row, text_projection without a bias.

Emulations (fp32 on the CPU; `mode` is the name of the dtype; cd = the compute dtype, f16 in the two f16-operand modes; sd = the stream dtype, f16 in
"f16" only).  Every rounding, with the line that performs it:
  tables      token and position table stored in cd: clip.cpp:25-26 (launch_copy_rows to cdt_; elementwise.hip st_f).
  embedding   sd(f32(tok[id]) + f32(pos[r % S])): elementwise.hip:512 (embed_tokens_kernel, one fp32 add, st_f to x.dt).
  LayerNorm   fp32 from what was stored (two passes: mean, then mean of (x - mean)^2; 1 / sqrtf(var + eps)), gamma / beta fp32, output stored in cd:
              norm.hip:469-492 (layernorm_cached_kernel; store8r).
  GEMMs       weights packed in cd (elementwise.hip pack_linear_kernel, round to nearest even), operands cd, fp32 accumulation, fp32 bias:
              igemm.hip:241-245.  "f32": the accumulator is a chain of K / 4 fp32 additions, one per v_mfma_f32_16x16x4f32 (igemm.hip:39-45, :223; _mm).  q | k stored in cd (igemm.hip:283 store_from_float), V^T stored in cd (igemm.hip:292, :300; igemm_common.h:657, :869).
  attention   "f16" / "f16_f32res": a mask sends f16 operands past the 32x32 family to attn_d64_f16_kernel (select.cpp:560 `!p.mask`, :607):
              Q pre-scaled once, q' = f16(f32(q) * sc) with sc = f32(0.125f * log2 e) (attention.hip:293); scores q' . k in fp32 plus mask * log2 e
              (:359); key tail -inf (:367); per 64-key tile a running maximum m, P = exp2(s - m) summed UNROUNDED into l (:383-387) and rounded to f16
              for the P V product (attention.hip:58 attn16_pv_f16); O = f16(acc * (1 / l)) (:83, :92).
              "f32": attn_d64_kernel<float> (select.cpp:608): scores (q . k) * sc in fp32 (attention.hip:209), P fp32, O fp32.
  residuals   out-projection and fc2: acc + bias + f32(stream) in fp32, one rounding to sd (igemm.hip:281-283; igemm_common.h:493, :526), in place.
  activation  fp32 on acc + bias (igemm.hip:254-260: gelu_erf with erff, or v / (1 + expf(-1.702 v))), h stored in cd (:283).
  tap         the stream copied to fp32 (clip.cpp:122, :125): exact.
  head        argmax_rows (first of tied maxima, elementwise.hip:526-531), gather to fp32 (:542, exact), LayerNorm fp32 -> fp32 (clip.cpp:130, nothing
              rounded), GEMV x fp32 times f32(cd(text_projection)) in fp32 (elementwise.hip:65, :79).

Bounds: nothing is fixed in advance and nothing comes from a GPU.  bound(case, mode) = MARGIN[mode] x (error of that mode's emulation against fp64 on
the case's operands).  MARGIN is vae_block_ref's: 4 for f32 (another summation order, MFMA-internal rounding, expf / erff / exp2 of a few ulps), 2 for
the two f16-operand modes (operand rounding, which the emulation reproduces, dominates there).

Error metrics, per batch entry: layer max|out - ref| / max|ref - x| (x the embedding: the branch, not the residual passing through); pooled vector
max|out - ref| / max|ref|.

Inputs: layer weights are seeded from the width, token rows / position table / ids from the case name and the width; all built once and never modified.
Token rows ~ unit variance + a per-channel offset, two outlier channels at +30 and -30 (real CLIP streams have such near-constant channels: they carry
the LayerNorm statistics and cost an f16 stream its low bits); both tables are f16 values, so that storing them in the compute dtype is exact in every
mode and the reference sees the operands the engine sees (the table conversion itself is tested bit for bit on unrounded rows); gamma 1 +- 0.2; q / k weights ~ N(0,1) 1.6 / sqrt(C) for scores of std 2 ... 3 (a flat softmax hides every
attention defect); fc1 ~ N(0,1) 1.5 / sqrt(C): pre-activations to |v| ~ 6, both tails of the activation; v / out / fc2 ~ N(0,1) / sqrt(fan_in): branches
of the size of the non-outlier stream.  Weight sets: "full"; "attn_only" (fc2 weight and bias zero); "mlp_only" (out-projection weight and bias
zero); "head" (both: the final stream is the embedding exactly, the pooled head is tested alone)."""
import math
import zlib

import numpy as np
import torch

MODES = {0: "f32", 1: "f16", 2: "f16_f32res"}      # SDXL_DTYPE_F32, _F16, _F16_F32RES
MARGIN = {"f32": 4.0, "f16": 2.0, "f16_f32res": 2.0}
WIDTHS = {768: (12, True), 1280: (20, False)}      # n_state -> (heads, QuickGELU): CLIP-L, OpenCLIP bigG
N_CTX = 77
EPS = 1e-5
LOG2E = 1.44269504088896340736
WSETS = ("full", "attn_only", "mlp_only", "head")

# (name, B, S, embed_dim or None for n_state, widths, weight set the case's bounds are made for)
CASES = (
    ("pair_77", 2, 77, None, (768, 1280), "full"),        # the production shape: row tiles straddle entries, keys padded to 128
    ("odd_77", 3, 77, None, (768, 1280), "full"),         # M = 231: M % 8 != 0, two entry boundaries inside one 256-row tile
    ("exact_64", 2, 64, None, (768, 1280), "full"),       # npad == S: no V^T zero fill, entries aligned to 4 keys
    ("short_9", 3, 9, None, (768, 1280), "full"),         # S < n_ctx: position r % S; one ragged key tile
    ("single_1", 1, 1, None, (768, 1280), "full"),        # M = 1; attention over one key returns V
    ("pool_9x77", 9, 77, None, (768, 1280), "head"),      # pooling GEMV in chunks of 8 + 1; EOT at 0, 76, the middle, tied maxima
    ("pool_embed_dim", 2, 16, 1280, (768,), "head"),      # embed_dim != n_state
)
# the embedding alone, bit for bit: unrounded tables (their conversion to the compute dtype is what is tested), ids with repeats, id 0 and id n_vocab - 1
EMBED_CASE = ("embed_3x9", 3, 9, None, (768, 1280), "full")
LAYER_CASES = tuple(c[0] for c in CASES if c[5] == "full")
POOL_CASES = tuple(c[0] for c in CASES if c[5] == "head")
# pool cases: entry -> EOT position, and entry -> later position that repeats the maximal id (the first wins)
POOL_EOT = {"pool_9x77": {0: 0, 1: 76, 2: 38, 3: 10, 4: 0, 5: 63, 6: 64, 7: 1, 8: 75}, "pool_embed_dim": {0: 5, 1: 15}}
POOL_TIES = {"pool_9x77": {3: 50, 4: 76, 8: 76}, "pool_embed_dim": {0: 11}}

DEFECTS = ("mask_shifted", "mask_off", "vt_group_entry", "key_tail_in_softmax", "heads_rotated", "scale_sqrt_c", "act_swapped", "residual_is_ln",
           "residual_dropped", "pos_by_row", "eot_last", "eot_plus_one", "pooled_without_ln")


def case(name):
    return next(c for c in CASES + (EMBED_CASE,) if c[0] == name)


def embed_dim(name, width):
    return case(name)[3] or width


def applies(defect, name, mode):
    """the cases at which a defect changes what the layer (weight set "full") or the head (weight set "head") computes, and the modes in which that
    change is held to leave the bound.  act_swapped is the one defect with a mode left out: GELU(erf) and QuickGELU differ by at most 0.021 (at |v| ~ 2),
    ~1 % of the MLP branch, and in "f16" the stream's own rounding on the +-30 channels (half an f16 spacing of 2^-5 against branches of ~5) sets a bound
    of that size -- 0.7 ... 1.3 x the bound there (2.0 at most with the attention knocked out), printed by test_cpu_clip_layer_ref.py.  The fc1 launch is the same in both f16-operand modes (f16 A,
    f16 weights, f16 h: the stream dtype does not reach it), so "f16_f32res", where the defect is 7 ... 9 x outside, covers that code.
    mask / scale / head-order defects need a second key (over one key attention returns V whatever the scores); vt_group_entry needs an entry boundary
    inside a 4-row group; the key tail exists where S is no multiple of the 64-key tile; pos_by_row needs a second entry whose flat rows are still inside
    the position table (beyond it the defect would read out of the table: nothing to emulate); eot_last needs tied maxima."""
    _, B, S, _, _, wset = case(name)
    layer = wset == "full"
    if mode not in MARGIN:
        return False
    return {"mask_shifted": layer and S > 1, "mask_off": layer and S > 1, "vt_group_entry": layer and B > 1 and S % 4 != 0,
            "key_tail_in_softmax": layer and S % 64 != 0, "heads_rotated": layer and S > 1, "scale_sqrt_c": layer and S > 1,
            "act_swapped": layer and mode != "f16", "residual_is_ln": layer, "residual_dropped": layer,
            "pos_by_row": B > 1 and B * S <= N_CTX,
            "eot_last": not layer and bool(POOL_TIES.get(name)), "eot_plus_one": not layer, "pooled_without_ln": not layer}[defect]


# ------------------------------------------------------------------------------------------------------------------ inputs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


_inputs = {}


def layer_weights(width, tag="block0"):
    """fp32 parameters of one block, the final LayerNorm included ([d_in, d_out] matrices, as the reference stores a Linear); seeded from the width"""
    key = ("w", width, tag)
    if key not in _inputs:
        C = width
        g = _gen(f"clip_layer/{width}/{tag}")
        r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        d = {}
        for n in ("attn_ln", "mlp_ln", "layer_norm"):
            d[n + ".gamma"], d[n + ".beta"] = 1.0 + 0.2 * r(C), 0.1 * r(C)
        for n, din, dout, sc in (("attn.query", C, C, 1.6), ("attn.key", C, C, 1.6), ("attn.value", C, C, 1.0), ("attn.out", C, C, 1.0),
                                 ("mlp.fc1", C, 4 * C, 1.5), ("mlp.fc2", 4 * C, C, 1.0)):
            d[n + ".weight"], d[n + ".bias"] = r(din, dout) * (sc / math.sqrt(din)), 0.1 * r(dout)
        _inputs[key] = {k: v.contiguous() for k, v in d.items()}
    return _inputs[key]


def weights(width, wset, tag="block0"):
    """layer_weights with the branches of the weight set knocked out"""
    assert wset in WSETS
    d = dict(layer_weights(width, tag))
    zero = {"full": (), "attn_only": ("mlp.fc2",), "mlp_only": ("attn.out",), "head": ("attn.out", "mlp.fc2")}[wset]
    for n in zero:
        d[n + ".weight"], d[n + ".bias"] = torch.zeros_like(d[n + ".weight"]), torch.zeros_like(d[n + ".bias"])
    return d


def text_projection(width, E):
    key = ("p", width, E)
    if key not in _inputs:
        _inputs[key] = (torch.randn(width, E, generator=_gen(f"clip_layer/{width}/proj{E}")) / math.sqrt(width)).contiguous()
    return _inputs[key]


def case_inputs(name, width):
    """tok [B S, C] (the case's input rows = the model's token table, n_vocab = B S), pos [n_ctx, C], ids [B, S] int64: a permutation of the rows; in the
    pool cases each entry's maximal id is moved to its POOL_EOT position and repeated at its POOL_TIES position.  EMBED_CASE: see there."""
    key = ("c", name, width)
    if key not in _inputs:
        _, B, S, _, _, _ = case(name)
        C, n = width, B * S
        g = _gen(f"clip_layer/{name}/{width}")
        r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        tok = r(n, C) + 0.5 * r(1, C)
        out_ch = torch.randperm(C, generator=g)[:2]
        tok[:, out_ch] += torch.tensor([30.0, -30.0])
        tok, pos = f16(tok), f16(0.3 * r(N_CTX, C))
        ids = torch.randperm(n, generator=g).reshape(B, S)
        if name == EMBED_CASE[0]:
            tok, pos = r(n, C) + 0.5 * r(1, C), 0.3 * r(N_CTX, C)
            tok[:, out_ch] += torch.tensor([30.0, -30.0])
            ids = torch.randint(0, n, (B, S), generator=g)
            ids[0, 0], ids[2, 8], ids[1, 5] = 0, n - 1, ids[1, 4]
        for b, e in POOL_EOT.get(name, {}).items():
            p = int(ids[b].argmax())
            ids[b, p], ids[b, e] = ids[b, e].clone(), ids[b, p].clone()
        for b, t in POOL_TIES.get(name, {}).items():
            ids[b, t] = ids[b].max()
        _inputs[key] = {"tok": tok.contiguous(), "pos": pos.contiguous(), "ids": ids.contiguous()}
    return _inputs[key]


def model_weights(name, width, wset, n_layer=1):
    """name -> numpy fp32, the parameter names of clip_param_specs for a tower of n_layer blocks on the case's tables (block 0: the weight set; further
    blocks: full blocks of their own seed)"""
    c = case_inputs(name, width)
    W = {"token_embedding.weight": c["tok"], "position_embedding": c["pos"], "text_projection": text_projection(width, embed_dim(name, width))}
    for i in range(n_layer):
        for k, v in (weights(width, wset) if i == 0 else weights(width, "full", f"block{i}")).items():
            if k.startswith("layer_norm"):
                if i == 0:
                    W[k] = v
            else:
                W[f"blocks.{i}.{k}"] = v
    for k in [k for k in W if k.endswith(".gamma")]:
        W[k[:-6] + ".eps"] = torch.tensor([EPS], dtype=torch.float32)
    return {k: v.numpy() for k, v in W.items()}


# ------------------------------------------------------------------------------------------------------------------ fp64 references
def _ln64(x, g, b):
    u = x - x.mean(-1, keepdim=True)
    return u / torch.sqrt((u * u).mean(-1, keepdim=True) + EPS) * g + b


def _heads(t, H):
    """[B,S,C] -> [B,H,S,64]"""
    B, S, C = t.shape
    return t.reshape(B, S, H, C // H).transpose(1, 2)


def _act64(v, quick):
    return v * torch.sigmoid(1.702 * v) if quick else 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def first_argmax(ids):
    return (ids == ids.max(-1, keepdim=True).values).to(torch.int64).argmax(-1)


_refs = {}


def ref(name, width, wset):
    """{"x": embedding, "out": stream after the layer [B,S,C], "pooled": [B,E], "scores": [B,H,S,S] before the mask} in fp64: computed once, shared,
    never modified"""
    key = (name, width, wset)
    if key not in _refs:
        H, quick = WIDTHS[width]
        c = case_inputs(name, width)
        w = {k: v.double() for k, v in weights(width, wset).items()}
        ids = c["ids"]
        B, S = ids.shape
        x = c["tok"].double()[ids] + c["pos"].double()[:S]
        lin = lambda t, n: t @ w[n + ".weight"] + w[n + ".bias"]      # noqa: E731
        h = _ln64(x, w["attn_ln.gamma"], w["attn_ln.beta"])
        q, k, v = (_heads(lin(h, "attn." + n), H) for n in ("query", "key", "value"))
        scores = q @ k.transpose(-1, -2) * 0.125
        mask = torch.full((S, S), -math.inf, dtype=torch.float64).triu(1)
        o = (torch.softmax(scores + mask, -1) @ v).transpose(1, 2).reshape(B, S, width)
        y = x + lin(o, "attn.out")
        if not _knocked_out(w, "mlp.fc2"):      # (knocked out: the branch is exactly 0)
            y = y + lin(_act64(lin(_ln64(y, w["mlp_ln.gamma"], w["mlp_ln.beta"]), "mlp.fc1"), quick), "mlp.fc2")
        sel = y[torch.arange(B), first_argmax(ids)]
        pooled = _ln64(sel, w["layer_norm.gamma"], w["layer_norm.beta"]) @ text_projection(width, embed_dim(name, width)).double()
        _refs[key] = {"x": x, "out": y, "pooled": pooled, "scores": scores}
    return _refs[key]


# ------------------------------------------------------------------------------------------------------------------ emulations
def f16(x):
    return x.half().float()


def _cd(mode, x):
    return x if mode == "f32" else f16(x)


def _sd(mode, x):
    return f16(x) if mode == "f16" else x


def _ln32(x, g, b):
    C = x.shape[-1]
    u = x - x.sum(-1, keepdim=True) / np.float32(C)
    rstd = 1.0 / torch.sqrt((u * u).sum(-1, keepdim=True) / np.float32(C) + np.float32(EPS))
    return u * rstd * g + b


def _act32(v, quick):
    return v / (1.0 + torch.exp(np.float32(-1.702) * v)) if quick else 0.5 * v * (1.0 + torch.erf(v * np.float32(0.70710678118654752440)))


def _mm(mode, a, w):
    """a [..,K] @ w [K,N] with fp32 accumulation.  "f32": the accumulator chain of igemm_kernel<float> -- every v_mfma_f32_16x16x4f32 adds the four
    products k = 16 s + 4 g + c (g = 0..3) of its step to the running fp32 accumulator (igemm.hip:39-45, :223), K / 4 roundings at the size of the
    partial sums, which over K = 3072 / 5120 (fc2) is the layer's largest fp32 error; a blocked CPU sum does not have it.  The f16-operand modes add 32
    products per MFMA and round their outputs to f16 or add them to an fp32 stream 2^13 coarser than this chain's error: plain matmul."""
    if mode != "f32":
        return a @ w
    K = a.shape[-1]
    idx = torch.arange(K).reshape(-1, 4, 4).transpose(1, 2).reshape(-1)      # [s][g][c] -> [s][c][g]: four consecutive entries = one MFMA
    ap, wp = a.reshape(-1, K)[:, idx].contiguous(), w[idx].contiguous()
    acc = torch.zeros(ap.shape[0], w.shape[1])
    for j in range(0, K, 4):
        acc += ap[:, j:j + 4] @ wp[j:j + 4]
    return acc.reshape(a.shape[:-1] + (w.shape[1],))


def embed_expected(tok, pos, ids, mode, by_row=False):
    """the stream after embed_tokens, bit for bit: sd(f32(cd(tok[id])) + f32(cd(pos[r % S])))"""
    B, S = ids.shape
    t = torch.arange(B * S).clamp(max=pos.shape[0] - 1).reshape(B, S) if by_row else torch.arange(S).expand(B, S)
    return _sd(mode, _cd(mode, tok)[ids] + _cd(mode, pos)[t])


def _attention(mode, q, k, v, S, npad, defect):
    """q, k [B,H,S,64], v [B,H,npad,64] (zero key tail) as stored -> O [B,H,S,64] as stored.  The kernels' 64-key tiles with their running maximum."""
    half = mode != "f32"
    scale = q.shape[1] ** -0.5 * 0.125 if defect == "scale_sqrt_c" else 0.125      # (H 64)^-1/2 = C^-1/2
    sc = np.float32(scale) * np.float32(LOG2E)
    if defect == "heads_rotated":
        k = torch.roll(k, 1, 1)
    s = (f16(q * sc) @ k.transpose(-1, -2)) if half else (q @ k.transpose(-1, -2)) * sc
    vis = 1 if defect == "mask_shifted" else 0
    if defect != "mask_off":
        s = s + torch.full((S, S), -math.inf).triu(1 + vis) * np.float32(LOG2E)
    tail = torch.full(s.shape[:-1] + (npad - S,), 0.0 if defect == "key_tail_in_softmax" else -math.inf)
    s = torch.cat([s, tail], -1)
    m = torch.full(s.shape[:-1] + (1,), -math.inf)
    l = torch.zeros_like(m)
    o = torch.zeros(q.shape)
    for t in range(npad // 64):
        st = s[..., t * 64:(t + 1) * 64]
        mnew = torch.maximum(m, st.max(-1, keepdim=True).values)
        msub = torch.where(mnew == -math.inf, torch.zeros_like(mnew), mnew)
        alpha = torch.exp2(m - msub)
        e = torch.exp2(st - msub)
        l = l * alpha + e.sum(-1, keepdim=True)
        o = o * alpha + (f16(e) if half else e) @ v[:, :, t * 64:(t + 1) * 64]
        m = mnew
    return _cd(mode, o * (1.0 / l))


def _knocked_out(w, n):
    return not bool(w[n + ".weight"].any()) and not bool(w[n + ".bias"].any())


def emulate(name, width, wset, mode, defect=None):
    """{"x": embedding as stored, "out": stream after the layer [B,S,C], "pooled": [B,E]} (fp32) of the one-layer model in `mode`"""
    H, quick = WIDTHS[width]
    if defect == "act_swapped":
        quick = not quick
    c = case_inputs(name, width)
    w = weights(width, wset)
    ids = c["ids"]
    B, S = ids.shape
    M, C = B * S, width
    npad = (S + 63) // 64 * 64
    lin = lambda a, n: _mm(mode, a, _cd(mode, w[n + ".weight"])) + w[n + ".bias"]      # noqa: E731
    x0 = embed_expected(c["tok"], c["pos"], ids, mode, by_row=defect == "pos_by_row")
    x = x0

    def residual(branch, x, ln):
        return _sd(mode, branch if defect == "residual_dropped" else branch + (ln if defect == "residual_is_ln" else x))

    # (a knocked-out projection -- weight and bias zero -- returns exactly 0 on finite operands: its branch is not computed)
    ln = _cd(mode, _ln32(x, w["attn_ln.gamma"], w["attn_ln.beta"]))
    if _knocked_out(w, "attn.out"):
        branch = torch.zeros(B, S, C)
    else:
        q, k, v = (_cd(mode, lin(ln, "attn." + n)) for n in ("query", "key", "value"))
        vt = torch.zeros(B, npad + 4, C)       # [b][key][channel]: V^T by its transposed index
        if defect == "vt_group_entry":
            rows = torch.arange(M)
            bb = (rows - rows % 4) // S
            vt[bb, rows - bb * S] = v.reshape(M, C)
        else:
            vt[:, :S] = v
        o = _attention(mode, _heads(q, H), _heads(k, H), _heads(vt[:, :npad], H), S, npad, defect)
        branch = lin(o.transpose(1, 2).reshape(B, S, C), "attn.out")
    x = residual(branch, x, ln)
    ln = _cd(mode, _ln32(x, w["mlp_ln.gamma"], w["mlp_ln.beta"]))
    branch = torch.zeros(B, S, C) if _knocked_out(w, "mlp.fc2") else lin(_cd(mode, _act32(lin(ln, "mlp.fc1"), quick)), "mlp.fc2")
    x = residual(branch, x, ln)
    # head
    if defect == "eot_last":
        eot = S - 1 - first_argmax(ids.flip(-1))
    else:
        eot = first_argmax(ids)
    flat = torch.arange(B) * S + eot
    if defect == "eot_plus_one":
        flat = (flat + 1) % M
    sel = x.reshape(M, C)[flat]
    seln = sel if defect == "pooled_without_ln" else _ln32(sel, w["layer_norm.gamma"], w["layer_norm.beta"])
    pooled = seln @ _cd(mode, text_projection(width, embed_dim(name, width)))
    return {"x": x0, "out": x, "pooled": pooled}


# ------------------------------------------------------------------------------------------------------------------ metrics and bounds
def layer_errors(out, name, width, wset):
    """per batch entry max|out - ref| / max|ref - x| (inf where out is not finite)"""
    r = ref(name, width, wset)
    o = out.double()
    return [float((o[b] - r["out"][b]).abs().max() / (r["out"][b] - r["x"][b]).abs().max()) if bool(torch.isfinite(o[b]).all()) else math.inf
            for b in range(o.shape[0])]


def pooled_errors(pooled, name, width, wset):
    """per batch entry max|pooled - ref| / max|ref|"""
    r = ref(name, width, wset)["pooled"]
    o = pooled.double()
    return [float((o[b] - r[b]).abs().max() / r[b].abs().max()) if bool(torch.isfinite(o[b]).all()) else math.inf for b in range(o.shape[0])]


_emu = {}


def _clean(name, width, wset, mode):
    key = (name, width, wset, mode)
    if key not in _emu:
        e = emulate(name, width, wset, mode)
        le = layer_errors(e["out"], name, width, wset) if wset != "head" else None
        _emu[key] = (le, pooled_errors(e["pooled"], name, width, wset))
    return _emu[key]


def layer_bounds(name, width, wset, mode):
    """([bound per entry], [emulation's error per entry]): bound = MARGIN[mode] x error of the mode's emulation on this case's operands"""
    e = _clean(name, width, wset, mode)[0]
    return [MARGIN[mode] * v for v in e], e


def pooled_bounds(name, width, wset, mode):
    e = _clean(name, width, wset, mode)[1]
    return [MARGIN[mode] * v for v in e], e
