"""The case matrix of tests/golden/weight_pack_bits.npz: every path of the weight packing (csrc/weights.cpp), seen through what the packed weights compute.

Shared by tools/record_weight_pack_fixture.py (which wrote the fixture, once, from the library of the commit BEFORE the six packing routines became
one), tests/test_gpu_weight_pack.py (every case again, bit for bit) and tests/test_cpu_weight_layout.py (the arena bytes through the device-free
layout pass, sdxl_debug_weight_layout).

Cases -- the smallest shapes at which each packing path is taken:
  unet/<config>/dt<d>[-f16w]   one forward of tiny_config / tiny_refiner_config on the probe inputs of test_unet_forward (B = 2, 16 x 16, 5 context tokens),
                               dtypes 0-7 on synthetic seed 0 (5, 6, 7: the fallback classes) and 5, 6, 7 on SEED_F16_WEIGHTS (their own classes)
  proj/...                     one LayerNorm-fed projection through transformer_projection per distinct (projection, form, producer form, path) of
                               tests/test_gpu_forms.py::CASES (+ F16_WHILO, which that list leaves to a test of its own), f16-valued weights, 64 rows x
                               B = 2, C = 128; the X2 GEGLU pair at C = 640 (8 C % 640 == 0, and C % 128 == 0: at a narrower width its X2 producer has no
                               fragment-order image, so no shadow is ever left and the entry refuses the pair)
  f16/...                      the f16 engine's folded forms: layer_norm_linear plain / GEGLU, ln_query_cross_attention fused on / off (M = 64,
                               K = N = 128, 9 context tokens); linear for dtypes 0, 1, 3 at N = 200 (ragged Npad) and as GEGLU at N = 224 (the entry
                               takes GEGLU widths that are multiples of 32 only: the next ragged one)
  vae/dt<d>/{decode,encode}    tiny_vae_config: decode of an 8 x 8 latent (decoder-only model), encode of a 64 x 64 image (model with encoder)
  clip/<tower>/dt<d>           forward_hidden_pooled of the tiny CLIP towers
  full/...                     arena bytes only, of empty replicas (no packing work) at full size: base / refiner UNet dtypes 0-7, the SDXL VAE

Layout of the fixture (numpy .npz, deflate):
  meta                JSON: parent commit, hipcc version line, sdxl_build_info, case names, cases the parent did not reproduce (left out)
  sha/<case>/<out>    SHA-256 of an output's little-endian float32 bytes
  sample/<case>/<out> 256 values of it at a fixed stride (diagnosis: how far off, where)
  int/<case>/<what>   integers: arena_bytes, mix_classes, shadow_taken
"""
import hashlib
import json
import math

import numpy as np

UNET_CONFIGS = ("tiny", "tiny_refiner")
F16W_DTYPES = (5, 6, 7)
VAE_DTYPES = (0, 1, 3)          # tests/test_gpu_models.py
CLIP_DTYPES = (0, 1, 2)         # tests/test_gpu_clip.py
NATIVE, F16, WHILO, AHILO, X2 = 0, 1, 2, 3, 4
QKV, QUERY, GEGLU = 0, 1, 2
FORM_NAME = ("NATIVE", "F16", "WHILO", "AHILO", "X2")
PROJ_NAME = ("qkv", "q2", "geglu")
# (projection, form, producer form, path): tests/test_gpu_forms.py::CASES without its sizes, + WHILO
PROJ_FORMS = [
    (QKV, NATIVE, NATIVE, "ln"), (GEGLU, NATIVE, NATIVE, "ln"),
    (QKV, F16, F16, "ln"), (QKV, F16, F16, "sh"), (QUERY, F16, F16, "ln"), (QUERY, F16, F16, "sh"), (GEGLU, F16, F16, "ln"), (GEGLU, F16, F16, "sh"),
    (GEGLU, AHILO, F16, "ln"), (GEGLU, AHILO, F16, "sh"),
    (QKV, X2, X2, "sh"), (QUERY, X2, X2, "ln"), (QUERY, X2, X2, "sh"), (GEGLU, X2, X2, "ln"), (GEGLU, X2, X2, "sh"),
    (GEGLU, WHILO, NATIVE, "ln"),
]
SAMPLE = 256


def unet_cases():
    out = [dict(kind="unet", config=c, dtype=d, f16w=False) for c in UNET_CONFIGS for d in range(8)]
    return out + [dict(kind="unet", config=c, dtype=d, f16w=True) for c in UNET_CONFIGS for d in F16W_DTYPES]


def proj_cases():
    return [dict(kind="proj", proj=p, form=f, pform=pf, path=path, C=640 if (p, f) == (GEGLU, X2) else 128) for p, f, pf, path in PROJ_FORMS]


def f16_cases():
    out = [dict(kind="lnlin", geglu=g) for g in (False, True)] + [dict(kind="lnxattn", fused=f) for f in (True, False)]
    return out + [dict(kind="linear", dtype=d, geglu=g) for d in (0, 1, 3) for g in (False, True)]


def vae_cases():
    return [dict(kind="vae", dtype=d, encode=e) for d in VAE_DTYPES for e in (False, True)]


def clip_cases():
    return [dict(kind="clip", config=c, dtype=d) for c in ("tiny_clip", "tiny_open_clip") for d in CLIP_DTYPES]


def full_cases():
    out = [dict(kind="full_unet", config=c, dtype=d) for c in ("base", "refiner") for d in range(8)]
    return out + [dict(kind="full_vae", dtype=d, encode=e) for d in VAE_DTYPES for e in (False, True)]


def model_cases():
    """the cases that run a model or an op (1-5)"""
    return unet_cases() + proj_cases() + f16_cases() + vae_cases() + clip_cases()


def all_cases():
    return model_cases() + full_cases()


def case_name(c):
    k = c["kind"]
    if k == "unet":
        return f"unet/{c['config']}/dt{c['dtype']}" + ("-f16w" if c["f16w"] else "")
    if k == "proj":
        return f"proj/{PROJ_NAME[c['proj']]}-{FORM_NAME[c['form']]}-from-{FORM_NAME[c['pform']]}-{c['path']}-C{c['C']}"
    if k == "lnlin":
        return "f16/layer_norm_linear" + ("-geglu" if c["geglu"] else "")
    if k == "lnxattn":
        return "f16/ln_query_cross_attention-" + ("fused" if c["fused"] else "launch")
    if k == "linear":
        return f"f16/linear-dt{c['dtype']}" + ("-geglu" if c["geglu"] else "")
    if k in ("vae", "full_vae"):
        return ("vae" if k == "vae" else "full/vae") + f"/dt{c['dtype']}/" + ("encode" if c["encode"] else "decode")
    if k == "clip":
        return f"clip/{c['config']}/dt{c['dtype']}"
    return f"full/unet-{c['config']}/dt{c['dtype']}"


# ---------------------------------------------------------------------------------------------------------------- configs (host only)
def unet_config(pkg, name):
    from oracle import config as OC
    from util import to_pkg_cfg
    if name in ("base", "refiner"):
        return pkg.sdxl_base_config() if name == "base" else pkg.sdxl_refiner_config()
    return to_pkg_cfg(pkg, OC.tiny_config() if name == "tiny" else OC.tiny_refiner_config())


def vae_config(pkg, full):
    from oracle import config as OC
    from util import to_pkg_vcfg
    return pkg.VAEConfig() if full else to_pkg_vcfg(pkg, OC.tiny_vae_config())


def clip_config(pkg, name):
    from oracle import clip as OCL
    c = OCL.tiny_clip_config() if name == "tiny_clip" else OCL.tiny_open_clip_config()
    return pkg.CLIPConfig(c.n_vocab, c.n_state, c.embed_dim, c.n_head, c.n_ctx, c.n_layer, c.quick_gelu)


def layout_query(pkg, c, ints):
    """(model, config, dtype, option) of sdxl_debug_weight_layout for a case that records arena bytes, None for the op cases; ints: its recorded
    integers (a UNet passes the classes the record holds: the fallback rows are decided on the weights, which a layout pass never sees)"""
    k = c["kind"]
    if k in ("unet", "full_unet"):
        return "unet", unet_config(pkg, c["config"]), c["dtype"], ints["mix_classes"] if k == "unet" else -1
    if k in ("vae", "full_vae"):
        return "vae", vae_config(pkg, k == "full_vae"), c["dtype"], int(c["encode"])
    if k == "clip":
        return "clip", clip_config(pkg, c["config"]), c["dtype"], 0
    return None


# ---------------------------------------------------------------------------------------------------------------- running a case (GPU)
def digest(t):
    """(SHA-256 of the little-endian float32 bytes, 256 values at a fixed stride) of a tensor"""
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype="<f4").reshape(-1)
    return hashlib.sha256(a.tobytes()).hexdigest(), a[::max(1, a.size // SAMPLE)][:SAMPLE].copy()


def _seeded(*shape, seed):
    import torch
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _run_unet(pkg, ctx, c):
    import torch
    from oracle import config as OC
    cfg = unet_config(pkg, c["config"])
    B, H, W = 2, 16, 16
    x = torch.from_numpy(OC.arb_tensor(B, 4, H, W)).cuda()
    context = torch.from_numpy(OC.arb_tensor(B, 5, cfg.context_dim)).cuda()
    y = torch.from_numpy(OC.arb_tensor(B, cfg.adm_in_channels)).cuda()
    u = pkg.UNet(ctx, cfg, c["dtype"], seed=pkg.SEED_F16_WEIGHTS if c["f16w"] else 0)
    out = u.forward(x, torch.tensor([999, 1], dtype=torch.int32).cuda(), context, y)
    return {"out": out}, {"mix_classes": u.mix_classes(), "arena_bytes": u.weight_arena()[1]}


def _run_proj(pkg, ctx, c):
    C, rows, B, proj = c["C"], 64, 2, c["proj"]
    N, M, s = {QKV: 3 * C, QUERY: C, GEGLU: 8 * C}[proj], rows * B, 100 + 10 * proj + c["form"]
    f16v = lambda t: t.half().float()
    w = f16v(_seeded(C, N, seed=s + 6) / math.sqrt(C))
    producer = (_seeded(M, C, seed=s + 1).cuda(), f16v(_seeded(C, C, seed=s + 2) * (0.5 / math.sqrt(C))).cuda(), (0.1 * _seeded(C, seed=s + 3)).cuda(), c["pform"])
    out, t, took = pkg.transformer_projection(ctx, _seeded(M, C, seed=s).cuda(), (1 + 0.1 * _seeded(C, seed=s + 4)).cuda(), (0.1 * _seeded(C, seed=s + 5)).cuda(),
                                              w.cuda(), (0.1 * _seeded(N, seed=s + 7)).cuda(), proj, c["form"], 1e-5, c["path"] == "sh", producer, batch=B)
    return {"out": out, "t": t}, {"shadow_taken": int(took)}


def _run_f16(pkg, ctx, c):
    M, K = 64, 128
    x, gamma, beta = _seeded(M, K, seed=70).cuda(), (1 + 0.1 * _seeded(K, seed=71)).cuda(), (0.1 * _seeded(K, seed=72)).cuda()
    if c["kind"] == "lnxattn":
        k, v = _seeded(1, 9, K, seed=74).cuda(), _seeded(1, 9, K, seed=75).cuda()
        wq = (_seeded(K, K, seed=73) / math.sqrt(K)).cuda()
        return {"out": pkg.ln_query_cross_attention(ctx, x.reshape(1, M, K), gamma, beta, wq, k, v, fused=c["fused"])}, {}
    if c["kind"] == "lnlin":
        w, b = (_seeded(K, K, seed=76) / math.sqrt(K)).cuda(), (0.1 * _seeded(K, seed=77)).cuda()
        return {"out": pkg.layer_norm_linear(ctx, x, gamma, beta, w, b, geglu=c["geglu"], dtype=pkg.DTYPE_F16)}, {}
    N = 224 if c["geglu"] else 200
    w, b = (_seeded(K, N, seed=78) / math.sqrt(K)).cuda(), (0.1 * _seeded(N, seed=79)).cuda()
    return {"out": pkg.linear(ctx, x, w, b, geglu=c["geglu"], dtype=c["dtype"])}, {}


def _run_vae(pkg, ctx, c):
    ld = pkg.LatentDecoder(ctx, vae_config(pkg, False), c["dtype"], seed=0, with_encoder=c["encode"])
    if c["encode"]:
        out = ld.encode_image(_seeded(1, 3, 64, 64, seed=51).clamp(-1, 1).cuda())
    else:
        out = ld.decode_latent((_seeded(2, 4, 8, 8, seed=50) * 0.5).cuda())
    return {"out": out}, {"arena_bytes": ld.weight_arena()[1]}


def _run_clip(pkg, ctx, c):
    import torch
    m = pkg.CLIP(ctx, clip_config(pkg, c["config"]), c["dtype"], seed=5)
    ids = torch.randint(1, 49000, (2, 77), generator=torch.Generator().manual_seed(1), dtype=torch.int64)
    ids[:, 0] = 49406
    for b in range(2):
        ids[b, 3 + 5 * b] = 49407
        ids[b, 4 + 5 * b:] = 49407 if c["config"] == "tiny_clip" else 0
    hidden, pooled = m.forward_hidden_pooled(ids, m.num_layers() - 1)
    return {"hidden": hidden, "pooled": pooled}, {"arena_bytes": m.weight_arena()[1]}


def _run_full(pkg, ctx, c):
    if c["kind"] == "full_unet":
        d = pkg.Diffuser(ctx, unet_config(pkg, c["config"]), c["dtype"], empty=True)
        return {}, {"mix_classes": d.diffusion.mix_classes(), "arena_bytes": d.diffusion.weight_arena()[1]}
    ld = pkg.LatentDecoder(ctx, vae_config(pkg, True), c["dtype"], empty=True, with_encoder=c["encode"])
    return {}, {"arena_bytes": ld.weight_arena()[1]}


def run_case(pkg, ctx, c):
    """-> ({output name: (sha, sample)}, {integer name: value})"""
    run = {"unet": _run_unet, "proj": _run_proj, "lnlin": _run_f16, "lnxattn": _run_f16, "linear": _run_f16, "vae": _run_vae, "clip": _run_clip,
           "full_unet": _run_full, "full_vae": _run_full}[c["kind"]]
    outs, ints = run(pkg, ctx, c)
    return {k: digest(v) for k, v in outs.items()}, {k: int(v) for k, v in ints.items()}


# ---------------------------------------------------------------------------------------------------------------- the fixture
def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def load_meta(z):
    return json.loads(str(z["meta"]))


def recorded(z, c):
    """({output name: (sha, sample)}, {integer name: value}) of a case as the fixture holds it"""
    name = case_name(c)
    outs = {k[len("sha/" + name) + 1:]: (str(z[k]), z["sample/" + k[4:]]) for k in z if k.startswith("sha/" + name + "/")}
    ints = {k[len("int/" + name) + 1:]: int(z[k]) for k in z if k.startswith("int/" + name + "/")}
    return outs, ints
